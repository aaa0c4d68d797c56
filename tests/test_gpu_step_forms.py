"""Every device form of the box-game step (ggrs_amd/csrc/box_game.h, glibc_sincosf.h) against the
CPU oracle, one step from arbitrary states, bit for bit: no tolerance, no case skipped, every value
finite (so NaN equality never arises).  The harness tests/native/step_forms_kat_device.hip runs one
lane per case; the cases, their lane orders and what they cover are tests/step_form_cases.py's.

  test_step_form        advance_player_general / advance_player (dispatch) on classes 1-6,
                        _domain / _lean / _lean_sc / _rec / _rec_q on classes 1-5, two lane orders
  test_players_form     advance_players_lean<N> / advance_players_rec<N>, N = 1, 2, 4, 12
  test_state_form       advance_state<P> (with disconnects) / _lean<P> / _lean_k<P> + fletcher16_state<P>
  test_chain            8 steps, the next step's sin/cos computed inside the step's hook
  test_fletcher         fletcher16_state<P>, fletcher_from_doubled<kMad24>, fletcher16_state_host<P>
  test_domain_digest    glibc_sincosf_domain / _k / _raw / _raw_k over every f32 in [0, 2 pi]
  test_sincos_constants kSincosLiteral and sincos_consts_vgpr() against glibc's published constants
"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import step_form_cases as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
FIELDS = ("x", "y", "vx", "vy", "rot")
STEP_FORMS = {"general": 0, "dispatch": 1, "domain": 2, "lean": 3, "lean_sc": 4, "rec": 5, "rec_q": 6}
ANY_ROTATION = ("general", "dispatch")  # the forms that take a rotation outside [+0, 2 pi]


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


class Kat:
    """The harness.  Every entry returns the HIP error code of its copies and launch; the first
    nonzero code fails the test that met it and every later call fails without launching."""

    def __init__(self, so):
        L = ctypes.CDLL(so)
        P = ctypes.POINTER
        u8, u16, u32, u64, i64 = ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64
        L.kat_step.argtypes = [ctypes.c_int, i64, P(u32), P(u8), P(u32)]
        L.kat_players.argtypes = [ctypes.c_int, ctypes.c_int, i64, P(u32), P(u8), P(u32)]
        L.kat_state.argtypes = [ctypes.c_int, ctypes.c_int, i64, P(u32), P(u32), P(u32), P(u32), P(u16)]
        L.kat_chain.argtypes = [ctypes.c_int, i64, ctypes.c_int, P(u32), P(u8), P(u32)]
        L.kat_fletcher.argtypes = [ctypes.c_int, ctypes.c_int, i64, P(u32), P(u16), P(u16), P(u16)]
        L.kat_domain_digest.argtypes = [ctypes.c_int, u32, u32, P(u64)]
        L.kat_sincos_consts.argtypes = [P(ctypes.c_double), P(ctypes.c_double)]
        self.L = L
        self.failed = None

    def call(self, name, *args):
        if self.failed:
            pytest.fail(f"not launched: {self.failed}")
        rc = getattr(self.L, name)(*args)
        if rc != 0:
            self.failed = f"{name} returned HIP error code {rc}"
            pytest.fail(self.failed)

    def step(self, form, players, inputs):
        pl, inp = np.ascontiguousarray(players, np.uint32), np.ascontiguousarray(inputs, np.uint8)
        out = np.zeros_like(pl)
        self.call("kat_step", form, pl.shape[0], _p(pl, ctypes.c_uint32), _p(inp, ctypes.c_uint8), _p(out, ctypes.c_uint32))
        return out

    def players(self, form, players, inputs):
        pl, inp = np.ascontiguousarray(players, np.uint32), np.ascontiguousarray(inputs, np.uint8)
        out = np.zeros_like(pl)
        self.call("kat_players", form, pl.shape[1], pl.shape[0], _p(pl, ctypes.c_uint32), _p(inp, ctypes.c_uint8),
                  _p(out, ctypes.c_uint32))
        return out

    def state(self, form, P, words, packed, disc):
        w = np.ascontiguousarray(words, np.uint32)
        out, ck = np.zeros_like(w), np.zeros(w.shape[0], np.uint16)
        self.call("kat_state", form, P, w.shape[0], _p(w, ctypes.c_uint32), _p(packed, ctypes.c_uint32),
                  _p(disc, ctypes.c_uint32), _p(out, ctypes.c_uint32), _p(ck, ctypes.c_uint16))
        return out, ck

    def chain(self, form, players, inputs):
        pl, inp = np.ascontiguousarray(players, np.uint32), np.ascontiguousarray(inputs, np.uint8)
        out = np.zeros((pl.shape[0], inp.shape[1], 5), np.uint32)
        self.call("kat_chain", form, pl.shape[0], inp.shape[1], _p(pl, ctypes.c_uint32), _p(inp, ctypes.c_uint8),
                  _p(out, ctypes.c_uint32))
        return out

    def fletcher(self, P, mad24, words):
        w = np.ascontiguousarray(words, np.uint32)
        outs = [np.zeros(w.shape[0], np.uint16) for _ in range(3)]
        self.call("kat_fletcher", P, mad24, w.shape[0], _p(w, ctypes.c_uint32), *[_p(o, ctypes.c_uint16) for o in outs])
        return outs

    def sincos_consts(self):
        lit, vgpr = np.zeros(10, np.float64), np.zeros(10, np.float64)
        self.call("kat_sincos_consts", _p(lit, ctypes.c_double), _p(vgpr, ctypes.c_double))
        return lit, vgpr

    def domain_digest(self, form, lo, hi):
        out = ctypes.c_uint64()
        self.call("kat_domain_digest", form, lo, hi, ctypes.byref(out))
        return out.value


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    return Kat(C.compile_kat("step_forms_kat_device", tmp_path_factory.mktemp("step_forms_kat")))


@pytest.fixture(scope="module")
def prep(oracle):
    return C.prepared(oracle)


def _hex(row):
    return "[" + " ".join(f"{int(v):08x}" for v in row) + "]"


def assert_steps_equal(got, want, an, idx, what):
    """got / want [n][5] for the cases idx [n]: names the first differing lane, its case and the
    fields that differ, and counts the differing lanes by class and by field."""
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size == 0:
        return
    j = int(bad[0])
    k = int(idx[j])
    by_class = {C.CLASS_NAMES[c]: int((an["cls"][idx[bad]] == c).sum()) for c in C.CLASS_NAMES}
    by_field = {f: int((got[bad, q] != want[bad, q]).sum()) for q, f in enumerate(FIELDS)}
    pytest.fail(
        f"{what}: {bad.size} of {idx.size} lanes differ from the oracle.  First: lane {j} (wave {j // 64}, lane "
        f"{j % 64} of it), class '{C.CLASS_NAMES[int(an['cls'][k])]}', input 0x{int(an['inputs'][k]):02x}, "
        f"clamps {bool(an['clamp'][k])}, mag2 {float(an['mag2'][k])!r}, in {_hex(an['players'][k])}, oracle "
        f"{_hex(want[j])}, device {_hex(got[j])}, fields {[f for q, f in enumerate(FIELDS) if got[j, q] != want[j, q]]}."
        f"  Differing lanes by class {by_class}, by field {by_field}.")


@pytest.mark.parametrize("order", ["sorted", "interleaved"])
@pytest.mark.parametrize("form", list(STEP_FORMS))
def test_step_form(kat, prep, form, order):
    an = prep["an"]
    idx = prep["orders"]["all" if form in ANY_ROTATION else "lean", order]
    got = kat.step(STEP_FORMS[form], an["players"][idx], an["inputs"][idx])
    assert_steps_equal(got, an["ref"][idx], an, idx, f"{form}, order {order}")


@pytest.mark.parametrize("N", [1, 2, 4, C.MAX_PLAYERS_REC])
@pytest.mark.parametrize("form", ["players_lean", "players_rec"])
def test_players_form(kat, prep, form, N):
    assert kat.L.kat_max_players() == C.MAX_PLAYERS_REC
    an = prep["an"]
    g = C.player_groups(an, prep["lean"], N)
    cl = an["clamp"][g]
    assert g.shape[0] % 64 != 0 and cl.all(axis=1).any() and (~cl).all(axis=1).any()
    for i in range(N):  # the clamp on player i alone
        assert (cl[:, i] & (cl.sum(axis=1) == 1)).any()
    got = kat.players(0 if form == "players_lean" else 1, an["players"][g], an["inputs"][g])
    assert_steps_equal(got.reshape(-1, 5), an["ref"][g].reshape(-1, 5), an, g.ravel(),
                       f"{form}<{N}> (lane = index // {N}, player = index % {N})")


@pytest.mark.parametrize("P", [1, 2, 3, 4])
@pytest.mark.parametrize("form", ["state", "state_lean", "state_lean_k"])
def test_state_form(kat, prep, oracle, form, P):
    an = prep["an"]
    f = ("state", "state_lean", "state_lean_k").index(form)
    s = C.state_lanes(an, prep["every"] if f == 0 else prep["lean"], P, seed=100 + P, with_disconnects=f == 0)
    n = s["words"].shape[0]
    assert n % 64 != 0
    if f == 0:
        w = C.wave_census(an, s["who"][0])
        assert ((w["ood"] == 1) & w["ood_lane0"]).any() and ((w["ood"] == 1) & w["ood_lane63"]).any()
        assert (w["ood"] == 64).any() and (s["disc"] != 0).any()
    before = C.words_to_bincode(P, s["words"])
    after = oracle.state_advance_batch(before, s["inputs"], s["status"])
    want = C.bincode_to_words(P, after)
    assert np.array_equal(C.words_to_bincode(P, want), after)
    got, ck = kat.state(f, P, s["words"], s["packed"], s["disc"])
    assert np.array_equal(got[:, 0], want[:, 0]), "frame"
    for i in range(P):
        cols = [1 + 2 * i, 2 + 2 * i, 1 + 2 * P + 2 * i, 2 + 2 * P + 2 * i, 1 + 4 * P + i]
        assert_steps_equal(got[:, cols], want[:, cols], an, s["who"][i],
                           f"{form}<{P}> player {i} (a Disconnected player steps with input 4, whatever the case's input)")
    want_ck = oracle.fletcher16_batch(after)
    bad = np.flatnonzero(ck != want_ck)
    assert bad.size == 0, (f"fletcher16_state<{P}> of {bad.size} stepped states differs from fletcher16 of their bincode "
                           f"bytes; first lane {bad[0]}: device {int(ck[bad[0]]):04x}, oracle {int(want_ck[bad[0]]):04x}")


@pytest.mark.parametrize("form", ["rec_q + domain_raw", "lean_sc + domain"])
def test_chain(kat, prep, oracle, form):
    an = prep["an"]
    st, inp = C.chain_cases(an, seed=8)
    steps = inp.shape[1]
    assert steps == 8 and st.shape[0] % 64 != 0
    want = np.zeros((st.shape[0], steps, 5), np.uint32)
    cur = st
    for t in range(steps):
        cur = oracle.ship_step_batch(cur, inp[:, t])
        want[:, t] = cur
    assert (want[:, :, 4] <= C.TWO_PI_BITS).all()
    turned = (want[:, 1:, 4] != want[:, :-1, 4]).any(axis=1)
    thrust_late = ((inp[:, 1:] & 3) % 3 != 0).any(axis=1)
    assert (turned & thrust_late).any()  # a later step's sin/cos comes from a rotation the chain itself made
    got = kat.chain(0 if form.startswith("rec_q") else 1, st, inp)
    diff = (got != want).any(axis=2)
    if diff.any():
        lanes = np.flatnonzero(diff.any(axis=1))
        lane = int(lanes[0])
        t = int(diff[lane].argmax())
        prev = st[lane] if t == 0 else want[lane, t - 1]
        pytest.fail(f"{form}: {lanes.size} of {st.shape[0]} lanes leave the oracle's chain.  First: lane {lane}, step {t}, "
                    f"input 0x{int(inp[lane, t]):02x} (the lane's inputs {[hex(int(b)) for b in inp[lane]]}), from "
                    f"{_hex(prev)}: oracle {_hex(want[lane, t])}, device {_hex(got[lane, t])}, fields "
                    f"{[f for q, f in enumerate(FIELDS) if got[lane, t, q] != want[lane, t, q]]}.  Lanes by their first "
                    f"differing step: {np.bincount(diff[lanes].argmax(axis=1), minlength=steps).tolist()}")


@pytest.mark.parametrize("mad24", [0, 1])
@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_fletcher(kat, oracle, P, mad24):
    words = C.fletcher_words(P, seed=200 + P)
    rows = C.words_to_bincode(P, words)
    want = np.array([oracle.fletcher16(r.tobytes()) for r in rows], np.uint16)
    state, doubled, host = kat.fletcher(P, mad24, words)
    for name, got in ((f"fletcher16_state<{P}>", state), (f"fletcher_from_doubled<{bool(mad24)}>", doubled),
                      (f"fletcher16_state_host<{P}>", host)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{name}: {bad.size} of {want.size} differ from fletcher16 of the bincode bytes; first row "
                               f"{bad[0]}, words {_hex(words[bad[0]])}: got {int(got[bad[0]]):04x}, oracle {int(want[bad[0]]):04x}")


@pytest.mark.parametrize("form", ["domain", "domain_k", "domain_raw", "domain_raw_k"])
def test_domain_digest(kat, form):
    g = GOLDEN["sincos_digest_0_2pi"]
    f = ("domain", "domain_k", "domain_raw", "domain_raw_k").index(form)
    assert kat.domain_digest(f, g["lo"], g["hi"]) == g["digest"], f"glibc_sincosf_{form} differs from libm somewhere in [0, 2 pi]"


# glibc 2.35 sysdeps/ieee754/flt-32/sincosf_data.c, __sincosf_table[0] (hpi_inv there is 2/pi * 2^24: the
# domain forms multiply by hpi_inv * 2^-24) and the 1.5 * 2^52 of the domain forms' rounding
GLIBC_SINCOS = {"hpi_inv * 2^-24": "0x1.45F306DC9C883p-1", "magic": "0x1.8p52", "hpi": "0x1.921FB54442D18p0",
                "s1": "-0x1.555545995a603p-3", "s2": "0x1.1107605230bc4p-7", "s3": "-0x1.994eb3774cf24p-13",
                "c1": "-0x1.ffffffd0c621cp-2", "c2": "0x1.55553e1068f19p-5", "c3": "-0x1.6c087e89a359dp-10",
                "c4": "0x1.99343027bf8c3p-16"}


def test_sincos_constants(kat):
    """A polynomial coefficient one ulp off changes no f32 result over the whole of [0, 2 pi] (the
    digests stay equal: measured), so the constants are pinned by value as well."""
    lit, vgpr = kat.sincos_consts()
    for i, (name, want) in enumerate(GLIBC_SINCOS.items()):
        assert float(lit[i]).hex() == float.fromhex(want).hex(), f"kSincosLiteral {name}"
        assert float(vgpr[i]).hex() == float.fromhex(want).hex(), f"sincos_consts_vgpr() {name}"
