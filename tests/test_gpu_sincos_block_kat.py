"""GPU known-answer test of the sin/cos block (ggrs_amd/csrc/synctest_sincos_block.h): what the
producer wave of the check_distance-8, two-player SyncTest kernel runs once per 8-step core block --
the block's eight turns (block_rot_chain), one sin/cos evaluation per lane published as a 16-byte
entry (sincos_block_pass), and the entry a step reads (sincos_block_entry).

tests/native/sincos_block_kat_device.hip runs the header's functions themselves, one wave per eight
(session, player) pairs, and beside them eight chained single-step calls of advance_player_rec_q with
the hook the per-step form used.  Compared here, bit for bit:
  * every lane's r[u] and the hand-off's field-4 words with the chained calls' rot after step u;
  * the entry step u + 1 reads, on every lane, with the (sr, cr, qs, qc) the chained calls' hook
    evaluated after step u;
  * every r[u] with the CPU oracle's step (ship_step_batch), chained.

A wave's eight pairs start from different rotations and take different inputs, so an entry read from
another step's, another player's or another session's lane differs from the expected one.
"""
import ctypes

import numpy as np
import pytest

from tests import step_form_cases as C

pytestmark = pytest.mark.gpu

CD, P, SESS, WAVE, PAIRS = 8, 2, 4, 64, 8
F32 = np.float32
TWO_PI = C.u2f(np.array([C.TWO_PI_BITS], np.uint32))[0]
RS = C.ROTATION_SPEED
LEFT, RIGHT = C.LEFT, C.RIGHT


class Kat:
    def __init__(self, so):
        self.L = ctypes.CDLL(so)
        u32, u8 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
        self.L.kat_sincos_block.argtypes = [ctypes.c_int, u32, u8, u32, u32, u32, u32, u32]
        self.failed = None

    def run(self, rot0, inp):
        """rot0 [n] u32 and inp [n][8] u8 per (session, player) pair, n a multiple of 8 ->
        r, hand4, ref_r [n / 8][64][8], sc, ref_sc [n / 8][64][8][4]"""
        if self.failed:
            pytest.fail(f"not launched: {self.failed}")
        rot0, inp = np.ascontiguousarray(rot0, np.uint32), np.ascontiguousarray(inp, np.uint8)
        n = rot0.shape[0]
        assert n % PAIRS == 0 and inp.shape == (n, CD)
        w = n // PAIRS
        r, hand4, ref_r = (np.zeros((w, WAVE, CD), np.uint32) for _ in range(3))
        sc, ref_sc = (np.zeros((w, WAVE, CD, 4), np.uint32) for _ in range(2))
        p = lambda a, ct: a.ctypes.data_as(ctypes.POINTER(ct))
        rc = self.L.kat_sincos_block(w, p(rot0, ctypes.c_uint32), p(inp, ctypes.c_uint8), *(p(a, ctypes.c_uint32)
                                                                                          for a in (r, hand4, sc, ref_r, ref_sc)))
        if rc != 0:
            self.failed = f"kat_sincos_block returned {rc}"
            pytest.fail(self.failed)
        return r, hand4, sc, ref_r, ref_sc


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    return Kat(C.compile_kat("sincos_block_kat_device", tmp_path_factory.mktemp("sincos_block_kat")))


def pair_of_lane():
    """the (session, player) pair of each of a wave's 64 lanes"""
    lane = np.arange(WAVE)
    return (lane // 16) * P + (lane % P)


def pad(rot0, inp):
    """to a multiple of 8 pairs, repeating the first cases"""
    n = rot0.shape[0]
    m = -n % PAIRS
    idx = np.concatenate([np.arange(n), np.arange(m) % n])
    return rot0[idx], inp[idx]


def oracle_chain(oracle, rot0, inp):
    """the oracle's rot after each of the eight steps [n][8]"""
    n = rot0.shape[0]
    cur = np.zeros((n, 5), np.uint32)
    cur[:, 0], cur[:, 1] = C.bits_of(F32(300.0)), C.bits_of(F32(400.0))
    cur[:, 4] = rot0
    want = np.zeros((n, CD), np.uint32)
    for u in range(CD):
        cur = oracle.ship_step_batch(cur, np.ascontiguousarray(inp[:, u]))
        want[:, u] = cur[:, 4]
    return want


def check(kat, oracle, rot0, inp):
    rot0, inp = pad(np.asarray(rot0, np.uint32), np.asarray(inp, np.uint8))
    assert (rot0 <= C.TWO_PI_BITS).all()
    r, hand4, sc, ref_r, ref_sc = kat.run(rot0, inp)
    w = rot0.shape[0] // PAIRS
    pair = pair_of_lane()

    def where(bad):
        b, lane, u = (int(v) for v in np.argwhere(bad)[0][:3])
        k = b * PAIRS + int(pair[lane])
        return f"wave {b} lane {lane} step {u}: start {int(rot0[k]):#x}, inputs {inp[k].tolist()}"

    bad = r != ref_r
    assert not bad.any(), f"r[u] differs from the chained steps' rot; {where(bad)}: got {r[bad][0]:#x}, want {ref_r[bad][0]:#x}"
    bad = hand4 != ref_r
    assert not bad.any(), f"the hand-off's field 4 differs; {where(bad)}"
    bad = (sc != ref_sc).any(axis=3)
    assert not bad.any(), (f"the entry a step reads differs from the per-step evaluation; {where(bad)}: got "
                           f"{[hex(int(v)) for v in sc[bad][0]]}, want {[hex(int(v)) for v in ref_sc[bad][0]]}")
    want = oracle_chain(oracle, rot0, inp).reshape(w, PAIRS, CD)[:, pair, :]
    bad = r != want
    assert not bad.any(), f"r[u] differs from the oracle's step; {where(bad)}: got {r[bad][0]:#x}, want {want[bad][0]:#x}"
    return r, sc


def test_every_nibble_at_every_step(kat, oracle):
    """all 16 direction nibbles at each of the eight step positions, the other steps turning left or
    right, from rotations in the middle of the domain and next to both wraps"""
    rng = np.random.default_rng(0x51C0)
    starts = np.concatenate([C._bits(F32(3.0), [0]), C._bits(F32(0.01), [0]), C._bits(F32(TWO_PI - F32(0.01)), [0])])
    rot0, inp = [], []
    for u in range(CD):
        for nib in range(16):
            for fill in (LEFT, RIGHT, 0):
                for s in starts:
                    row = np.full(CD, fill, np.uint8)
                    row[u] = nib
                    rot0.append(s), inp.append(row)
    rot0, inp = np.array(rot0, np.uint32), np.array(inp, np.uint8)
    order = rng.permutation(rot0.shape[0])  # neighbouring pairs of a wave differ
    check(kat, oracle, rot0[order], inp[order])


def test_wraps_land_at_every_step(kat, oracle):
    """0, 2 pi, their f32 neighbours, and starts within one kRotationSpeed of 0 and of 2 pi on either
    side of every multiple of it up to eight, held left, held right and alternating: the a < 0 wrap and
    the a >= 2 pi wrap each occur at every step position, and a turn lands on exactly 2 pi (where >=
    and > differ)"""
    around = np.arange(-3, 4)
    starts = [np.array([0, 1, 2, 3], np.uint32), C._bits(C.TWO_PI_BITS, np.arange(-3, 1))]
    for k in range(0, CD + 1):
        for frac in (0.0, 0.25, 0.75):
            d = F32(F32(k + frac) * RS)
            starts.append(C._bits(d, around) if d > 0 else np.array([0], np.uint32))
            starts.append(C._bits(F32(TWO_PI - d), around))
    starts = np.unique(np.concatenate(starts))
    starts = starts[starts <= C.TWO_PI_BITS]
    # a start whose first right turn is exactly 2 pi must be among them
    exact = starts[(C.u2f(starts) + RS) == TWO_PI]
    assert exact.size > 0, "no start lands on exactly 2 pi"
    rows = np.array([[LEFT] * CD, [RIGHT] * CD, [LEFT, RIGHT] * 4, [RIGHT, LEFT] * 4, [RIGHT, RIGHT, 0, LEFT] * 2], np.uint8)
    si, ri = (a.ravel() for a in np.meshgrid(np.arange(starts.size), np.arange(rows.shape[0])))
    rng = np.random.default_rng(0x2B1)
    order = rng.permutation(si.size)
    rot0, inp = starts[si][order], rows[ri][order]
    check(kat, oracle, rot0, inp)
    # both wraps did occur at every step position (worked out from the oracle's chain and the inputs)
    chain = oracle_chain(oracle, rot0, inp)
    before = np.concatenate([rot0[:, None], chain[:, :-1]], axis=1)
    a = C.u2f(before) + np.where(inp & LEFT, -RS, np.where(inp & RIGHT, RS, F32(0.0))).astype(F32)
    assert a.dtype == F32
    for u in range(CD):
        assert (a[:, u] < 0).any(), f"no wrap below 0 at step {u}"
        assert (a[:, u] >= TWO_PI).any(), f"no wrap at 2 pi at step {u}"
    assert (a == TWO_PI).any()


def test_random_rotations_and_inputs(kat, oracle):
    """4096 seeded random in-domain rotations with random nibbles: every pair of every wave differs"""
    rng = np.random.default_rng(0xB10C)
    n = 4096
    rot0 = C._rand_rot(rng, n)
    inp = rng.integers(0, 16, (n, CD)).astype(np.uint8)
    r, sc = check(kat, oracle, rot0, inp)
    # the cases can tell lanes apart: within a wave, the two players of a session and the four
    # sessions read different entries at every step in nearly every wave
    e = sc.reshape(-1, SESS, CD, P, CD, 4)[:, :, 0]  # role 0's reads [wave][session][player][step][4]
    assert ((e[:, :, 0] != e[:, :, 1]).any(axis=3).mean()) > 0.9
    assert ((e[:, 0] != e[:, 1]).any(axis=3).mean()) > 0.9
    # and consecutive steps' entries differ where the pair turned
    assert ((sc[:, :, 1:] != sc[:, :, :-1]).any(axis=3).mean()) > 0.4
