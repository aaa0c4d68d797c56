"""GPU known-answer test of the increment block (ggrs_amd/csrc/synctest_sincos_block.h, box_game.h):
what the two waves of the check_distance-8, two-player SyncTest kernel run per 8-step core block --
the block's eight turns (block_rot_chain), one sin/cos evaluation per lane finished into the 8-byte
velocity increment of the step that reads it (increment_block_pass: the lane of role j folds it with
its own record of row j + 1), the entry a step reads (increment_block_entry), the producer's step on
an increment (advance_player_inc_turned) and the consumer's batch sub-step (advance_player_inc).

tests/native/increment_block_kat_device.hip runs the headers' functions themselves, one wave per
eight (session, player) pairs, and beside them nine chained single-step calls of advance_player_rec_q
with the hook the per-step form used.  Compared here, bit for bit, on every lane and every step:
  * x, y, vx, vy after each of the eight steps, and the hand-off's field-4 word, with the chained
    calls' state;
  * the increment each step ran on -- step 0's folded in front of the loop, steps 1..7 and the next
    block's step 0 read from the entries -- with the increment the chained form computed there;
  * the batch sub-step of the lane of role j with the chained calls' state after step j + 1;
  * the chained calls' whole state with the CPU oracle's step (ship_step_batch), chained.

A wave's eight pairs start from different states and take different inputs, so an entry folded with
another row's record or read from another step's, player's or session's lane differs from the
expected one.
"""
import ctypes

import numpy as np
import pytest

from tests import step_form_cases as C

pytestmark = pytest.mark.gpu

CD, ROWS, P, SESS, WAVE, PAIRS = 8, 9, 2, 4, 64, 8
F32 = np.float32
TWO_PI = C.u2f(np.array([C.TWO_PI_BITS], np.uint32))[0]
UP, DOWN, LEFT, RIGHT = C.UP, C.DOWN, C.LEFT, C.RIGHT


class Kat:
    def __init__(self, so):
        self.L = ctypes.CDLL(so)
        u32, u8 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)
        self.L.kat_increment_block.argtypes = [ctypes.c_int, u32, u8, u32, u32, u32, u32, u32, u32]
        self.failed = None

    def run(self, start, inp):
        """start [n][5] u32 and inp [n][9] u8 per (session, player) pair, n a multiple of 8 ->
        st [w][64][8][4], r [w][64][8], inc [w][64][9][2], batch [w][64][5], ref_st [w][64][9][5],
        ref_inc [w][64][9][2]"""
        if self.failed:
            pytest.fail(f"not launched: {self.failed}")
        start, inp = np.ascontiguousarray(start, np.uint32), np.ascontiguousarray(inp, np.uint8)
        n = start.shape[0]
        assert n % PAIRS == 0 and start.shape == (n, 5) and inp.shape == (n, ROWS)
        w = n // PAIRS
        st = np.zeros((w, WAVE, CD, 4), np.uint32)
        r = np.zeros((w, WAVE, CD), np.uint32)
        inc, ref_inc = (np.zeros((w, WAVE, ROWS, 2), np.uint32) for _ in range(2))
        batch = np.zeros((w, WAVE, 5), np.uint32)
        ref_st = np.zeros((w, WAVE, ROWS, 5), np.uint32)
        p = lambda a, ct: a.ctypes.data_as(ctypes.POINTER(ct))
        rc = self.L.kat_increment_block(w, p(start, ctypes.c_uint32), p(inp, ctypes.c_uint8),
                                        *(p(a, ctypes.c_uint32) for a in (st, r, inc, batch, ref_st, ref_inc)))
        if rc != 0:
            self.failed = f"kat_increment_block returned {rc}"
            pytest.fail(self.failed)
        return st, r, inc, batch, ref_st, ref_inc


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    return Kat(C.compile_kat("increment_block_kat_device", tmp_path_factory.mktemp("increment_block_kat")))


def pair_of_lane():
    """the (session, player) pair of each of a wave's 64 lanes"""
    lane = np.arange(WAVE)
    return (lane // 16) * P + (lane % P)


def pad(start, inp):
    """to a multiple of 8 pairs, repeating the first cases"""
    n = start.shape[0]
    m = -n % PAIRS
    idx = np.concatenate([np.arange(n), np.arange(m) % n])
    return start[idx], inp[idx]


def oracle_chain(oracle, start, inp):
    """the oracle's state after each of the nine steps [n][9][5]"""
    cur = np.ascontiguousarray(start, np.uint32)
    want = np.zeros((start.shape[0], ROWS, 5), np.uint32)
    for u in range(ROWS):
        cur = oracle.ship_step_batch(cur, np.ascontiguousarray(inp[:, u]))
        want[:, u] = cur
    return want


def check(kat, oracle, start, inp):
    start, inp = pad(np.asarray(start, np.uint32), np.asarray(inp, np.uint8))
    assert (start[:, 4] <= C.TWO_PI_BITS).all()
    st, r, inc, batch, ref_st, ref_inc = kat.run(start, inp)
    w = start.shape[0] // PAIRS
    pair = pair_of_lane()
    role = (np.arange(WAVE) % 16) // P

    def where(bad):
        b, lane = (int(v) for v in np.argwhere(bad)[0][:2])
        rest = [int(v) for v in np.argwhere(bad)[0][2:]]
        k = b * PAIRS + int(pair[lane])
        return f"wave {b} lane {lane} at {rest}: start {[hex(int(v)) for v in start[k]]}, inputs {inp[k].tolist()}"

    bad = inc != ref_inc
    assert not bad.any(), (f"the increment a step ran on differs from the chained form's; {where(bad)}: got "
                           f"{inc[bad][0]:#x}, want {ref_inc[bad][0]:#x}")
    bad = st != ref_st[:, :, :CD, :4]
    assert not bad.any(), f"x, y, vx, vy differ from the chained steps'; {where(bad)}: got {st[bad][0]:#x}, want {ref_st[:, :, :CD, :4][bad][0]:#x}"
    bad = r != ref_st[:, :, :CD, 4]
    assert not bad.any(), f"the hand-off's field 4 differs from the chained steps' rot; {where(bad)}"
    want_batch = ref_st[:, np.arange(WAVE), role + 1, :]  # the state after step j + 1 on the lane of role j
    bad = batch != want_batch
    assert not bad.any(), f"the batch sub-step differs from the chained step j + 1; {where(bad)}"
    want = oracle_chain(oracle, start, inp).reshape(w, PAIRS, ROWS, 5)[:, pair]
    bad = ref_st != want
    assert not bad.any(), f"the chained steps differ from the oracle's; {where(bad)}: got {ref_st[bad][0]:#x}, want {want[bad][0]:#x}"
    return inc, want


def states(x, y, vx, vy, rot_bits):
    return C._states(x, y, vx, vy, rot_bits)


def test_every_nibble_at_every_row(kat, oracle):
    """all 16 direction nibbles at each of the nine rows, the other rows cycling thrust, brake and
    neither (with turns) in three phases, so that neighbouring rows always differ in (sgn, keep): an
    entry folded with the row before or behind its own differs"""
    rng = np.random.default_rng(0x1BC0)
    cycle = np.array([UP | LEFT, DOWN | RIGHT, LEFT, UP | RIGHT, DOWN, RIGHT], np.uint8)
    rots = np.concatenate([C._bits(F32(0.7), [0]), C._bits(F32(2.4), [0]), C._bits(F32(4.0), [0]), C._bits(F32(5.5), [0])])
    start, inp = [], []
    for u in range(ROWS):
        for nib in range(16):
            for phase in range(3):
                for rb in rots:
                    row = cycle[(np.arange(ROWS) + phase) % cycle.size].copy()
                    row[u] = nib
                    start.append(states(300.0, 400.0, 1.5, -2.0, rb)[0]), inp.append(row)
    start, inp = np.array(start, np.uint32), np.array(inp, np.uint8)
    # neighbouring rows of the fill differ in thrust / brake / neither
    kind = np.where(cycle & UP, 1, np.where(cycle & DOWN, 2, 0))
    assert (kind != np.roll(kind, 1)).all()
    order = rng.permutation(start.shape[0])  # neighbouring pairs of a wave differ
    check(kat, oracle, start[order], inp[order])


def test_quadrants_and_wraps(kat, oracle):
    """start rotations in all four quadrants and next to both wraps, held and alternating turns under
    thrust, brake and neither: the quadrant signs qs and qc each take both values under each, the two
    differ from each other (quadrants 2 and 4), and the sine and cosine differ, so swapped signs or
    values show"""
    quad = [F32(0.3), F32(1.2), F32(1.9), F32(2.9), F32(3.4), F32(4.5), F32(5.0), F32(6.1)]
    rots = [C._bits(q, [0]) for q in quad]
    rots += [np.array([0, 1, 2], np.uint32), C._bits(C.TWO_PI_BITS, np.arange(-2, 1))]
    for k in (1, 3, 6):  # the wraps land inside the block
        d = F32(F32(k + 0.5) * C.ROTATION_SPEED)
        rots += [C._bits(d, [0]), C._bits(F32(TWO_PI - d), [0])]
    rots = np.unique(np.concatenate(rots))
    rows = []
    for ud in (UP, DOWN, 0):
        rows += [[ud | LEFT] * ROWS, [ud | RIGHT] * ROWS, [ud | LEFT, ud | RIGHT] * 4 + [ud | LEFT], [ud] * ROWS]
    rows += [[UP | LEFT, DOWN | LEFT, LEFT] * 3, [DOWN | RIGHT, RIGHT, UP | RIGHT] * 3]
    rows = np.array(rows, np.uint8)
    si, ri = (a.ravel() for a in np.meshgrid(np.arange(rots.size), np.arange(rows.shape[0])))
    rng = np.random.default_rng(0x9AD)
    order = rng.permutation(si.size)
    start, inp = states(250.0, 350.0, -0.75, 0.5, rots[si][order]), rows[ri][order]
    check(kat, oracle, start, inp)
    # the rot each row's step starts from (the oracle's), its quadrant and the row's thrust / brake /
    # neither: every combination occurs
    chain = oracle_chain(oracle, start, inp)
    before = C.u2f(np.concatenate([start[:, None, 4], chain[:, :-1, 4]], axis=1)).astype(np.float64)
    q = np.minimum((before / (np.pi / 2)).astype(np.int64), 3)
    kind = np.where(inp & UP, 1, np.where(inp & DOWN, 2, 0))
    for quadrant in range(4):
        for k in range(3):
            assert ((q == quadrant) & (kind == k)).any(), f"no step in quadrant {quadrant} with thrust kind {k}"


def test_clamp_at_every_step(kat, oracle):
    """starts at speed 6.9 .. 7.1 along the heading under thrust (held, and with gaps that let the
    speed fall below the cap and rise through it again), with and without a turn: the speed clamp
    fires at every step position, and first fires at different ones"""
    rng = np.random.default_rng(0xC1A)
    speeds = np.linspace(6.9, 7.1, 41)
    rows = [[UP] * ROWS, [UP | LEFT] * ROWS, [UP | RIGHT] * ROWS, [UP, 0, UP | LEFT] * 3, [0, UP, UP] * 3, [0, 0, UP | RIGHT] * 3,
            [DOWN, UP, UP, UP, UP] + [UP] * 4, [UP, UP, DOWN, UP, 0, UP, UP, UP | LEFT, UP]]
    rows = np.array(rows, np.uint8)
    start, inp = [], []
    for row in rows:
        for sp in speeds:
            ang = rng.random() * 2.0 * np.pi
            rb = min(C.bits_of(F32(ang)), C.TWO_PI_BITS)
            a = float(C.u2f(np.array([rb], np.uint32))[0])
            start.append(states(300.0, 400.0, sp * np.cos(a), sp * np.sin(a), np.array([rb], np.uint32))[0])
            inp.append(row)
    start, inp = np.array(start, np.uint32), np.array(inp, np.uint8)
    order = rng.permutation(start.shape[0])
    start, inp = start[order], inp[order]
    check(kat, oracle, start, inp)
    # where the clamp fired, from the oracle's chain alone: the speed before clamping, 0.98 v + the
    # increment of the heading, in binary64 (margins far above f32 rounding)
    chain = oracle_chain(oracle, start, inp)
    prev = np.concatenate([start[:, None, :], chain[:, :-1, :]], axis=1)
    v = np.stack([C.u2f(prev[:, :, 2]), C.u2f(prev[:, :, 3])], axis=2).astype(np.float64)
    a = C.u2f(prev[:, :, 4]).astype(np.float64)
    sign = np.where(inp & UP, 1.0, np.where(inp & DOWN, -1.0, 0.0))
    pre = 0.98 * v + 0.25 * sign[:, :, None] * np.stack([np.cos(a), np.sin(a)], axis=2)
    mag = np.hypot(pre[:, :, 0], pre[:, :, 1])
    fired, quiet = mag > 7.001, mag < 6.999
    for u in range(ROWS):
        assert fired[:, u].any(), f"no clamp at step {u}"
        assert quiet[:, u].any(), f"no step {u} without a clamp"
    first = np.where(fired.any(axis=1), fired.argmax(axis=1), -1)
    assert len(set(first.tolist()) - {-1}) >= 4, "the clamp first fires at too few step positions"


def test_random_pairs(kat, oracle):
    """4096 seeded random pairs (uniform states, random nibbles): every pair of every wave differs"""
    rng = np.random.default_rng(0x1AC4)
    n = 4096
    start = C._uniform(rng, n)
    inp = rng.integers(0, 16, (n, ROWS)).astype(np.uint8)
    inc, _ = check(kat, oracle, start, inp)
    # the cases can tell lanes apart: within a wave, the two players of a session and the four
    # sessions run on different increments at three steps in four (half of the nibbles neither
    # thrust nor brake, so two lanes both hold (-0.0, -0.0) at one step in four)
    e = inc.reshape(-1, SESS, CD, P, ROWS, 2)[:, :, 0]  # role 0's [wave][session][player][row][2]
    assert ((e[:, :, 0] != e[:, :, 1]).any(axis=3).mean()) > 0.6
    assert ((e[:, 0] != e[:, 1]).any(axis=3).mean()) > 0.6
    # and consecutive steps' increments differ
    assert ((inc[:, :, 1:] != inc[:, :, :-1]).any(axis=3).mean()) > 0.6
