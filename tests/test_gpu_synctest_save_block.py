"""GPU known-answer test of synctest_save_block (ggrs_amd/csrc/synctest_save.h): what the consumer
wave of the check_distance-8, two-player SyncTest kernel does with one 8-step core block -- the role
equality test by state bits, one Fletcher-16 and one save per step.

tests/native/save_block_kat_device.hip runs the header's function itself, one one-wave block per
case, on hand-off buffers crafted here and a small ring per block; this file restates the bincode
bytes, Fletcher-16 and the ring layout in numpy and compares every byte of every ring.

Wave layout: lane = session * 16 + role * 2 + player (four session slots, eight roles, two
players).  Hand-off buffer: per step 64 x 4 words (fields x, y, vx, vy per lane), then 64 words
(rot per lane).  Ring of a block, as the engine's buffers at L = 4 lanes: ring [R][11][4] u32,
ring_ck [R][4] u16, first_ck [R][4] u16.
"""
import ctypes

import numpy as np
import pytest

from tests import step_form_cases as C

pytestmark = pytest.mark.gpu

CD, P, SESS, WAVE, F = 8, 2, 4, 64, 11
STEP_WORDS = WAVE * 5
STRIDE = 16 * 192                      # arena bytes per block: room for R <= 16
FIELD_WORD = lambda q, pl: (1 + 2 * pl, 2 + 2 * pl, 5 + 2 * pl, 6 + 2 * pl, 9 + pl)[q]  # box_game.h fld_x .. fld_rot at P = 2


def fletcher16(rows):
    """Fletcher-16 of each row of bytes, reduced mod 255 after every byte (the reference's fletcher16)"""
    rows = np.ascontiguousarray(rows, np.uint8)
    s1, s2 = np.zeros(rows.shape[0], np.uint32), np.zeros(rows.shape[0], np.uint32)
    for k in range(rows.shape[1]):
        s1 = (s1 + rows[:, k]) % 255
        s2 = (s2 + s1) % 255
    return ((s2 << 8) | s1).astype(np.uint16)


def test_fletcher16_restatement():
    # the published Fletcher-16 test vectors
    for text, want in ((b"abcde", 0xC8F0), (b"abcdef", 0x2057), (b"abcdefgh", 0x0627)):
        assert int(fletcher16(np.frombuffer(text, np.uint8)[None, :])[0]) == want


class Kat:
    def __init__(self, so):
        self.L = ctypes.CDLL(so)
        Pt = ctypes.POINTER
        self.L.kat_save_block.argtypes = [ctypes.c_int, Pt(ctypes.c_int32), Pt(ctypes.c_uint32), Pt(ctypes.c_uint8),
                                          ctypes.c_int64, Pt(ctypes.c_uint64)]
        self.failed = None

    def run(self, ctl, hand, arena):
        """ctl [n][4] (R, sr, t, nsess), hand [n][8][320] u32, arena [n][STRIDE] u8 -> (arena after, lane masks)"""
        if self.failed:
            pytest.fail(f"not launched: {self.failed}")
        ctl, hand = np.ascontiguousarray(ctl, np.int32), np.ascontiguousarray(hand, np.uint32)
        out = np.ascontiguousarray(arena, np.uint8).copy()
        n = ctl.shape[0]
        assert hand.shape == (n, CD, STEP_WORDS) and out.shape == (n, STRIDE)
        flagged = np.zeros(n, np.uint64)
        p = lambda a, ct: a.ctypes.data_as(ctypes.POINTER(ct))
        rc = self.L.kat_save_block(n, p(ctl, ctypes.c_int32), p(hand, ctypes.c_uint32), p(out, ctypes.c_uint8), STRIDE,
                                   p(flagged, ctypes.c_uint64))
        if rc != 0:
            self.failed = f"kat_save_block returned {rc}"
            pytest.fail(self.failed)
        return out, flagged


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    return Kat(C.compile_kat("save_block_kat_device", tmp_path_factory.mktemp("save_block_kat")))


def lane_of(g, role, pl):
    return g * 16 + role * 2 + pl


def equal_hand(rng, n):
    """states [n][8 steps][4 sessions][2 players][5 fields], random bits, and the hand-off buffers in
    which every role of a session holds them"""
    st = rng.integers(0, 1 << 32, (n, CD, SESS, P, 5), dtype=np.uint64).astype(np.uint32)
    per_lane = np.broadcast_to(st[:, :, :, None, :, :], (n, CD, SESS, CD, P, 5)).reshape(n, CD, WAVE, 5)
    hand = np.concatenate([per_lane[..., :4].reshape(n, CD, WAVE * 4), per_lane[..., 4]], axis=2)
    return st, np.ascontiguousarray(hand)


def hand_word(u, lane, q):
    """index of field q of a lane in step u's 320 hand-off words"""
    return (lane * 4 + q) if q < 4 else (WAVE * 4 + lane)


def expected_arena(before, ctl, st):
    """the arenas after each block saved its eight steps from the states st"""
    out = before.copy()
    n = ctl.shape[0]
    for b in range(n):
        R, sr, t, nsess = (int(x) for x in ctl[b])
        ring = out[b, :R * F * SESS * 4].view(np.uint32).reshape(R, F, SESS)
        ring_ck = out[b, R * F * SESS * 4:R * F * SESS * 4 + R * SESS * 2].view(np.uint16).reshape(R, SESS)
        first_ck = out[b, R * 184:R * 192].view(np.uint16).reshape(R, SESS)
        for u in range(CD):
            slot = (sr + u) % R
            words = np.zeros((nsess, F), np.uint32)
            words[:, 0] = np.uint32((t + u - CD + 1) & 0xFFFFFFFF)
            for pl in range(P):
                for q in range(5):
                    words[:, FIELD_WORD(q, pl)] = st[b, u, :nsess, pl, q]
            ck = fletcher16(C.words_to_bincode(P, words))
            ring[slot, :, :nsess] = words.T
            ring_ck[slot, :nsess] = ck
            first_ck[slot, :nsess] = ck
    return out


def fresh_arena(rng, n):
    return rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)


def test_equal_roles_every_start_slot(kat):
    """every role holds the same state: nothing is flagged; at every start slot of R = 10 and 13 the
    eight cells, frame words, ring_ck and first_ck entries are the restated ones and every other byte
    of the arena keeps its pattern"""
    rng = np.random.default_rng(0x5A7E)
    ctl = [(R, sr, 0, SESS) for R in (10, 13) for sr in range(R)]
    ctl = np.array(ctl, np.int32)
    n = ctl.shape[0]
    ctl[:, 2] = rng.integers(CD, 0x7FFFFFF0, n)
    ctl[0, 2], ctl[1, 2] = CD - 1, 0x7FFFFFF0  # frames 0 .. 7; the largest
    st, hand = equal_hand(rng, n)
    before = fresh_arena(rng, n)
    after, flagged = kat.run(ctl, hand, before)
    assert (flagged == 0).all(), f"flagged lane masks {[hex(int(x)) for x in flagged]}"
    want = expected_arena(before, ctl, st)
    bad = np.argwhere(after != want)
    assert bad.size == 0, (f"{bad.shape[0]} arena bytes differ; first block {bad[0][0]} (R, sr, t, nsess = {ctl[bad[0][0]]}) "
                           f"byte {bad[0][1]}: got {after[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
    # the restated arenas did change where they should: 8 x (11 words + 2 checksums) x 4 sessions
    assert ((want != before).sum(axis=1) > 8 * SESS * 40).all()


def test_one_bit_flipped_is_flagged(kat):
    """one bit of one field of one (step, role, player) lane differs: the lane and its next role see
    it, whatever the step, role (0 and 7 wrap around the row), player, field and bit (0 and 31)"""
    rng = np.random.default_rng(0xB17)
    grid = [(u, role, pl, q, bit) for u in range(CD) for role in range(CD) for pl in range(P) for q in range(5)
            for bit in (0, 31)]
    n = len(grid)
    ctl = np.array([(10, k % 10, 100 + k, SESS) for k in range(n)], np.int32)
    _, hand = equal_hand(rng, n)
    want = np.zeros(n, np.uint64)
    for k, (u, role, pl, q, bit) in enumerate(grid):
        g = k % SESS
        hand[k, u, hand_word(u, lane_of(g, role, pl), q)] ^= np.uint32(1 << bit)
        want[k] = (1 << lane_of(g, role, pl)) | (1 << lane_of(g, (role + 1) % CD, pl))
    _, flagged = kat.run(ctl, hand, fresh_arena(rng, n))
    assert (flagged != 0).all(), f"not flagged: {[grid[k] for k in np.flatnonzero(flagged == 0)[:8]]}"
    bad = np.flatnonzero(flagged != want)
    assert bad.size == 0, (f"{bad.size} lane masks differ; first {grid[bad[0]]}: got {int(flagged[bad[0]]):#x}, "
                           f"want {int(want[bad[0]]):#x}")


def test_fletcher_collision_is_flagged(kat):
    """one role's state differs from the others in two fields whose differences cancel in both
    Fletcher-16 sums (+5 at bincode byte 20, -5 at byte 71: sum1 +5 - 5, sum2 5 * (56 - 5) = 255):
    the checksums are equal, the bits are not, and the block is flagged"""
    rng = np.random.default_rng(0xC011)
    st, hand = equal_hand(rng, 1)
    u, g, role, pl = 5, 2, 3, 0
    x, rot = int(st[0, u, g, pl, 0]), int(st[0, u, g, pl, 4])
    x = (x & ~0xFF) | 0x40            # bincode byte 20: x's low byte
    rot = (rot & 0x00FFFFFF) | (0x80 << 24)  # byte 71: rot's high byte
    for lane_role in range(CD):
        lane = lane_of(g, lane_role, pl)
        hand[0, u, hand_word(u, lane, 0)] = x
        hand[0, u, hand_word(u, lane, 4)] = rot
    x2, rot2 = x + 5, rot - (5 << 24)
    words = np.zeros((2, F), np.uint32)
    words[:, 0] = 77
    for p_ in range(P):
        for q in range(5):
            words[:, FIELD_WORD(q, p_)] = st[0, u, g, p_, q]
    words[:, FIELD_WORD(0, pl)], words[:, FIELD_WORD(4, pl)] = (x, x2), (rot, rot2)
    rows = C.words_to_bincode(P, words)
    assert (rows[0] != rows[1]).sum() == 2 and rows[0, 20] + 5 == rows[1, 20] and rows[0, 71] - 5 == rows[1, 71]
    ck = fletcher16(rows)
    assert ck[0] == ck[1], "the crafted states do not collide"
    lane = lane_of(g, role, pl)
    hand[0, u, hand_word(u, lane, 0)] = x2
    hand[0, u, hand_word(u, lane, 4)] = rot2
    _, flagged = kat.run(np.array([(10, 3, 77 + CD - 1 - u, SESS)], np.int32), hand, fresh_arena(rng, 1))
    assert int(flagged[0]) == (1 << lane) | (1 << lane_of(g, role + 1, pl))


@pytest.mark.parametrize("nsess", [1, 2, 3])
def test_partial_blocks(kat, nsess):
    """blocks of one, two and three sessions: the lanes of the missing sessions hold different garbage
    in every role; they flag nothing and store nothing, the sessions present are saved as in a full block"""
    rng = np.random.default_rng(0x9A7 + nsess)
    ctl = np.array([(R, sr, 1000 + 8 * sr, nsess) for R in (10, 13) for sr in (0, 4, R - 1)], np.int32)
    n = ctl.shape[0]
    st, hand = equal_hand(rng, n)
    garbage = rng.integers(0, 1 << 32, (n, CD, STEP_WORDS), dtype=np.uint64).astype(np.uint32)
    missing = np.zeros(STEP_WORDS, bool)
    for lane in range(nsess * 16, WAVE):
        for q in range(5):
            missing[hand_word(0, lane, q)] = True
    hand[:, :, missing] = garbage[:, :, missing]
    before = fresh_arena(rng, n)
    after, flagged = kat.run(ctl, hand, before)
    assert (flagged == 0).all(), f"flagged lane masks {[hex(int(x)) for x in flagged]}"
    want = expected_arena(before, ctl, st)
    bad = np.argwhere(after != want)
    assert bad.size == 0, (f"{bad.shape[0]} arena bytes differ; first block {bad[0][0]} (R, sr, t, nsess = {ctl[bad[0][0]]}) "
                           f"byte {bad[0][1]}: got {after[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
