"""GPU parity of the check_distance-8, two-player SyncTest kernel whose consumer wave saves once per
core step (ggrs_amd/csrc/synctest_save.h): lane (session, role j, player) stores step j of each
8-step block into ring slot (first slot + j) mod R, and writes the first-seen checksum of that slot.

Bit-exact against the oracle's SyncTestSession, every lane: the per-frame display checksums, the
final state, and the saved-state ring's frames, checksums and state bytes (check_lane of
test_gpu_synctest).  R = max_prediction + 1 = 10, 12, 16 and input delay 0, 2, on one full block
(4 lanes, the fast prologue) and a full block plus a one-session block (5 lanes).

A session's first cd + 1 calls have no rollback yet and always run on the sequential kernel, so
every case first advances cd + 1 frames in a call of its own (see test_gpu_synctest_split.py);
each listed launch is then exactly one launch of the batched kernel.
"""
import pytest

from tests.test_gpu_synctest import check_lane, lane_inputs, make_engine, run_chunks

pytestmark = pytest.mark.gpu

CD, PLAYERS = 8, 2

LAUNCHES = [
    [16],          # one core block between the edge blocks
    [24],          # two core blocks: both hand-off buffers
    [48, 40],      # 40 = lcm(8, R = 10): every ring slot at every block position
    [16, 16, 16],  # a wrong first_ck from one launch would halt lanes in the next launch's edge steps
]


@pytest.mark.parametrize("delay", [0, 2])
@pytest.mark.parametrize("maxp", [9, 11, 15])
@pytest.mark.parametrize("launches", LAUNCHES, ids=["_".join(map(str, n)) for n in LAUNCHES])
@pytest.mark.parametrize("lanes", [4, 5])
def test_one_save_per_core_step_every_lane(oracle, lanes, launches, maxp, delay):
    frames = CD + 1 + sum(launches)
    inputs = lane_inputs(oracle, 5100 + 16 * lanes + maxp + delay, lanes, frames, PLAYERS, 0)
    eng = make_engine(lanes, PLAYERS, maxp, CD, delay, frames)
    assert run_chunks(eng, inputs, [CD + 1] + launches) == frames
    assert eng.current_frame() == frames
    trace = eng.trace(0, frames)
    for lane in range(lanes):
        check_lane(oracle, eng, inputs, lane, PLAYERS, maxp, CD, delay, frames, trace)
    status, _, _ = eng.mismatches()
    assert (status == 0).all()
