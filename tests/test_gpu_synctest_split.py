"""GPU parity of the check_distance-8 SyncTest kernel's two-wave (producer / consumer) core blocks.

Bit-exact against the oracle's SyncTestSession, every lane: the per-frame display checksums, the
final state, and the saved-state ring's frames, checksums and state bytes (check_lane of
test_gpu_synctest).  cd 8, max_prediction 9, input delay 2, the default path.

The launch lists below are the pipelined launches.  A session's first cd + 1 calls have no
rollback yet and always run on the sequential kernel, so every case first advances cd + 1 frames
in a call of its own; each listed launch is then exactly one launch of the batched kernel.
"""
import numpy as np
import pytest

from tests.test_gpu_synctest import check_lane, lane_inputs, make_engine, run_chunks

pytestmark = pytest.mark.gpu

MAXP, CD, DELAY = 9, 8, 2

CASES = [
    # the smallest launch with a core block: edge block, one core block, edge block; two full blocks
    (8, 2, [16]),
    # a ragged last block; back-to-back launches, whose last edge stores and the next launch's core
    # stores meet in the same ring cells
    (7, 2, [24, 16, 16]),
    # launches off the 8-step grid: general steps around aligned core blocks
    (9, 2, [21, 19, 40]),
    # core blocks on both sides of the input restage (every 128 steps in the one-wave kernel, every
    # 64 in the split one): the batch's look-ahead row against the restage
    (5, 2, [136]),
    (5, 2, [264]),
    # longer than the 528 raw rows held at once: they are re-read inside the loop
    (4, 2, [544]),
    # the other player counts
    (13, 1, [40]),
    (10, 3, [40]),
    (6, 4, [40]),
]


@pytest.mark.parametrize("lanes,players,launches", CASES,
                         ids=[f"{l}x{p}-{'_'.join(map(str, n))}" for l, p, n in CASES])
def test_split_core_blocks_every_lane(oracle, lanes, players, launches):
    frames = CD + 1 + sum(launches)
    inputs = lane_inputs(oracle, 2300 + lanes, lanes, frames, players, 0)
    eng = make_engine(lanes, players, MAXP, CD, DELAY, frames)
    assert run_chunks(eng, inputs, [CD + 1] + launches) == frames
    assert eng.current_frame() == frames
    trace = eng.trace(0, frames)
    for lane in range(lanes):
        check_lane(oracle, eng, inputs, lane, players, MAXP, CD, DELAY, frames, trace)
    status, _, _ = eng.mismatches()
    assert (status == 0).all()


def test_launches_after_a_failed_launch(oracle):
    """A mismatch in the second 16-frame launch: every later launch starts with the failure already
    recorded, so its producer wave leaves before any core block and its consumer wave must leave
    with it.  Error frame, mask and halted state as the reference session."""
    from ggrs_amd import MismatchedChecksum, SessionBuilder
    players, frames, lanes, bad_lane, chunk, call = 2, 120, 70, 66, 16, 20
    inputs = lane_inputs(oracle, 9, lanes, frames, players, 0)
    sess = (SessionBuilder().with_num_players(players).with_max_prediction_window(MAXP)
            .with_check_distance(CD).with_input_delay(DELAY).with_num_lanes(lanes)
            .with_input_capacity(frames + 16).start_synctest_session())
    sess.engine.corrupt_on_load(bad_lane, call)
    sess.add_local_inputs(inputs)
    with pytest.raises(MismatchedChecksum) as ei:
        done = 0
        while done < frames:
            n = min(chunk, frames - done)
            sess.advance_frames(n, check=False)
            done += n
        sess.raise_on_mismatch()
    r = oracle.synctest_run(inputs[:, bad_lane, :], players, MAXP, CD, DELAY, corrupt_frame=call)
    assert r["result"].status == 1
    assert ei.value.current_frame == r["result"].mismatch_frame == call + 1
    mask = int(r["result"].mismatch_mask)
    assert ei.value.mismatched_frames == [call + 1 - CD + k for k in range(64) if mask >> k & 1]
    assert list(ei.value.lanes) == [bad_lane]
    st, mf, mm = sess.engine.mismatches()
    assert st[bad_lane] == 1 and mf[bad_lane] == call + 1 and int(mm[bad_lane]) == mask
    assert bytes(sess.engine.state(bad_lane)) == bytes(r["final_state"])
    fr, ck, sts = sess.engine.ring(bad_lane)
    for s in range(len(fr)):
        assert int(ck[s]) == int(r["ring_cksums"][s]) and bytes(sts[s]) == bytes(r["ring_states"][s])
    assert (st[np.arange(lanes) != bad_lane] == 0).all()
    for lane in (0, bad_lane - 1, lanes - 1):
        check_lane(oracle, sess.engine, inputs, lane, players, MAXP, CD, DELAY, frames)
