"""GPU parity of the check_distance-8 SyncTest kernel's input-record table and one-block-ahead reads.

The core, edge and batch steps take their decoded input from a 16-entry table in LDS, indexed by
the raw byte's low four bits, and the producer reads a core block's bytes and records during the
block before it.  Bit-exact against the oracle's SyncTestSession, every lane (check_lane of
test_gpu_synctest): display checksums, final state, the saved-state ring.  cd 8, max_prediction 9,
input delay 2, the default path.

As in test_gpu_synctest_split, every case first advances cd + 1 frames in a call of its own (no
rollback yet: the sequential kernel); each listed launch is then one launch of the batched kernel.
"""
import numpy as np
import pytest

from tests.test_gpu_synctest import check_lane, lane_inputs, make_engine, run_chunks

MAXP, CD, DELAY = 9, 8, 2


def run_and_check(oracle, inputs, lanes, players, launches):
    frames = CD + 1 + sum(launches)
    assert inputs.shape == (frames, lanes, players)
    eng = make_engine(lanes, players, MAXP, CD, DELAY, frames)
    assert run_chunks(eng, inputs, [CD + 1] + launches) == frames
    assert eng.current_frame() == frames
    trace = eng.trace(0, frames)
    for lane in range(lanes):
        check_lane(oracle, eng, inputs, lane, players, MAXP, CD, DELAY, frames, trace)
    status, _, _ = eng.mismatches()
    assert (status == 0).all()


def nibble_cycle(frames, lanes, players):
    """Every low-nibble value on every player: any 8 consecutive frames of the 8 lanes together
    hold all 16 (the edge blocks), any 16 frames of one lane do (the core blocks, the batches)."""
    f, l, p = np.meshgrid(np.arange(frames), np.arange(lanes), np.arange(players), indexing="ij")
    return ((f + 2 * l + 7 * p) & 15).astype(np.uint8)


@pytest.fixture(scope="module")
def table_inputs():
    lanes, players, frames = 8, 2, CD + 1 + 64
    low = nibble_cycle(frames, lanes, players)
    for p in range(players):
        for lo, hi in ((0, 8), (frames - 8, frames), (CD + 1, CD + 9)):
            assert set(low[lo:hi, :, p].ravel().tolist()) == set(range(16))
        assert all(set(low[20:36, lane, p].tolist()) == set(range(16)) for lane in range(lanes))
    high = np.random.default_rng(4321).integers(0, 16, size=low.shape).astype(np.uint8) << 4
    assert (high != 0).any()
    return low, low | high


def test_oracle_ignores_the_high_nibble(oracle, table_inputs):
    """CPU only: the reference reads bits 0..3 of an input byte, so the two input sets of
    test_every_table_entry describe the same sessions."""
    low, full = table_inputs
    for lane in range(low.shape[1]):
        a = oracle.synctest_run(low[:, lane, :], 2, MAXP, CD, DELAY)
        b = oracle.synctest_run(full[:, lane, :], 2, MAXP, CD, DELAY)
        assert a["result"].status == 0 and b["result"].status == 0
        assert (a["cksum"] == b["cksum"]).all()
        assert bytes(a["final_state"]) == bytes(b["final_state"])
        assert a["ring_frames"].tolist() == b["ring_frames"].tolist()
        assert (a["ring_cksums"] == b["ring_cksums"]).all()
        assert all(bytes(x) == bytes(y) for x, y in zip(a["ring_states"], b["ring_states"]))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["low_nibble", "high_nibble_set"])
def test_every_table_entry(oracle, table_inputs, which):
    """One 64-frame launch whose inputs cycle through all 16 table entries on both players, in the
    core, edge and batch steps; then the same with random high nibbles, which the table's index
    mask must drop as make_input_rec does."""
    inputs = table_inputs[0] if which == "low_nibble" else table_inputs[1]
    run_and_check(oracle, inputs, 8, 2, [64])


# 528 raw rows are held at once and a launch of n frames needs n + cd of them: 520 is the largest
# launch without a re-read; the others re-read at step 512, the first of their last 2, 3 and 5
# core blocks, whose records were read ahead from the rows the re-read replaces
@pytest.mark.gpu
@pytest.mark.parametrize("n", [520, 528, 536, 552])
def test_read_ahead_at_the_raw_reread(oracle, n):
    lanes, players = 4, 2
    inputs = lane_inputs(oracle, 5100 + n, lanes, CD + 1 + n, players, 0)
    run_and_check(oracle, inputs, lanes, players, [n])


# [16]: no core block (the producer passes publish() and the barriers without reading ahead);
# [24]: one core block, read ahead of publish() only; [16, 16]: back to back
@pytest.mark.gpu
@pytest.mark.parametrize("launches", [[16], [24], [16, 16]], ids=["16", "24", "16_16"])
def test_first_and_last_block_read_ahead(oracle, launches):
    lanes, players = 5, 2
    inputs = lane_inputs(oracle, 5200 + len(launches) + launches[0], lanes, CD + 1 + sum(launches), players, 0)
    run_and_check(oracle, inputs, lanes, players, launches)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 136])
@pytest.mark.parametrize("players,lanes", [(1, 13), (3, 10), (4, 6)])
def test_one_wave_kernel_with_the_table(oracle, players, lanes, n):
    inputs = lane_inputs(oracle, 5300 + players, lanes, CD + 1 + n, players, 0)
    run_and_check(oracle, inputs, lanes, players, [n])


@pytest.mark.gpu
def test_launches_after_a_failed_launch_return_before_reading_ahead(oracle):
    """A mismatch in the second 24-frame launch (one core block each): the later launches find the
    failure recorded and both waves leave through the early returns, which sit ahead of the first
    block's read-ahead and of publish(); the failing lane is not running from then on.  Error
    frame, mask and halted state as the reference session; the other lanes as the oracle."""
    from ggrs_amd import MismatchedChecksum, SessionBuilder
    players, frames, lanes, bad_lane, chunk, call = 2, 120, 70, 66, 24, 30
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
    assert (st[np.arange(lanes) != bad_lane] == 0).all()
    for lane in (0, bad_lane - 1, bad_lane + 1, lanes - 1):
        check_lane(oracle, sess.engine, inputs, lane, players, MAXP, CD, DELAY, frames)
