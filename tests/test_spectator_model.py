"""CPU checks of the spectator restatement (tests/spectator_model.py) and of the spectator engine's
configuration checks, which run before the device is touched (include/ggrs_amd.h,
ggrs_spectator_engine_create; SessionBuilder.with_max_frames_behind / with_catchup_speed)."""
import numpy as np
import pytest

from tests import spectator_model as M


@pytest.mark.parametrize("P", [1, 2, 4])
def test_model_in_step_is_a_plain_fold(oracle, P):
    """Every frame delivered before its call, speed 1: one AdvanceFrame per call, no waits."""
    calls = 50
    rows = oracle.gen_inputs(oracle.session_seed(P, 0x57EC), calls, P)
    out = M.run(rows, np.arange(calls), num_players=P)
    state = oracle.state_new(P)
    for f in range(calls):
        state = oracle.state_advance(state, rows[f])
        assert out["advanced"][f] == 1
        assert out["checksums"][f] == oracle.fletcher16(state), f
    assert bytes(out["state"]) == bytes(state)
    assert (out["current_frame"], out["last_recv"], out["waited"], out["error"]) == (calls - 1, calls - 1, 0, 0)


def test_model_catchup_wait_and_too_far_behind(oracle):
    P = 2
    rows = oracle.gen_inputs(7, 200, P)
    # nothing for 5 calls, then frames 0..19 at once: behind 20, 17, 14, 11 > 10 -> 3 per call, then 8 -> 1
    recv = np.array([-1] * 5 + [19] * 10, np.int32)
    out = M.run(rows, recv, num_players=P, max_frames_behind=10, catchup_speed=3)
    assert out["waited"] == 5
    assert list(out["advanced"]) == [0] * 5 + [3, 3, 3, 3, 1, 1, 1, 1, 1, 1]
    # the host 60 frames ahead of the frame to grab: lost for good, while frames keep arriving
    out = M.run(rows, np.array([59, 61, 62, 62], np.int32), num_players=P)
    assert list(out["advanced"]) == [1, 0, 0, 0] and out["error"] == M.E_TOO_FAR_BEHIND
    assert out["current_frame"] == 0 and out["last_recv"] == 62 and out["waited"] == 0


def test_model_note_needs_an_input_event(oracle):
    """A note is visible only with an Event::Input: it takes effect at the first call at or after
    its own that delivers a frame, and marks the player Disconnected for frames after last_frame."""
    P = 2
    rows = oracle.gen_inputs(9, 40, P)
    recv = np.array([0, 1, 2, 2, 2, 5, 6, 7], np.int32)
    notes = np.zeros(8, np.int32)
    notes[3] = M.note(1, 3)  # arrives with a message that carries no new frame
    out = M.run(rows, recv, notes, num_players=P)
    state = oracle.state_new(P)
    for f in range(6):  # calls 0-2 advance 0-2, calls 3-4 wait, call 5 advances 3, 6 -> 4, 7 -> 5
        status = [0, M.STATUS_DISCONNECTED if f > 3 else 0]
        state = oracle.state_advance(state, rows[f], np.array(status, np.uint8))
    assert out["waited"] == 2 and out["current_frame"] == 5
    assert bytes(out["state"]) == bytes(state)


def test_model_stop_rules(oracle):
    P = 2
    rows = oracle.gen_inputs(11, 100, P)
    # an arrival naming a frame not yet added
    out = M.run(rows, np.array([0, 1, 50, 51], np.int32), num_players=P, windows=[(4, 0, 50)])
    assert out["error"] == M.E_INVALID and list(out["advanced"]) == [1, 1, 0, 0] and out["last_recv"] == 1
    # a needed row that left the window
    out = M.run(rows, np.array([0, 1, 30, 31], np.int32), num_players=P, windows=[(2, 0, 40), (2, 10, 74)])
    assert out["error"] == M.E_PRECONDITION and list(out["advanced"]) == [1, 1, 0, 0] and out["current_frame"] == 1


@pytest.mark.parametrize("P,D,mp,calls", [(2, 3, 8, 100), (4, 5, 8, 77), (3, 1, 6, 64)])
def test_model_matches_the_p2p_oracles_confirmed_state(oracle, P, D, mp, calls):
    """The oldest cell of a P2P session's ring (frame tag g) is confirmed: it equals the spectator's
    state after frames 0..g-1 of the same rows, in bytes and checksum.  (Newer cells still carry
    predictions and are not compared.)"""
    rows = oracle.gen_inputs(oracle.session_seed(P * 100 + D, 0x57EC), calls, P)
    out = oracle.p2p_run(rows, num_players=P, latency=D, max_prediction=mp)
    assert out["rc"] == 0
    frames = out["ring_frames"]
    held = [i for i in range(len(frames)) if frames[i] >= 0]
    i = min(held, key=lambda j: frames[j])
    g = int(frames[i])
    assert 0 < g < calls
    spec = M.run(rows, np.arange(g), num_players=P)
    assert spec["current_frame"] == g - 1
    assert bytes(spec["state"]) == bytes(out["ring_states"][i])
    assert spec["checksums"][g - 1] == out["ring_cksums"][i]


@pytest.mark.parametrize("kw,msg", [
    (dict(max_frames_behind=0), "Max frames behind cannot be smaller than 1"),
    (dict(max_frames_behind=60), "Max frames behind cannot be larger or equal"),
    (dict(catchup_speed=0), "Catchup speed cannot be smaller than 1"),
    (dict(catchup_speed=5, max_frames_behind=5), "Catchup speed cannot be larger or equal"),
    (dict(num_players=5), "num_players"),
    (dict(num_sessions=0), "num_sessions"),
])
def test_bad_spectator_config_rejected_without_device(engine_lib, kw, msg):
    from ggrs_amd import InvalidRequest, SpectatorEngine
    args = dict(num_sessions=4, num_players=2)
    args.update(kw)
    with pytest.raises(InvalidRequest, match=msg):
        SpectatorEngine(**args)


def test_builder_mirrors_the_reference_messages(engine_lib):
    """builder.rs:214-248, in the reference's order: each with_* checks on its own call, the catch-up
    speed against the max_frames_behind set so far."""
    from ggrs_amd import InvalidRequest, SessionBuilder
    with pytest.raises(InvalidRequest, match=r"Max frames behind cannot be smaller than 1\."):
        SessionBuilder().with_max_frames_behind(0)
    with pytest.raises(InvalidRequest,
                       match=r"Max frames behind cannot be larger or equal than the Spectator buffer size \(60\)"):
        SessionBuilder().with_max_frames_behind(60)
    with pytest.raises(InvalidRequest, match=r"Catchup speed cannot be smaller than 1\."):
        SessionBuilder().with_catchup_speed(0)
    with pytest.raises(InvalidRequest,
                       match="Catchup speed cannot be larger or equal than the allowed maximum frames behind host"):
        SessionBuilder().with_catchup_speed(10)  # the default max_frames_behind is 10
    with pytest.raises(InvalidRequest, match="Catchup speed cannot be larger"):
        SessionBuilder().with_max_frames_behind(5).with_catchup_speed(5)
    b = SessionBuilder().with_max_frames_behind(59).with_catchup_speed(58)
    assert (b.max_frames_behind, b.catchup_speed) == (59, 58)
    # the defaults are valid, and a bad engine configuration behind the builder is still refused
    with pytest.raises(InvalidRequest, match="num_players"):
        SessionBuilder().with_num_players(5).with_num_lanes(4).start_spectator_session()
