"""CPU checks of tests/time_sync_model.py, the reference of the device's time sync
(ggrs_p2p_set_time_sync / time_sync): the reference's own time_sync.rs unit tests, the f32 average
where exact integers would differ, the spacing of recommendations, the closing call, the claim the
kernel rests on (current_frame = the local players' last queued frame - input_delay, against the
oracle's session) -- and the inputs of the GPU parity test (tests/test_gpu_time_sync.py), so that the
conditions that test relies on are asserted here on the model alone."""
import functools

import numpy as np
import pytest

from tests import time_sync_model as T

S, CALLS, FPS = 130, 240, 60
SEED = 5


@pytest.mark.parametrize("local_adv,remote_adv,want", [(0, 0, 0), (5, -5, -5), (-1, 1, 1), (-4, 4, 4), (-40, 40, 40)])
def test_reference_unit_tests(local_adv, remote_adv, want):
    """time_sync.rs's sync_layer_tests: 60 pushes of one pair."""
    ts = T.TimeSync()
    for i in range(60):
        ts.advance_frame(i, local_adv, remote_adv)
    assert ts.average_frame_advantage() == want


def test_f32_average_is_not_the_exact_one():
    """Window sums -400 and -220: -7.3333335f - -13.333333f = 5.9999995f, halved and truncated 2; in
    exact integers 180 / 60 = 3, MIN_RECOMMENDATION."""
    ts = T.TimeSync()
    ts.local = [-13] * 20 + [-14] * 10
    ts.remote = [-7] * 20 + [-8] * 10
    assert (sum(ts.local), sum(ts.remote)) == (-400, -220)
    assert ts.average_frame_advantage() == 2 and ts.exact_average() == 3
    x = T.Session()
    x.endpoint.time_sync = ts
    assert x.step(0, 100, 99, T.NULL_FRAME) == (-1, 2, 0)  # no recommendation at 2


def test_recommendations_are_at_least_61_frames_apart():
    """The peer reports itself 20 frames ahead throughout: the window average reaches 3 with nine
    entries, then `cur > next_recommended_sleep` lets one through every 61 frames."""
    x = T.Session()
    at = []
    for c in range(200):
        local, ahead, skip = x.step(c, c, c - 1, c, remote_advantage=20 if c == 0 else T.KEEP)
        assert skip in (0, ahead)
        if skip:
            at.append(c)
    assert at == [9, 70, 131, 192] and x.next_recommended_sleep == 252
    # a session that no longer advances is not asked again: cur stays below next_recommended_sleep
    for c in range(200, 330):
        assert x.step(c, 199, 198, T.NULL_FRAME)[2] == 0


def test_closing_call():
    """The advantage is updated by the closing call's poll; frames_ahead is 0 from it on; nothing is
    pushed or taken in any more."""
    x = T.Session()
    for c in range(40):
        x.step(c, c, max(c - 2, -1), c, rtt_ms=100 if c == 0 else -1, remote_advantage=9 if c == 0 else T.KEEP)
    ep = x.endpoint
    assert ep.local_frame_advantage == 37 + 3 - 39 and x.frames_ahead == 4  # (ping 50 ms: 3 frames)
    before = (list(ep.time_sync.local), list(ep.time_sync.remote))
    assert x.step(40, 40, 35, 40, close=True) == (35 + 3 - 40, 0, 0)
    assert (ep.time_sync.local, ep.time_sync.remote) == before and ep.closed_call == 40
    assert x.step(41, 41, 41, 41, rtt_ms=1000, remote_advantage=-30) == (-2, 0, 0)
    assert (ep.round_trip_time, ep.remote_frame_advantage, ep.time_sync.local) == (100, 9, before[0])


def test_intake_clamps():
    x = T.Session()
    x.step(0, 0, T.NULL_FRAME, 0, rtt_ms=1 << 30, remote_advantage=40000)
    assert (x.endpoint.round_trip_time, x.endpoint.remote_frame_advantage) == (1 << 20, 32767)
    assert x.endpoint.local_frame_advantage == 0  # nothing received yet: not updated
    x.step(1, 1, 0, 1, remote_advantage=-40000)
    assert x.endpoint.remote_frame_advantage == -32768
    assert x.endpoint.local_frame_advantage == 0 + ((1 << 19) * 60) // 1000 - 1


@pytest.mark.parametrize("delay,mp", [(0, 8), (2, 8), (0, 0), (2, 0)])
def test_current_frame_is_last_queued_frame_minus_delay(oracle, delay, mp):
    """The kernel derives current_frame from the word the scheduled kernels store, the local players'
    last queued frame after the call (modelled as packet_emit_model.pushes models it): equal to the
    oracle's current_frame at the call's start + input_delay at every call, accepted or dropped, in
    rollback and in lockstep mode, through stalls at the prediction threshold."""
    calls = 240
    skipped = 0
    for s in range(12):
        rows = oracle.gen_inputs(oracle.session_seed(s, 0x7153), calls, 2, 0)
        arrive = oracle.stall_schedule(calls, max(mp, 8), 900 + s, stall_every=40 if s % 2 else 10 ** 9)
        out = oracle.p2p_sched_run(rows, arrive, None, num_players=2, local_mask=0b01, input_delay=delay,
                                   max_prediction=mp)
        assert out["rc"] == 0 and set(np.unique(out["advanced"])) <= {0, 1}
        adv = out["advanced"][:, None]
        cur, pushed = T.tables(adv, delay)
        assert cur[-1, 0] + adv[-1, 0] == out["current_frame"]
        ll = np.maximum.accumulate(pushed[:, 0])  # emit_ll: the last queued frame after each call
        assert (ll - delay == cur[:, 0]).all()
        skipped += out["skips"]
    assert skipped > 0


def oracle_tables(rows, arrive, events, P, mask, delay, mp):
    """(advanced [calls][S], stop_call [S]) from the oracle's P2PSession per session."""
    from oracle import oracle as o
    calls, S_ = arrive.shape
    advanced = np.zeros((calls, S_), np.uint8)
    stop = np.full(S_, -1, np.int32)
    for s in range(S_):
        out = o.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=mask,
                              input_delay=delay, max_prediction=mp)
        if out["rc"] != 0:
            stop[s] = out["result"].frames_done
        advanced[:, s] = out["advanced"]
    return advanced, stop


@functools.lru_cache(maxsize=None)
def parity_case(P, local, delay, mp, S_=S, calls=CALLS, seed=SEED):
    """The GPU parity test's inputs and the model's run of them: (rows, arrive, events, rtt_ms,
    remote_advantage, the model's outputs with the sessions' current_frame table `cur`).  The schedules are tests/test_gpu_p2p_emit.py's."""
    from oracle import oracle as o
    from tests.test_gpu_p2p_sched import schedules
    mask = sum(1 << k for k in local)
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0x7153), calls, P, 0) for s in range(S_)], axis=1)
    arrive, events = schedules(S_, calls, max(mp, 8), 19 + P + delay + seed, mask, P)
    advanced, stop = oracle_tables(rows, arrive, events, P, mask, delay, mp)
    cur, pushed = T.tables(advanced, delay, stop)
    rtt, radv = T.input_tables(S_, calls, seed)
    m = T.run(cur, pushed, np.maximum.accumulate(arrive, axis=0), events, ~mask & ((1 << P) - 1), FPS, rtt, radv, stop)
    m["cur"] = cur
    return rows, arrive, events, rtt, radv, m


def proves_something(m):
    """The conditions under which a parity run over the model's outputs `m` shows the feature."""
    skip = m["skip_frames"]
    S_ = skip.shape[1]
    recs = (skip > 0).sum(axis=0)
    assert (recs >= 2).sum() >= S_ // 4, (recs >= 2).sum()
    assert (recs == 0).sum() >= S_ // 8, (recs == 0).sum()
    assert (m["state"][4] >= 0).sum() > 5  # closed endpoints
    assert m["state"][6].sum() >= 8        # (call, session) pairs where the f32 average is not the exact one
    assert (m["frames_ahead"] < 0).any() and (m["local_advantage"] > 0).any() and (m["local_advantage"] < 0).any()


def exactly_61_apart(m, cur):
    """Sessions with two consecutive recommendations exactly 61 frames apart."""
    out = []
    for s in range(cur.shape[1]):
        at = cur[m["skip_frames"][:, s] > 0, s]
        if (np.diff(at) == 61).any():
            out.append(s)
    return out


def test_the_parity_inputs_prove_something(oracle):
    rows, arrive, events, rtt, radv, m = parity_case(2, (0,), 0, 8)
    proves_something(m)
    assert exactly_61_apart(m, m["cur"])
    assert (radv == 40000).sum() == 1 and (np.abs(radv) == 32767).sum() == 4
