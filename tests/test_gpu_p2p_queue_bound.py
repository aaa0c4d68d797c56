"""GPU parity of the scheduled P2P engine (p2p_sched.hip) at the reference's 128-entry InputQueue
(input_queue.rs:6, :207) and under events bytes with bits at or above num_players.

The bound: every case is one engine of 200 sessions, each with its own rung of
tests/queue_bound_schedules.py -- the stall ladder (a silence of L = 100 .. 149 calls, then the
burst), the rate runs (remote inputs 1 .. 5 calls late for 320 calls: a lockstep session falls a
frame behind every two calls), the catch-up ladder (remote inputs ahead of a session far behind its
calls) -- or a jittered network with a disconnect (schedules() of test_gpu_p2p_sched.py, 300
calls).  EVERY session's state, ring, counts, frames, skips and error are bit-exact against
oracle.p2p_sched_run (check_sessions), whose stopping call tests/test_input_queue_model.py pins;
each case first asserts on the oracle alone that it straddles the bound.

The events: bits at or above num_players name no player and are dropped where the bytes enter
device memory (bit 4 of a stored byte is the scheduled kernels' own peer-report flag)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import packet_emit_model as E  # noqa: E402
from tests import packet_feed_model as F  # noqa: E402
from tests import queue_bound_schedules as B  # noqa: E402
from tests.test_gpu_p2p_sched import FORMS, check_sessions, peer_report_schedules, schedules, set_form  # noqa: E402

pytestmark = pytest.mark.gpu

S, CALLS = 200, B.RATE_CALLS
PIECES = (37, 64, 99, 120)


@functools.lru_cache(maxsize=None)
def bound_case(P, local, delay, mp, sparse=False, rungs_only=False):
    """rows [CALLS][S][P], arrive, events [CALLS][S], the rung of every session ((kind, value);
    ("jitter", i) for the jittered ones) and the oracle's stopping call per session (-1: it runs
    through)."""
    from oracle import oracle as o
    mask = sum(1 << k for k in local)
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0xB0D), CALLS, P, 1) for s in range(S)], axis=1)
    n_rungs = S if rungs_only else len(B.RUNGS)
    arrive, labels = B.rung_table(n_rungs, CALLS)
    events = np.zeros((CALLS, S), np.uint8)
    if not rungs_only:
        ja, je = schedules(S - n_rungs, B.JITTER_CALLS, 8, 41 + P + delay + mp, mask, P)
        ja = np.concatenate([ja, np.repeat(ja[-1:], CALLS - B.JITTER_CALLS, axis=0)])
        arrive = np.concatenate([arrive, ja], axis=1)
        events[:B.JITTER_CALLS, n_rungs:] = je
        labels = labels + [("jitter", i) for i in range(S - n_rungs)]
    return rows, np.ascontiguousarray(arrive), events, labels, oracle_stops(rows, arrive, events, P, mask, delay, mp, sparse)


def oracle_stops(rows, arrive, events, P, mask, delay, mp, sparse=False):
    from oracle import oracle as o
    stop = np.full(arrive.shape[1], -1, np.int32)
    for s in range(arrive.shape[1]):
        out = o.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=mask,
                              input_delay=delay, max_prediction=mp, sparse_saving=sparse)
        assert out["rc"] in (0, -4), (s, out["rc"])
        if out["rc"] == -4:
            stop[s] = out["result"].frames_done
    return stop


def assert_straddles(labels, stop, ladders=("stall", "catch_up")):
    """Conditions on the oracle alone: the case has sessions on both sides of the bound, and on each
    ladder the last rung that survives its burst and the first that stops there."""
    assert (stop >= 0).sum() >= 20 and (stop < 0).sum() >= 20, ((stop >= 0).sum(), (stop < 0).sum())
    burst = dict(stall=lambda L: 20 + L, catch_up=lambda u: 141)
    for kind in ladders:
        at = {v: stop[s] == burst[kind](v) for s, (k, v) in enumerate(labels) if k == kind}
        assert any(not at[v] and at.get(v + 1, False) for v in at), (kind, at)


def run_engine(P, local, delay, mp, rows, arrive, events, pieces=PIECES, sparse=False, **kw):
    from ggrs_amd import P2PEngine
    eng = P2PEngine(arrive.shape[1], num_players=P, local_players=local, input_delay=delay, max_prediction=mp,
                    remote_latency=1, input_capacity=CALLS, **kw)
    if sparse:
        eng.set_sparse_saving(True)
    eng.set_arrival_schedule(True)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    for n in pieces:
        eng.advance_frames(n)
    assert sum(pieces) == CALLS
    return eng


def assert_stops(eng, stop):
    """The sessions with an error are the oracle's, each at the oracle's frame count so far: a session
    stopped at call c has run c calls (frames + skipped)."""
    from ggrs_amd._lib import GGRS_E_PRECONDITION
    frames, skipped, errors = eng.sessions()
    assert ((errors == GGRS_E_PRECONDITION) == (stop >= 0)).all(), np.nonzero((errors != 0) != (stop >= 0))[0]
    assert (errors[stop < 0] == 0).all()
    ran = frames + skipped
    assert (ran[stop >= 0] == stop[stop >= 0]).all(), np.nonzero((ran != stop) & (stop >= 0))[0]


@pytest.mark.parametrize("P,local,delay", [(2, (0,), 0), (2, (1,), 2), (4, (1, 3), 0), (3, (), 0)])
def test_lockstep_sessions_stop_at_the_oracles_call(oracle, P, local, delay):
    """Lockstep mode: last_confirmed_frame follows the current frame, so the queue's tail stands at
    current - 2 and the session stops with the newest remote frame 126 past its current one."""
    rows, arrive, events, labels, stop = bound_case(P, local, delay, 0)
    assert_straddles(labels, stop)
    eng = run_engine(P, local, delay, 0, rows, arrive, events)
    assert_stops(eng, stop)
    check_sessions(eng, rows, arrive, events, range(S), CALLS)


def test_max_prediction_1_is_no_engine_configuration(oracle):
    """The smallest rollback window the engine takes is 2: ggrs_p2p_engine_create wants remote_latency
    in 1 .. max_prediction - 1 (tests/test_abi.py pins that), also for an engine that then switches to
    arrival schedules.  max_prediction 1 is therefore checked on the oracle and the queue model alone
    (tests/test_input_queue_model.py); the rollback cases here start at 2."""
    from ggrs_amd import InvalidRequest, P2PEngine
    with pytest.raises(InvalidRequest):
        P2PEngine(S, num_players=2, local_players=(0,), max_prediction=1, remote_latency=1, input_capacity=CALLS)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mp", [2, 3, 8, 40])
def test_rollback_sessions_stop_at_the_oracles_call(oracle, monkeypatch, form, mp):
    set_form(monkeypatch, form)
    rows, arrive, events, labels, stop = bound_case(2, (0,), 0, mp)
    # (max_prediction 40: last_confirmed_frame is 40 after the catch-up ladder's silence, and its
    # rungs, frames up to 140, stay below 40 - 1 + 128)
    assert_straddles(labels, stop, ("stall",) if mp == 40 else ("stall", "catch_up"))
    eng = run_engine(2, (0,), 0, mp, rows, arrive, events)
    assert_stops(eng, stop)
    check_sessions(eng, rows, arrive, events, range(S), CALLS)


def test_rollback_sparse_saving(oracle, monkeypatch):
    set_form(monkeypatch, "flat")
    P, local, delay, mp = 4, (1,), 1, 8
    rows, arrive, events, labels, stop = bound_case(P, local, delay, mp, True)
    assert_straddles(labels, stop)
    eng = run_engine(P, local, delay, mp, rows, arrive, events, sparse=True)
    assert_stops(eng, stop)
    check_sessions(eng, rows, arrive, events, range(S), CALLS, sparse_saving=True)


@pytest.mark.parametrize("split", ["0", "1"])
def test_rollback_flat_one_and_two_waves(oracle, monkeypatch, split):
    set_form(monkeypatch, "flat")
    monkeypatch.setenv("GGRS_SCHED_SPLIT", split)
    P, local, delay, mp = 2, (1,), 2, 8
    rows, arrive, events, labels, stop = bound_case(P, local, delay, mp)
    assert_straddles(labels, stop)
    eng = run_engine(P, local, delay, mp, rows, arrive, events)
    assert_stops(eng, stop)
    check_sessions(eng, rows, arrive, events, range(S), CALLS)


# The stall ladder's stopping calls are 146 .. 169 (20 + L, L = 126 .. 149), the catch-up ladder's 141
# and the rate runs' (lockstep) 253 .. 257: launches that begin at, end with and cross them.
@pytest.mark.parametrize("pieces", [(141, 5, 1, 63, 64, 46), (142, 5, 23, 84, 3, 63), (1, 63, 64, 192)],
                         ids=["first", "last", "mid-stage"])
@pytest.mark.parametrize("mp", [0, 8])
def test_stopping_call_first_last_and_inside_a_launch(oracle, pieces, mp):
    rows, arrive, events, labels, stop = bound_case(2, (0,), 0, mp)
    starts = np.cumsum((0,) + pieces)
    if pieces[0] == 141:
        assert {141, 146, 147}.issubset(set(starts)) and {141, 146, 147}.issubset(set(stop))  # first in a launch
    elif pieces[0] == 142:
        assert {141, 146, 169}.issubset(set(starts - 1)) and {141, 146, 169}.issubset(set(stop))  # last in a launch
        assert mp or 253 in set(starts - 1) and 253 in set(stop)
    eng = run_engine(2, (0,), 0, mp, rows, arrive, events, pieces=pieces)
    assert_stops(eng, stop)
    check_sessions(eng, rows, arrive, events, range(S), CALLS)


@pytest.mark.parametrize("form", FORMS)
def test_first_burst_at_the_widest_delivery_code(oracle, monkeypatch, form):
    """Silent sessions whose first burst is 253, 254 and 255 frames (the call record's delivery count
    saturates at 254, kArrTooFar), beside bursts of 126 .. 130 frames around the queue's 128."""
    set_form(monkeypatch, form)
    from oracle import oracle as o
    P, mp, n = 2, 8, 64
    bursts = [(253, 254, 255, 126, 127, 128, 129, 130)[s % 8] for s in range(n)]
    arrive = np.stack([B.silent_start(b, CALLS) for b in bursts], axis=1)
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0xB0D), CALLS, P, 1) for s in range(n)], axis=1)
    events = np.zeros((CALLS, n), np.uint8)
    stop = oracle_stops(rows, arrive, events, P, 0b01, 0, mp)
    assert [int(stop[s]) for s in range(8)] == [253, 254, 255, -1, -1, -1, 129, 130]
    eng = run_engine(P, (0,), 0, mp, rows, arrive, events, pieces=(253, 1, 1, 65))
    assert_stops(eng, stop)
    check_sessions(eng, rows, arrive, events, range(n), CALLS)


@pytest.mark.parametrize("mp", [0, 8])
def test_display_trace_up_to_the_stopping_call(oracle, monkeypatch, mp):
    set_form(monkeypatch, "flat")
    P, local, delay = 3, (0,), 0
    rows, arrive, events, labels, stop = bound_case(P, local, delay, mp)
    assert_straddles(labels, stop)
    eng = run_engine(P, local, delay, mp, rows, arrive, events, trace_capacity=CALLS)
    assert_stops(eng, stop)
    tr = eng.trace(0, CALLS)
    for s in range(S):
        out = oracle.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=0b001,
                                   max_prediction=mp)
        done = out["result"].frames_done
        assert done == (stop[s] if stop[s] >= 0 else CALLS)
        assert (tr[:done, s] == out["ck_trace"][:done]).all(), (s, int(np.argmax(tr[:done, s] != out["ck_trace"][:done])))
    check_sessions(eng, rows, arrive, events, range(0, S, 7), CALLS)


def test_packet_fed_lockstep_ladder(oracle):
    """The lockstep ladders as wire packets of up to 128 frames (tests/packet_feed_model.py's sender;
    a longer burst arrives as its first 128 frames): the packet-fed engine equals the table-fed one
    and the oracle under the table the feed wrote."""
    from tests.test_gpu_p2p_packets import assert_same, engines, run_pair
    P, local, mp, W = 2, (0,), 0, 128
    rows, arrive, events, labels, _ = bound_case(P, local, 0, mp, rungs_only=True)
    m = F.run(rows, arrive, 0b01, mp, max_packet_inputs=W, seed=3)
    assert (m["stop_call"] < 0).all() and (m["rows"] == rows).all()
    stop = oracle_stops(rows, m["arrive"], events, P, 0b01, 0, mp)
    assert (stop >= 0).sum() >= 20
    at = {v: stop[s] == 20 + v for s, (k, v) in enumerate(labels) if k == "stall"}
    assert any(not at[v] and at.get(v + 1, False) for v in at), at
    A, Bt = engines(S, P, local, mp, CALLS, W=W)
    assert run_pair(A, Bt, rows, m, events, PIECES, 0b01) == CALLS
    assert_same(A, Bt)
    status, ack = A.packet_results(0, CALLS)
    assert (status == m["status"]).all() and (ack == m["ack"]).all()
    assert_stops(A, stop)
    check_sessions(A, rows, m["arrive"], events, range(S), CALLS)


def test_packet_emit_stops_with_the_session(oracle, monkeypatch):
    """Packet emit on: a session's emit rows say "stopped" from the oracle's stopping call on (nothing
    is emitted from there, the pending inputs stay as they were), against tests/packet_emit_model.py."""
    from tests.test_gpu_p2p_emit import assert_emitted, assert_state, pushed_table
    set_form(monkeypatch, "flat")
    P, local, delay, mp, W = 2, (0,), 0, 0, 64
    rows, arrive, events, labels, stop = bound_case(P, local, delay, mp)
    assert_straddles(labels, stop)
    pushed, pstop = pushed_table(oracle, rows, arrive, events, P, 0b01, delay, mp)
    assert (pstop == stop).all()
    ack = np.maximum(np.maximum.accumulate(pushed, axis=0) - 2, -1).astype(np.int32)
    m = E.run(rows, pushed, 0b01, W, F.max_packet_bytes(1, W), ack, None, events,
              recv=np.maximum.accumulate(arrive, axis=0), stop_call=stop)
    from ggrs_amd import P2PEngine
    eng = P2PEngine(S, num_players=P, local_players=local, input_delay=delay, max_prediction=mp, remote_latency=1,
                    input_capacity=CALLS)
    eng.set_arrival_schedule(True)
    eng.set_packet_emit(W)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    got = []
    done = 0
    for n in PIECES:
        eng.advance_frames(n)
        got.append(eng.emit_packets(done, n, ack[done:done + n]))
        done += n
    got = tuple(np.concatenate([g[i] for g in got]) for i in range(4))
    assert_emitted(got, m)
    assert_state(eng, m)
    for s in np.nonzero(stop >= 0)[0]:
        c = int(stop[s])
        assert (got[0][c:, s] == -1).all() and (got[1][c:, s] == 0).all(), s
        assert c == 0 or (got[0][:c, s] >= 0).any(), s
    assert_stops(eng, stop)


# ---------------------------------------------------------------- events bytes

EV_S, EV_CALLS = 96, 160


def stray_bits(events, P, seed):
    """events with, on about one call in ten, random bits among 4 .. 7 and P .. 3 set as well."""
    rng = np.random.default_rng(seed)
    high = sum(1 << b for b in range(P, 8))
    stray = rng.integers(1, 256, events.shape).astype(np.uint8) & high
    out = np.where(rng.random(events.shape) < 0.1, events | stray, events).astype(np.uint8)
    assert (out & 0xf0).any() and (out & (0x0f & high)).any() and ((out & 0x10) != 0).sum() > events.shape[1]
    return out


@functools.lru_cache(maxsize=None)
def events_case(P, local, mp, with_reports=False):
    from oracle import oracle as o
    mask = sum(1 << k for k in local)
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0xE7), EV_CALLS, P, 1) for s in range(EV_S)], axis=1)
    reports = None
    if with_reports:
        arrive, events, reports = peer_report_schedules(EV_S, EV_CALLS, mp, 29, P, mask)
    else:
        arrive, events = schedules(EV_S, EV_CALLS, mp, 5 + P, mask, P, disconnect_every=3)
    return rows, arrive, stray_bits(events, P, 7 + P), reports


def run_events_engine(P, local, mp, rows, arrive, events, reports=None, sparse=False, **kw):
    from ggrs_amd import P2PEngine
    eng = P2PEngine(EV_S, num_players=P, local_players=local, max_prediction=mp, remote_latency=1,
                    input_capacity=EV_CALLS, **kw)
    if sparse:
        eng.set_sparse_saving(True)
    eng.set_arrival_schedule(True)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    if reports is not None:
        eng.add_peer_reports(0, reports)
    for n in (37, 64, 59):
        eng.advance_frames(n)
    return eng


@pytest.mark.parametrize("P,local", [(2, (0,)), (3, (1,))])
def test_stray_event_bits_chains(oracle, monkeypatch, P, local):
    """The time-aligned form has no reports table: a stored bit 4 would read through a null pointer."""
    set_form(monkeypatch, "chains")
    rows, arrive, events, _ = events_case(P, local, 8)
    eng = run_events_engine(P, local, 8, rows, arrive, events)
    check_sessions(eng, rows, arrive, events, range(EV_S), EV_CALLS)
    frames, skipped, errors = eng.sessions()
    assert (errors == 0).sum() > EV_S // 2


@pytest.mark.parametrize("P,local", [(2, (1,)), (3, (0,))])
def test_stray_event_bits_flat_sparse(oracle, monkeypatch, P, local):
    set_form(monkeypatch, "flat")
    rows, arrive, events, _ = events_case(P, local, 8)
    eng = run_events_engine(P, local, 8, rows, arrive, events, sparse=True)
    check_sessions(eng, rows, arrive, events, range(EV_S), EV_CALLS, sparse_saving=True)


@pytest.mark.parametrize("P,local", [(2, (0,)), (3, (0, 2))])
def test_stray_event_bits_flat_trace(oracle, monkeypatch, P, local):
    set_form(monkeypatch, "flat")
    rows, arrive, events, _ = events_case(P, local, 8)
    eng = run_events_engine(P, local, 8, rows, arrive, events, trace_capacity=EV_CALLS)
    check_sessions(eng, rows, arrive, events, range(EV_S), EV_CALLS)
    tr = eng.trace(0, EV_CALLS)
    for s in range(EV_S):
        out = oracle.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=eng.local_mask,
                                   max_prediction=8)
        done = out["result"].frames_done
        assert (tr[:done, s] == out["ck_trace"][:done]).all(), s


def test_stray_event_bits_beside_peer_reports(oracle, monkeypatch):
    """P = 3 with peer reports added (the reports table is allocated): a stray bit 4 on a call without
    a report must not be read as one (a zero report would mark player 0 reported by player 0)."""
    set_form(monkeypatch, "flat")
    P, local, mp = 3, (0,), 8
    rows, arrive, events, reports = events_case(P, local, mp, True)
    assert ((events & 0x10) != 0)[reports == 0].sum() > EV_S and (reports != 0).sum() > EV_S // 2
    eng = run_events_engine(P, local, mp, rows, arrive, events, reports=reports)
    check_sessions(eng, rows, arrive, events, range(EV_S), EV_CALLS, reports=reports)
    frames, skipped, errors = eng.sessions()
    assert (errors == 0).sum() > EV_S // 2


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("P,local", [(2, (0,)), (3, (1,))])
def test_stray_event_bits_through_the_packet_feed(oracle, P, local, on_device):
    """receive_packets' events, as a host array and as a device tensor the ingest kernel reads in
    place: the packet-fed engine equals the table-fed one and the oracle."""
    from tests.test_gpu_p2p_packets import assert_same, engines, garbage_rows
    mp = 8
    mask = sum(1 << k for k in local)
    rows, arrive, events, _ = events_case(P, local, mp)
    m = F.run(rows, arrive, mask, mp, seed=P)
    assert (m["arrive"] == arrive).all() and (m["rows"] == rows).all()
    A, Bt = engines(EV_S, P, local, mp, EV_CALLS)
    A.add_inputs(0, garbage_rows(rows, mask, 99))
    Bt.add_inputs(0, rows)
    Bt.add_arrivals(0, arrive, events)
    done = 0
    for n in (37, 64, 59):
        args = [m["start"][done:done + n], m["length"][done:done + n], m["packets"][done:done + n], events[done:done + n]]
        if on_device:
            args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
            torch.cuda.synchronize()  # torch's copies, before the engine's stream reads the tensors in place
        A.receive_packets(done, *args)
        A.advance_frames(n)
        Bt.advance_frames(n)
        A.synchronize()  # ... and the launch has read them before they are released
        done += n
    assert_same(A, Bt)
    check_sessions(A, rows, arrive, events, range(EV_S), EV_CALLS)
