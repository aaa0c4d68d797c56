"""GPU parity of the P2P engine's packet feed (ggrs_p2p_set_packet_feed / receive_packets /
read_packet_results, csrc/p2p_ingest.hip).  The scheme everywhere: engine A is fed by the wire
packets of tests/packet_feed_model.py's sender, with random garbage in the remote columns of its
add_inputs rows; engine B is fed the existing way, the rows as the model's receiver holds them plus
the model's effective arrival table.  Every session of A equals B (state, ring, sessions, stats),
and a third of them equal the oracle's P2PSession (check_sessions of tests/test_gpu_p2p_sched.py)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import packet_feed_model as M  # noqa: E402
from tests.test_gpu_p2p_sched import (CASES, check_sessions, peer_report_schedules, schedules,  # noqa: E402
                                      set_form)

pytestmark = pytest.mark.gpu

PIECES = (1, 3, 60, 17, 159)


def garbage_rows(rows, mask, seed):
    """rows with every remote column replaced by random bytes (the feed ignores them)."""
    out = rows.copy()
    cols = M.remote_columns(rows.shape[2], mask)
    out[:, :, cols] = np.random.default_rng(seed).integers(0, 256, out[:, :, cols].shape, dtype=np.uint8)
    return out


def engines(S, P, local, mp, cap, W=64, delay=0, pred=0, sparse=False, desync=0, stride=None, **kw):
    """(A, B): the packet-fed engine and the one fed arrival rows."""
    from ggrs_amd import P2PEngine
    out = []
    for feed in (True, False):
        e = P2PEngine(S, num_players=P, local_players=local, input_delay=delay, max_prediction=mp, remote_latency=1,
                      predictor=pred, input_capacity=cap, **kw)
        if sparse:
            e.set_sparse_saving(True)
        if desync:
            e.set_desync_detection(desync)
        e.set_arrival_schedule(True)
        if feed:
            e.set_packet_feed(W, stride)
        out.append(e)
    return out


def receive(eng, m, c0, n, events=None):
    eng.receive_packets(c0, m["start"][c0:c0 + n], m["length"][c0:c0 + n], m["packets"][c0:c0 + n],
                        None if events is None else events[c0:c0 + n])


def run_pair(A, B, rows, m, events, pieces, mask, reports=None):
    """Both engines over the same calls in the same pieces, every row added up front."""
    A.add_inputs(0, garbage_rows(rows, mask, 99))
    B.add_inputs(0, m["rows"])
    B.add_arrivals(0, m["arrive"], events)
    if reports is not None:
        B.add_peer_reports(0, reports)
    done = 0
    for n in pieces:
        receive(A, m, done, n, events)
        if reports is not None:
            A.add_peer_reports(done, reports[done:done + n])
        A.advance_frames(n)
        B.advance_frames(n)
        done += n
    return done


def assert_same(A, B, errors_of_b=None):
    """Every session of A against B: states, rings, sessions and stats (errors_of_b: B's errors where
    they are not A's -- B stops a session through the arrival table's error; A's are the caller's)."""
    assert (A.states() == B.states()).all()
    fa, sa, ea = A.sessions()
    fb, sb, eb = B.sessions()
    assert (fa == fb).all() and (sa == sb).all()
    assert (eb == (ea if errors_of_b is None else errors_of_b)).all(), (ea, eb)
    for x, y in zip(A.stats(), B.stats()):
        assert (x == y).all()
    for s in range(A.num_sessions):
        for x, y in zip(A.ring(s), B.ring(s)):
            assert (x == y).all(), s


@functools.lru_cache(maxsize=None)
def parity_inputs(P, local, mp, model):
    from oracle import oracle as o
    S, calls = 200, 240
    mask = sum(1 << k for k in local)
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0x5C4E), calls, P, model) for s in range(S)], axis=1)
    arrive, events = schedules(S, calls, mp, 11 + P, mask, P)
    return rows, arrive, events, M.run(rows, arrive, mask, mp, seed=P + mp)


@pytest.mark.parametrize("form,P,local,delay,mp,pred,model,sparse",
                         [("chains",) + CASES[0]] + [("flat",) + c for c in CASES])
def test_packet_fed_sessions_match_the_schedule_fed_engine_and_the_oracle(oracle, monkeypatch, form, P, local, delay,
                                                                         mp, pred, model, sparse):
    """Undamaged packets with re-sent frames, launches and receive_packets split 1, 3, 60, 17, 159:
    the schedule's stalls, bursts and disconnects, as test_p2p_arrival_schedules_match_oracle."""
    set_form(monkeypatch, form)
    rows, arrive, events, m = parity_inputs(P, local, mp, model)
    calls, S = arrive.shape
    mask = sum(1 << k for k in local)
    assert (m["arrive"] == arrive).all() and (m["rows"] == rows).all()
    A, B = engines(S, P, local, mp, calls, delay=delay, pred=pred, sparse=sparse)
    assert run_pair(A, B, rows, m, events, PIECES, mask) == calls
    assert_same(A, B)
    status, ack = A.packet_results(0, calls)
    assert (status == m["status"]).all() and (ack == arrive).all()
    check_sessions(A, rows, arrive, events, range(0, S, 3), calls, sparse_saving=sparse)
    frames, skipped, errors = A.sessions()
    assert skipped.sum() > 0  # stalls past max_prediction: calls at the prediction threshold
    rb, _ = A.stats()
    assert rb.sum() > S


def test_live_loop_through_small_rings(oracle):
    """One add_inputs(1 row) + receive_packets(1) + advance_frames(1) per call over input_capacity 64:
    the row ring, the arrival ring and the reference-row lookup wrap several times."""
    S, calls, P, mp, cap = 70, 300, 2, 8, 64
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 0x11FE), calls, P, s % 2) for s in range(S)], axis=1)
    arrive, events = schedules(S, calls, mp, 3, 0b01, P, disconnect_every=0)
    m = M.run(rows, arrive, 0b01, mp, seed=4, cap=cap, row_hi=lambda c: c)
    assert (m["arrive"] == arrive).all()
    A, B = engines(S, P, (0,), mp, cap)
    junk = garbage_rows(rows, 0b01, 5)
    for c in range(calls):
        A.add_inputs(c, junk[c:c + 1])
        receive(A, m, c, 1)
        A.advance_frames(1)
        B.add_inputs(c, rows[c:c + 1])
        B.add_arrivals(c, arrive[c:c + 1])
        B.advance_frames(1)
    assert_same(A, B)
    status, ack = A.packet_results(calls - cap, cap)
    assert (status == m["status"][-cap:]).all() and (ack == arrive[-cap:]).all()
    check_sessions(A, rows, arrive, events, range(0, S, 3), calls)
    frames, skipped, errors = A.sessions()
    assert (errors == 0).all() and skipped.sum() > 0 and frames.min() > 3 * cap


@pytest.mark.parametrize("cap,stride", [(2100, None), (100, 1012), (60, 256)])
def test_kernel_staging_forms(oracle, cap, stride):
    """The ingest kernel's other staging shapes: an input_capacity whose row tags do not fit in LDS
    beside the packets (read from memory instead), the longest packet rows (one call staged at a
    time), and rows of which four calls are staged at a time; a receive_packets of 39 calls crosses
    several groups."""
    S, calls, P, mp = 70, 60, 3, 8
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 0x57A6), calls, P, 0) for s in range(S)], axis=1)
    arrive, events = schedules(S, calls, mp, 23, 0b010, P, disconnect_every=0)
    m = M.run(rows, arrive, 0b010, mp, seed=8, stride=stride)
    A, B = engines(S, P, (1,), mp, cap, stride=m["stride"])
    assert run_pair(A, B, rows, m, None, (1, 20, 39), 0b010) == calls
    assert_same(A, B)
    status, ack = A.packet_results(0, calls)
    assert (status == m["status"]).all() and (ack == arrive).all()
    check_sessions(A, rows, arrive, events, range(0, S, 3), calls)


def test_damaged_packets(oracle):
    """Every seventh session gets one damaged packet (truncated, random bytes, withheld, a stale
    duplicate, a reference no longer kept, a gap, frames beyond the call): status and ack of every
    (call, session) equal the model's; a dropped packet costs the session frames until the sender's
    next one; the sessions a packet stops stop at the model's call -- B through the arrival table's
    error at the same call; the undamaged sessions run their own schedule."""
    from ggrs_amd._lib import GGRS_E_INVALID
    P, mask, mp = 2, 0b01, 8
    rows, arrive, damage = M.damage_case(P=P, local_mask=mask, max_prediction=mp)
    calls, S = arrive.shape
    m = M.run(rows, arrive, mask, mp, seed=9, damage=damage)
    assert set(m["applied"].values()) == set(M.DAMAGE) | {"ahead"}
    A, B = engines(S, P, (0,), mp, calls)
    events = np.zeros((calls, S), np.uint8)
    assert run_pair(A, B, rows, m, None, (1, 3, 60, 17, 119), mask) == calls
    status, ack = A.packet_results(0, calls)
    assert (status == m["status"]).all(), np.argwhere(status != m["status"])[:5]
    assert (ack == m["ack"]).all()
    frames, skipped, errors = A.sessions()
    stopped = m["stop_call"] >= 0
    assert stopped.sum() >= 2 and (errors == m["error"]).all(), (errors, m["error"])
    assert (frames[stopped] <= m["stop_call"][stopped]).all()
    assert_same(A, B, errors_of_b=np.where(stopped, GGRS_E_INVALID, 0))
    damaged = sorted({s for _, s in damage})
    running = [s for s in range(S) if not stopped[s] and (s in damaged or s % 3 == 0)]
    check_sessions(A, m["rows"], m["arrive"], events, running, calls)
    for s in np.nonzero(stopped)[0]:  # up to the stopping call, the oracle's session
        c = int(m["stop_call"][s])
        out = oracle.p2p_sched_run(m["rows"][:c, s], m["arrive"][:c, s], None, num_players=P, local_mask=mask,
                                   max_prediction=mp)
        assert out["rc"] == 0 and bytes(A.state(s)) == bytes(out["final_state"]), s
        assert frames[s] == out["current_frame"] and skipped[s] == out["skips"], s
    undamaged = [s for s in range(S) if s not in damaged]
    assert (m["arrive"][:, undamaged] == arrive[:, undamaged]).all() and (m["rows"] == rows)[:, undamaged].all()
    assert (errors[undamaged] == 0).all()


@pytest.mark.parametrize("P,local", [(2, (0,)), (3, (0,))])
def test_recoded_packets(oracle, P, local):
    """Every third session gets, at several of its calls, the sender's packet in other bytes
    (tests/codec_cases.py's recode; 1 and 2 input bytes): runs split, zero-length runs, padded varints,
    input_sizes = Some(zero deltas) and bytes after the stream deliver as the packet would have (status
    1); Some(..) with uneven or negative sizes is dropped with UNSUPPORTED / E_DELTA.  Status and ack of
    every (call, session) equal the model's, A equals the schedule-fed B, the running sessions the
    oracle's."""
    import collections
    from tests import codec_cases as C
    mask, mp = sum(1 << k for k in local), 8
    rows, arrive, damage = M.recode_case(P, mask, max_prediction=mp)
    calls, S = arrive.shape
    m = M.run(rows, arrive, mask, mp, seed=9, damage=damage)
    plain = M.run(rows, arrive, mask, mp, seed=9)
    times = collections.Counter(m["applied"].values())
    assert set(times) == set(M.RECODE) and min(times.values()) >= 5, times
    assert (m["stop_call"] == -1).all()
    A, B = engines(S, P, local, mp, calls)
    events = np.zeros((calls, S), np.uint8)
    assert run_pair(A, B, rows, m, None, (1, 3, 60, 17, calls - 81), mask) == calls
    status, ack = A.packet_results(0, calls)
    assert (status == m["status"]).all(), np.argwhere(status != m["status"])[:5]
    assert (ack == m["ack"]).all()
    for (c, s), kind in m["applied"].items():
        want = 1 if kind in C.ACCEPTING else C.RECODE_STATUS[kind]
        assert status[c, s] == want, (c, s, kind, status[c, s])
    accepting = sorted({s for (_, s), kind in m["applied"].items() if kind in C.ACCEPTING})
    assert ((status == 1) == (plain["status"] == 1))[:, accepting].all() and (ack == arrive)[:, accepting].all()
    assert_same(A, B)
    frames, skipped, errors = A.sessions()
    assert (errors == 0).all()
    recoded = sorted({s for _, s in m["applied"]})
    check_sessions(A, m["rows"], m["arrive"], events, recoded + [s for s in range(1, S, 6)], calls)


def test_long_bursts_and_overlong_packets(oracle):
    """A stall of 40 calls, then one packet of 40+ frames (max_packet_inputs 64); every other
    session stalls for 66 calls and its sender's packet after the stall carries max_packet_inputs + 1
    frames: dropped whole with GGRS_CODEC_E_CAP, the frames arrive with the next packets."""
    S, calls, P, mp, W = 66, 130, 2, 8, 64
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 0xB0), calls, P, s % 2) for s in range(S)], axis=1)
    arrive = np.zeros((calls, S), np.int32)
    for s in range(S):
        a = np.arange(calls) - 1 - s % 3
        a[30:(96 if s % 2 else 70) + s % 5] = a[29]
        arrive[:, s] = np.maximum(a, -1)
    damage = {(96 + s % 5, s): "overlong" for s in range(1, S, 2)}
    m = M.run(rows, arrive, 0b01, mp, max_packet_inputs=W, seed=2, damage=damage,
              stride=M.max_packet_bytes(1, W + 1), overlap=False)
    assert m["applied"] == damage
    burst = m["ack"][70:75] - m["ack"][69:74]
    assert burst.max() >= 40 and (m["status"] == M.CODEC_E_CAP).sum() == len(damage)
    A, B = engines(S, P, (0,), mp, calls, W=W, stride=m["stride"])
    assert run_pair(A, B, rows, m, None, (64, 66), 0b01) == calls
    status, ack = A.packet_results(0, calls)
    assert (status == m["status"]).all() and (ack == m["ack"]).all()
    assert_same(A, B)
    check_sessions(A, rows, m["arrive"], np.zeros((calls, S), np.uint8), range(0, S, 3), calls)
    frames, skipped, errors = A.sessions()
    assert (errors == 0).all() and (skipped > 20).all()


def test_misuse_raises(oracle):
    from ggrs_amd import InvalidRequest, P2PEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    S, P, W = 8, 2, 16
    stride = M.max_packet_bytes(1, W)
    none = (np.full((1, S), -1, np.int32), np.zeros((1, S), np.int32), np.zeros((1, S, stride), np.uint8))

    def fresh(schedule=True):
        e = P2PEngine(S, num_players=P, local_players=(0,), max_prediction=8, remote_latency=1, input_capacity=32)
        if schedule:
            e.set_arrival_schedule(True)
        return e

    e = fresh(schedule=False)
    with pytest.raises(GgrsError) as err:  # without arrival schedules
        e.set_packet_feed(W, stride)
    assert err.value.code == GGRS_E_STATE
    e = fresh()
    e.add_inputs(0, np.zeros((4, S, P), np.uint8))
    with pytest.raises(GgrsError) as err:  # receive_packets without the mode
        e.receive_packets(0, *none)
    assert err.value.code == GGRS_E_STATE
    for bad_w, bad_stride in ((W, stride - 4), (W, stride + 2), (0, stride), (129, 4096), (W, 2048)):
        with pytest.raises(InvalidRequest):
            e.set_packet_feed(bad_w, bad_stride)
    e.set_packet_feed(W, stride)
    with pytest.raises(GgrsError) as err:  # add_arrivals in the mode
        e.add_arrivals(0, np.full((1, S), -1, np.int32))
    assert err.value.code == GGRS_E_STATE
    with pytest.raises(InvalidRequest):  # out of order
        e.receive_packets(1, *none)
    e.receive_packets(0, *none)
    with pytest.raises(InvalidRequest):
        e.receive_packets(0, *none)
    with pytest.raises(InvalidRequest):  # call 4's row is not added
        e.receive_packets(1, *(np.repeat(a, 4, axis=0) for a in none))
    with pytest.raises(InvalidRequest):
        e.packet_results(0, 2)
    e.advance_frames(1)
    with pytest.raises(GgrsError) as err:  # after the first call
        e.set_packet_feed(W, stride)
    assert err.value.code == GGRS_E_STATE
    status, ack = e.packet_results(0, 1)
    assert (status == 0).all() and (ack == -1).all()
    e = fresh()
    e.add_inputs(0, np.zeros((4, S, P), np.uint8))
    e.add_arrivals(0, np.full((1, S), -1, np.int32))
    with pytest.raises(GgrsError):  # after the first arrivals
        e.set_packet_feed(W, stride)


def test_desync_reports_in_packet_mode(oracle):
    """Desync detection's per-call reports (ggrs_p2p_read_reports) of a packet-fed engine equal the
    schedule-fed engine's."""
    S, calls, P, mp, interval = 96, 160, 2, 8, 10
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 0xDE5), calls, P, 1) for s in range(S)], axis=1)
    arrive, events = schedules(S, calls, mp, 17, 0b01, P, disconnect_every=0)
    m = M.run(rows, arrive, 0b01, mp, seed=1)
    A, B = engines(S, P, (0,), mp, calls, desync=interval)
    assert run_pair(A, B, rows, m, None, (37, 64, 59), 0b01) == calls
    assert_same(A, B)
    ra, rb = A.reports(0, calls), B.reports(0, calls)
    for key in ra:
        assert (ra[key] == rb[key]).all(), key
    assert (ra["frame"] >= 0).sum() > S


def test_peer_reports_in_packet_mode(oracle):
    """ggrs_p2p_add_peer_reports after receive_packets, chunk by chunk: the peers' disconnect reports
    act on a packet-fed engine as on the schedule-fed one (and as the oracle's, the panics included)."""
    from ggrs_amd._lib import GGRS_E_PRECONDITION
    S, calls, P, local, mp = 96, 160, 4, (0,), 8
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 91), calls, P, 1) for s in range(S)], axis=1)
    arrive, events, reports = peer_report_schedules(S, calls, mp, 29, P, 0b0001)
    m = M.run(rows, arrive, 0b0001, mp, seed=6)
    assert (m["arrive"] == arrive).all()
    A, B = engines(S, P, local, mp, calls)
    assert run_pair(A, B, rows, m, events, (37, 64, 59), 0b0001, reports=reports) == calls
    assert_same(A, B)
    check_sessions(A, rows, arrive, events, range(0, S, 3), calls, reports=reports)
    frames, skipped, errors = A.sessions()
    assert (errors == GGRS_E_PRECONDITION).sum() > 0 and (errors == 0).sum() > S // 2
