"""tests/event_queue_model.py against sequences derived by hand from the reference
(src/sessions/p2p_session.rs:430-469, :804-817, :846-937; src/network/protocol.rs:329-376, :534-574;
src/sessions/p2p_spectator_session.rs:199-239), and the proof that every GPU case of
tests/test_gpu_event_queue.py and tests/test_gpu_spectator_event_queue.py keeps at least one session in
every state it claims to test.  CPU only."""
import numpy as np
import pytest

from tests import event_queue_cases as C
from tests import event_queue_model as M


def kinds(q):
    return [r[0] for r in q.q]


def test_101_endpoint_events_leave_the_newest_100():
    q = M.SessionQueue(128)
    for c in range(101):
        q.p2p_call(c, net=M.NET_INTERRUPTED if c % 2 == 0 else M.NET_RESUMED, interrupted_ms=1500)
    assert len(q.q) == 100 and q.dropped == 0
    assert [r[2] for r in q.q] == list(range(1, 101))
    assert q.q[0] == (M.NETWORK_RESUMED, 0, 1, 0) and q.q[-1] == (M.NETWORK_INTERRUPTED, 0, 100, 1500)


def full_queue():
    q = M.SessionQueue(128)
    for c in range(100):
        q.p2p_call(c, net=M.NET_RESUMED)
    assert len(q.q) == 100
    return q


def test_desync_and_wait_overshoot_until_the_next_handled_event():
    """compare_local_checksums_against_peers and check_wait_recommendation push without the trim of
    handle_event: 104, still 104 after a call without an endpoint event, 100 after a handled Input."""
    q = full_queue()
    q.p2p_call(100, desync=[(30, 1, 2), (10, 3, 4), (20, 5, 6)], skip=3)
    assert len(q.q) == 104
    assert list(q.q)[-4:] == [(M.DESYNC_DETECTED, 0, 100, M.desync_payload(10, 3, 4)),
                              (M.DESYNC_DETECTED, 0, 100, M.desync_payload(20, 5, 6)),
                              (M.DESYNC_DETECTED, 0, 100, M.desync_payload(30, 1, 2)),
                              (M.WAIT_RECOMMENDATION, 0, 100, 3)]
    q.p2p_call(101)
    assert len(q.q) == 104
    q.p2p_call(102, skip=0, events=1, rmask=2)  # (a local player's bit, a non-positive skip: nothing)
    assert len(q.q) == 104 and q.closed_call == -1
    q.p2p_call(103, handled=1)
    assert len(q.q) == 100 and q.q[0][2] == 4 and q.q[-1][0] == M.WAIT_RECOMMENDATION and q.dropped == 0


def test_the_order_inside_one_call():
    q = M.SessionQueue(128)
    q.p2p_call(3, events=2, disc_req=1, handled=1, net=15, spec_net=(M.NET_DISCONNECTED | M.NET_RESUMED, M.NET_INTERRUPTED),
               skip=5, desync=[(9, 1, 2), (2, 3, 4)], rmask=2, interrupted_ms=1500, spec_interrupted_ms=2000)
    assert list(q.q) == [(M.NETWORK_RESUMED, 0, 3, 0), (M.DISCONNECTED, 0, 3, 0), (M.NETWORK_INTERRUPTED, 0, 3, 1500),
                         (M.NETWORK_RESUMED, 1, 3, 0), (M.DISCONNECTED, 1, 3, 0), (M.NETWORK_INTERRUPTED, 2, 3, 2000),
                         (M.DESYNC_DETECTED, 0, 3, M.desync_payload(2, 3, 4)), (M.DESYNC_DETECTED, 0, 3, M.desync_payload(9, 1, 2)),
                         (M.WAIT_RECOMMENDATION, 0, 3, 5)]
    assert q.closed_call == 3


def test_disc_req_after_the_hosts_own_disconnect_raises_nothing():
    """disconnect_player closes the endpoint without an event (p2p_session.rs:485-511,
    protocol.rs:311-319); on_input's check `state != Disconnected` (:571) then fails."""
    q = M.SessionQueue(128)
    q.p2p_call(2, events=2, rmask=2)
    assert not q.q and q.closed_call == 2
    q.p2p_call(6, disc_req=1, events=2, rmask=2)
    q.p2p_call(9, net=M.NET_DISCONNECTED)
    assert not q.q and q.closed_call == 2


def test_a_timeout_after_disc_req_raises_nothing():
    """on_input sets disconnect_event_sent (:573), which poll's timeout checks (:361)."""
    q = M.SessionQueue(128)
    q.p2p_call(2, disc_req=1, events=2, rmask=2)
    q.p2p_call(8, net=M.NET_DISCONNECTED)
    q.p2p_call(9, disc_req=1)
    assert list(q.q) == [(M.DISCONNECTED, 0, 2, 0)] and q.closed_call == 2
    # ... and in one call, the request's event is the one
    q = M.SessionQueue(128)
    q.p2p_call(4, disc_req=1, net=M.NET_DISCONNECTED)
    assert list(q.q) == [(M.DISCONNECTED, 0, 4, 0)]


def test_shutdown_is_no_event_and_spectators_have_no_closed_flag():
    q = M.SessionQueue(128)
    q.p2p_call(0, net=M.NET_SHUTDOWN, spec_net=(M.NET_SHUTDOWN,))
    assert not q.q
    q.p2p_call(1, spec_net=(M.NET_DISCONNECTED,))
    q.p2p_call(2, spec_net=(M.NET_DISCONNECTED,))
    assert kinds(q) == [M.DISCONNECTED] * 2 and q.closed_call == -1


def test_a_full_ring_drops_the_oldest_and_counts_it():
    q = full_queue()
    for c in range(100, 104):
        q.p2p_call(c, desync=[(7 * f, f, c) for f in range(10)])
    assert len(q.q) == 128 and q.dropped == 12
    assert q.q[0][2] == 12 and q.q[-1] == (M.DESYNC_DETECTED, 0, 103, M.desync_payload(63, 9, 103))
    q.p2p_call(104, net=M.NET_RESUMED)  # the push drops one more, then the trim cuts to 100
    assert len(q.q) == 100 and q.dropped == 13 and q.q[-1][0] == M.NETWORK_RESUMED


def test_a_spectator_session_never_exceeds_100():
    case = C.spectator_case()
    m = M.EventQueueModel(case["S"], 128, interrupted_ms=1500, spectator=True)
    seen = np.zeros(case["S"], np.int64)
    for c in range(case["calls"]):
        m.collect(c, 1, handled=case["handled"][c:c + 1], net=case["net"][c:c + 1])
        seen = np.maximum(seen, m.lengths())
    assert seen.max() == 100 and (np.array([q.dropped for q in m.sessions]) == 0).all()
    # the one Disconnected, whatever follows
    for q in m.sessions:
        assert kinds(q).count(M.DISCONNECTED) <= 1
    assert any(q.closed_call >= 0 for q in m.sessions) and any(q.closed_call < 0 for q in m.sessions)
    busy = [q for q in m.sessions if len(q.q) == 100]
    assert busy and all(q.q[0][2] > 0 for q in busy)  # (cut: the first calls' events are gone)


def test_hand_sequences_through_the_batch_interface():
    """tests/event_queue_cases.py's hand_sequences, the GPU test's input, gives the states above."""
    case = C.hand_sequences()
    m = C.run_model(case)
    length, dropped, status, closed = C.words(m)
    assert length[:3].tolist() == [100, 100, 128] and dropped.tolist() == [0, 0, 12, 0, 0, 0, 0]
    assert status.tolist() == [0, 0, 0, M.EVENTS_LOST, 0, 0, 0] and m.over_stage == {3}
    assert closed.tolist() == [-1, -1, -1, -1, 3, 2, 2]
    assert len(m.sessions[4].q) == 9 and not m.sessions[5].q and kinds(m.sessions[6]) == [M.DISCONNECTED]
    # session 1 in calls: 104 after call 100 and after call 101, 100 after call 102
    by_call = M.EventQueueModel(case["S"], 128, 2, C.RMASK)
    seen = []
    for c in range(104):
        by_call.collect(c, 1, case["events"][c:c + 1], case["disc_req"][c:c + 1], case["handled"][c:c + 1],
                        case["net"][c:c + 1], case["spec_net"][c:c + 1], case["skip"][c:c + 1], C.desync_of(case, c, 1))
        seen.append(by_call.lengths()[1])
    assert seen[99:103] == [100, 104, 104, 100]


@pytest.mark.parametrize("K", [0, 1, 4])
def test_the_general_case_reaches_its_edges_and_does_not_depend_on_the_split(K):
    case = C.general(K)
    m = C.run_model(case)
    C.general_reaches_its_edges(case, m)
    if K:
        assert any(r[1] == K for q in m.sessions for r in q.q)  # the last spectator endpoint's events
    split = C.run_model(case, C.PIECES)
    assert C.words(split)[0].tolist() == C.words(m)[0].tolist()
    assert (C.queue_array(split) == C.queue_array(m)).all()
    # shuffled records against the same records in order
    ordered = dict(case, desync=C.in_order(case["desync"]))
    assert (C.queue_array(C.run_model(ordered)) == C.queue_array(m)).all()
    assert not (ordered["desync"][0] == case["desync"][0]).all()


def test_the_drain_cases_cut_where_they_claim():
    case = C.general(0)
    m = C.run_model(case)
    length = np.array(m.lengths())
    ends = np.cumsum(length)
    b = int(np.flatnonzero(length > 0)[3])  # a session boundary inside the list
    for max_records, want in ((int(ends[b]) - 1, int(ends[b - 1])), (int(ends[b]) + 1, int(ends[b])), (0, 0),
                              (int(ends[-1]), int(ends[-1]))):
        mm = C.run_model(case)
        got, left = mm.drain(max_records)
        assert len(got) == want and left == int(ends[-1]) - want, (max_records, want)
        assert [r[0] for r in got] == sorted(r[0] for r in got)
        assert all(not q.q for q in mm.sessions[:b]) or max_records == 0
    # a drain between two collections
    mm, (got, left) = C.run_model(case, (64, 96), drain_at=64, max_records=int(ends[-1]))
    assert got and left == 0 and sum(mm.lengths()) > 0
    # the sparse case: one busy session in 37
    sp = C.sparse(4099)
    ms = C.run_model(sp)
    assert sum(1 for n in ms.lengths() if n) == 111 and set(ms.lengths()) == {0, 7}
    got, left = ms.drain(10 ** 6)
    assert len(got) == 777 and left == 0 and {r[0] % 37 for r in got} == {0}
