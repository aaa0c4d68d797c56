"""GPU parity of the P2P engine's event queue (ggrs_p2p_set_event_queue / collect_events / drain_events /
read_event_queue_state, csrc/p2p_events.hip and events_device.h) against tests/event_queue_model.py, per
session and per record.  The unit is a function of its rows, so the rows are synthesized
(tests/event_queue_cases.py, whose cases tests/test_event_queue_model.py proves non-vacuous); only the
engine-list case and the last test run other units."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import event_queue_cases as C  # noqa: E402
from tests import event_queue_model as M  # noqa: E402

pytestmark = pytest.mark.gpu


def engine(S_=C.S, K=0, capacity=C.CAPACITY, queue=True):
    """The polls give the NetworkInterrupted payloads: 2000 - 500 and 3000 - 1000 ms."""
    from ggrs_amd import P2PEngine
    e = P2PEngine(S_, num_players=2, local_players=(0,), input_delay=0, max_prediction=8, remote_latency=1,
                  input_capacity=64)
    e.set_arrival_schedule(True)
    e.set_endpoint_poll(2000, 500, 0)
    if K:
        e.set_spectator_emit(K, 64)
        e.set_spectator_poll(3000, 1000, 0)
    if queue:
        e.set_event_queue(capacity)
    return e


def dev(a):
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def collect(eng, case, c0, n, device=False, desync="own"):
    sl = slice(c0, c0 + n)
    rows = [case["events"][sl], case["disc_req"][sl], case["handled"][sl], case["net"][sl],
            case["spec_net"][sl] if case["K"] else None, case["skip"][sl]]
    ds = C.desync_of(case, c0, n) if desync == "own" else desync
    if device:
        rows = [None if r is None else dev(r) for r in rows]
        ds = tuple(dev(a) for a in ds)
    eng.collect_events(c0, n, *rows, desync=ds, on_device=device)
    if device:
        eng.synchronize()  # (the tensors go out of scope)


def drive(eng, case, pieces=None, device=False):
    for i, (c0, n) in enumerate(C.pieces_of(pieces or (case["calls"],), case["calls"])):
        collect(eng, case, c0, n, device is True or (device == "both" and i % 2 == 0))


def assert_matches(eng, m, capacity=C.CAPACITY):
    """Lengths, drop counters, status, closing calls and every record of every queue; a session over
    the staging bound is compared by its status alone (which records it kept is unspecified)."""
    got = eng.event_queue_state()
    ok = np.array([s not in m.over_stage for s in range(m.S)])
    for name, g, w in zip(("length", "dropped", "status", "closed_call"), got, C.words(m)):
        keep = ok | (name in ("status", "closed_call"))
        assert (g[keep] == w[keep]).all(), (name, np.argwhere(g != w)[:5], g[g != w][:5], w[g != w][:5])
    want = C.queue_array(m, capacity)
    for f in C.RECORD.names:
        bad = (got[4][f] != want[f]) & ok[None, :]
        assert not bad.any(), (f, np.argwhere(bad)[:5], got[4][f][bad][:5], want[f][bad][:5])


# ---- 1. parity, whatever the split

@pytest.mark.parametrize("K", [0, 1, 4])
def test_queues_match_the_model_whatever_the_split(K):
    """S = 130 (two full waves and a two-lane tail), 160 calls in invocations of 1, 7, 64 and 88 calls
    (host arrays and device tensors alternating) and again in one invocation."""
    case = C.general(K)
    m = C.run_model(case)
    C.general_reaches_its_edges(case, m)
    split, whole = engine(K=K), engine(K=K)
    drive(split, case, C.PIECES, "both")
    drive(whole, case)
    assert_matches(split, m)
    assert_matches(whole, m)


def test_trim_overshoot_ring_overflow_and_the_staging_bound():
    """The hand-derived sequences at the smallest capacity: 101 events leave 100; 104 until a handled
    Input; 140 pushes into a ring of 128; 65 desync records in one invocation."""
    from ggrs_amd._lib import GGRS_EVENTS_LOST
    case = C.hand_sequences()
    m = C.run_model(case)
    assert m.over_stage == {3} and m.lengths()[:3] == [100, 100, 128]
    eng = engine(case["S"], K=case["K"])
    seen = []
    for c0, n in C.pieces_of((100, 1, 1, 1, 7), case["calls"]):
        collect(eng, case, c0, n)
        seen.append(int(eng.event_queue_state(queue=False)[0][1]))
    assert seen[:4] == [100, 104, 104, 100]
    assert_matches(eng, m)
    length, dropped, status, closed = eng.event_queue_state(queue=False)
    assert status[3] == GGRS_EVENTS_LOST == M.EVENTS_LOST and length[3] == M.STAGE_D and dropped[2] == 12
    # the session over the bound took 64 of its own records, in frame order
    q = eng.event_queue_state()[4][:, 3]
    assert (q["kind"][:64] == M.DESYNC_DETECTED).all() and (q["call"][:64] == 5).all()
    frames = (q["payload"][:64] & 0xffffffff).astype(np.int64)
    assert (np.diff(frames) > 0).all() and frames.max() < 65


@pytest.mark.parametrize("device", [False, True])
def test_shuffled_desync_records_against_the_same_in_order(device):
    case = C.general(1)
    ordered = dict(case, desync=C.in_order(case["desync"]))
    assert not (ordered["desync"][2] == case["desync"][2]).all()
    a, b = engine(K=1), engine(K=1)
    drive(a, case, (64, 96), device)
    drive(b, ordered, (64, 96), device)
    m = C.run_model(case)
    assert_matches(a, m)
    assert_matches(b, m)


# ---- 2. the engine's own list

def test_the_engines_own_desync_list(oracle):
    """Two coupled engines with one corrupted peer per three matches
    (tests/test_gpu_desync_compare.py's smallest shape): n_desync == -1 gives what the arrays
    ggrs_p2p_read_desync_events returns give, and GGRS_E_STATE while the comparison lags."""
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    from tests.test_desync_compare_model import CALLS, CASES, S, matches, oracle_events
    from tests.test_gpu_desync_compare import engine as pair_engine, hand_over
    interval, mp = CASES[0]
    rows, arr, refs = matches(interval, mp)
    engs = [pair_engine(k, mp, interval, 4096) for k in (0, 1)]
    for k, e in enumerate(engs):
        e.set_event_queue(C.CAPACITY)
        e.add_inputs(0, rows[k])
        e.add_arrivals(0, arr[k])
    chunks, done = (17, 64, 79), 0
    for i, n in enumerate(chunks):
        for e in engs:
            e.advance_frames(n)
        for k in (0, 1):
            hand_over(engs[k], engs[1 - k], done, n, "from")
        if i == 1:
            with pytest.raises(GgrsError) as err:  # the comparison has not run through these calls
                engs[0].collect_events(done, n, desync="engine")
            assert err.value.code == GGRS_E_STATE and str(done) in str(err.value)
        for e in engs:
            e.compare_reports(done, n, wait=False)
        if i == 0:
            engs[0].collect_events(done, n, desync="engine")
        elif i == 1:
            # two invocations over one comparison: the list is scanned for each one's calls
            engs[0].collect_events(done, 30, desync="engine")
            engs[0].collect_events(done + 30, n - 30, desync="engine")
        done += n
    engs[0].collect_events(chunks[0] + chunks[1], chunks[2], desync="engine")
    engs[1].collect_events(0, CALLS, desync="engine")
    for k, e in enumerate(engs):
        want = oracle_events(refs, k)
        assert len(want) > 0
        listed = e.desync_events()
        assert sorted(zip(*(a.tolist() for a in listed))) == want
        m = M.EventQueueModel(S, C.CAPACITY)
        m.collect(0, CALLS, desync=listed)
        assert not m.over_stage and sum(m.lengths()) == len(want)
        assert_matches(e, m)
        # ... and a bare engine given the arrays
        bare = engine(S)
        bare.collect_events(0, CALLS, desync=listed)
        for g, w in zip(bare.event_queue_state(), e.event_queue_state()):
            assert (g == w).all()


# ---- 3. the drain

def assert_drained(got, want_records):
    want = C.drained_array(want_records)
    assert got.dtype == want.dtype and len(got) == len(want)
    for f in want.dtype.names:
        assert (got[f] == want[f]).all(), (f, np.argwhere(got[f] != want[f])[:5])


def test_drain_all_of_it_at_session_boundaries_and_nothing():
    case = C.general(0)
    ends = np.cumsum(C.run_model(case).lengths())
    b = int(np.flatnonzero(np.diff(np.concatenate([[0], ends])) > 0)[3])
    for max_records in (int(ends[-1]), int(ends[b]) - 1, int(ends[b]) + 1, 0, None):
        eng, m = engine(), C.run_model(case)
        drive(eng, case)
        got, left = eng.drain_events(max_records)
        want, want_left = m.drain(C.S * C.CAPACITY if max_records is None else max_records)
        assert left == want_left
        assert_drained(got, want)
        assert_matches(eng, m)  # what stayed, and the drained queues empty
        # the rest, into device tensors
        d_s = torch.full((max(left, 1),), -1, dtype=torch.int32, device="cuda")
        d_r = torch.zeros((max(left, 1), 16), dtype=torch.uint8, device="cuda")
        n_read, n_left = eng.drain_events(max(left, 1), out=(d_s, d_r))
        want, _ = m.drain(left)
        assert (n_read, n_left) == (left, 0) and len(want) == left
        eng.synchronize()
        rest = np.zeros(left, got.dtype)
        rest["session"] = d_s.cpu().numpy()[:left]
        recs = d_r.cpu().numpy()[:left].copy().view(C.RECORD).reshape(-1)
        for f in C.RECORD.names:
            rest[f] = recs[f]
        assert_drained(rest, want)
        assert (eng.event_queue_state(queue=False)[0] == 0).all()


def test_drain_an_empty_engine_and_between_two_collections():
    case = C.general(4)
    eng = engine(K=4)
    got, left = eng.drain_events()
    assert len(got) == 0 and left == 0
    m, (want, want_left) = C.run_model(case, (64, 96), drain_at=64, max_records=700)
    assert want and want_left > 0  # (some sessions handed over, some kept)
    collect(eng, case, 0, 64)
    got, left = eng.drain_events(700)
    assert left == want_left
    assert_drained(got, want)
    collect(eng, case, 64, 96)
    assert_matches(eng, m)  # the rings go on from where the drain left them


@pytest.mark.parametrize("S_", [4099, 1])
def test_the_scan_across_its_block_level(S_):
    """S = 4099: 17 blocks of the scan, a two-level scan with one busy session in 37; S = 1."""
    case = C.sparse(S_)
    m = C.run_model(case)
    eng = engine(S_)
    drive(eng, case)
    assert_matches(eng, m)
    got, left = eng.drain_events(777)
    want, want_left = m.drain(777)
    assert left == want_left == 0 and len(want) == (777 if S_ == 4099 else 7)
    assert_drained(got, want)
    assert (eng.event_queue_state(queue=False)[0] == 0).all()


# ---- 4. misuse

def test_misuse():
    from ggrs_amd import P2PEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError, InvalidRequest
    case = C.general(0)

    def state_error(fn):
        with pytest.raises(GgrsError) as e:
            fn()
        assert e.value.code == GGRS_E_STATE, e.value

    plain = engine(queue=False)
    state_error(lambda: plain.collect_events(0, 1))                    # unconfigured
    state_error(plain.drain_events)
    state_error(plain.event_queue_state)
    for capacity in (127, 1025):
        with pytest.raises(InvalidRequest):
            plain.set_event_queue(capacity)
    plain.add_inputs(0, np.zeros((2, C.S, 2), np.uint8))
    plain.add_arrivals(0, np.zeros((2, C.S), np.int32))
    plain.poll_endpoints(0, 1, np.zeros(1, np.uint64))
    plain.advance_frames(1)
    state_error(lambda: plain.set_event_queue(128))                    # after the first call
    fixed = P2PEngine(C.S, num_players=2, local_players=(0,), max_prediction=8, remote_latency=2, input_capacity=64)
    state_error(lambda: fixed.set_event_queue(128))                    # a fixed-latency engine
    eng = engine()
    for capacity in (128, 1024):
        eng.set_event_queue(capacity)
    eng.set_event_queue(C.CAPACITY)
    with pytest.raises(InvalidRequest):
        collect(eng, case, 1, 1)                                       # out of order
    collect(eng, case, 0, 2)
    with pytest.raises(InvalidRequest):
        collect(eng, case, 1, 1)                                       # repeated
    with pytest.raises(InvalidRequest):
        collect(eng, case, 0, 2)
    with pytest.raises(InvalidRequest):
        eng.collect_events(2, -1)
    state_error(lambda: eng.collect_events(2, 1, desync="engine"))     # no comparison configured
    eng.collect_events(2, 0)                                           # nothing to do
    collect(eng, case, 2, 158)
    # nothing above changed the queues: the 160 calls that ran are the model's
    assert_matches(eng, C.run_model(case))


# ---- 5. an engine without the unit is unchanged

def test_an_engine_without_the_unit_is_unchanged(oracle):
    """The same scheduled calls with polls and time sync on two engines, one of which also collects and
    drains: states, rings, the other units' outputs and state are equal, and the queues are the model's
    over the rows the other units wrote."""
    from tests import endpoint_poll_model as P
    from tests.test_gpu_endpoint_poll import CALLS, S, engine as poll_engine
    from tests.test_gpu_p2p_packets import assert_same
    from tests.test_gpu_p2p_sched import schedules
    now, kinds, _ = P.gpu_case(P.CLOCKS[0])
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 0xE9E), CALLS, 2, 0) for s in range(S)], axis=1)
    arrive, events = schedules(S, CALLS, 8, 33, 0b01, 2)
    A, B = poll_engine(time_sync=True), poll_engine(time_sync=True)
    A.set_event_queue(C.CAPACITY)
    m = M.EventQueueModel(S, C.CAPACITY, rmask=P.CASE_RMASK, interrupted_ms=P.CASE_TIMEOUT - P.CASE_NOTIFY)
    outs = {id(A): [], id(B): []}
    for c0, n in C.pieces_of((13, 8), CALLS):
        sl = slice(c0, c0 + n)
        for e in (A, B):
            e.add_arrivals(c0, arrive[sl], events[sl])
            polled = e.poll_endpoints(c0, n, now[sl], kinds[sl])
            e.add_inputs(c0, rows[sl])
            e.advance_frames(n)
            synced = e.time_sync(c0, n)
            outs[id(e)].append(polled + synced)
        polled, synced = outs[id(A)][-1][:4], outs[id(A)][-1][4:]
        A.collect_events(c0, n, events=events[sl], net_events=polled[3], skip_frames=synced[2])
        m.collect(c0, n, events=events[sl], net=polled[3], skip=synced[2])
        if c0 > 60:
            A.drain_events(500)
            m.drain(500)
    assert sum(len(q.q) for q in m.sessions) > 0 or any(q.closed_call >= 0 for q in m.sessions)
    assert_matches(A, m)
    assert_same(A, B)
    for a, b in zip(outs[id(A)], outs[id(B)]):
        for x, y in zip(a, b):
            assert (x == y).all()
    for fa, fb in ((A.time_sync_state, B.time_sync_state), (A.endpoint_state, B.endpoint_state)):
        for x, y in zip(fa(), fb()):
            assert (x == y).all()
