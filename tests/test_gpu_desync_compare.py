"""GPU parity of the device's checksum comparison (ggrs_p2p_set_desync_compare / add_remote_reports /
add_remote_reports_from / compare_reports / read_desync_events / read_desync_state,
csrc/p2p_desync.hip) against the oracle's two-peer run (oracle_p2p_sched_desync_pair_run) and
tests/desync_compare_model.py: both machines of every match as two coupled P2P engines whose report
rows cross in device memory or through the host, every DesyncDetected event, the per-session summary
and both 32-entry tables; launch splits, the three row sources, the packet feed, a full event list, a
lost row, refused reports, lockstep mode, misuse -- and an engine that does not configure the
comparison against one that does."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import desync_compare_model as M  # noqa: E402
from tests import packet_feed_model as F  # noqa: E402
from tests.test_desync_compare_model import (CALLS, CASES, S, cut, lost_row_case, matches, model_run,  # noqa: E402
                                             oracle_events, refused_case)

pytestmark = pytest.mark.gpu

CHUNKS = {(7, 8): (17, 64, 79), (1, 6): (80, 80), (25, 9): (160,)}


def engine(k, mp, interval, max_events=None, feed=False, cap=CALLS, S_=S):
    from ggrs_amd import P2PEngine
    e = P2PEngine(S_, num_players=2, local_players=(k,), max_prediction=mp, remote_latency=1, input_capacity=cap)
    e.set_arrival_schedule(True)
    if feed:
        e.set_packet_feed(64)
    if interval:
        e.set_desync_detection(interval)
    if max_events:
        e.set_desync_compare(max_events)
    return e


def hand_over(dst, src, first, n, source):
    """The rows of src's calls first .. first + n - 1 into dst, by one of the three ways."""
    if source == "from":
        dst.add_remote_reports_from(src, first, n)
        return
    r = src.reports(first, n)
    args = [r["frame"], r["checksum"], r["local_last"]]
    if source == "device":
        d = torch.device("cuda")
        args = [torch.from_numpy(args[0]).to(d), torch.from_numpy(args[1].view(np.int16)).to(d),
                torch.from_numpy(args[2]).to(d)]
    dst.add_remote_reports(first, *args)
    if source == "device":
        dst.synchronize()  # (the tensors go out of scope: the copy on the engine's stream has read them)


def run_pair(interval, mp, chunks, max_events, source="from", feed=False):
    """Two coupled engines over the oracle pair's rows; returns them after the last chunk."""
    rows, arr, refs = matches(interval, mp)
    engs = [engine(k, mp, interval, max_events[k], feed) for k in (0, 1)]
    pk = []
    for k, e in enumerate(engs):
        e.add_inputs(0, rows[k])
        if feed:
            pk.append(F.run(rows[k], arr[k], 1 << k, mp, seed=k))
            assert (pk[k]["arrive"] == arr[k]).all()
        else:
            e.add_arrivals(0, arr[k])
    done = 0
    for n in chunks:
        for k, e in enumerate(engs):
            if feed:
                e.receive_packets(done, pk[k]["start"][done:done + n], pk[k]["length"][done:done + n],
                                  pk[k]["packets"][done:done + n])
            e.advance_frames(n)
        for k in (0, 1):
            hand_over(engs[k], engs[1 - k], done, n, source)
        for e in engs:
            e.compare_reports(done, n, wait=False)
        done += n
    assert done == CALLS
    return engs


def events_of(e):
    return sorted(zip(*(a.tolist() for a in e.desync_events())))


def assert_state(e, m, what=range(9)):
    got, want = e.desync_state(), m.state()
    for i in what:
        assert (got[i] == want[i]).all(), (i, np.argwhere(got[i] != want[i])[:5])


def assert_pair(engs, interval, mp):
    rows, arr, refs = matches(interval, mp)
    for k, e in enumerate(engs):
        want = oracle_events(refs, k)
        assert e.compare_reports(CALLS, 0) == len(want)
        assert events_of(e) == want
        m, _ = model_run(interval, mp, k)
        assert_state(e, m)
        for g, w in zip(e.desync_state()[1:6], M.summary_of(want, S)):
            assert (g == w).all()
        assert (e.sessions()[2] == 0).all()


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("interval,mp", CASES)
def test_coupled_engines_match_the_oracle(oracle, monkeypatch, interval, mp, lds):
    """GGRS_DESYNC_COMPARE_LDS: a block's tables in LDS for the launch, or touched in HBM."""
    monkeypatch.setenv("GGRS_DESYNC_COMPARE_LDS", lds)
    rows, arr, refs = matches(interval, mp)
    sizes = [len(oracle_events(refs, k)) for k in (0, 1)]
    assert min(sizes) > 0
    assert_pair(run_pair(interval, mp, CHUNKS[(interval, mp)], sizes), interval, mp)


def test_launch_splits(oracle):
    """160 one-call launches and one 160-call launch: the same events and state."""
    interval, mp = CASES[0]
    a = run_pair(interval, mp, (1,) * CALLS, (4096, 4096))
    b = run_pair(interval, mp, (CALLS,), (4096, 4096))
    assert_pair(a, interval, mp)
    assert_pair(b, interval, mp)


@pytest.mark.parametrize("source", ["host", "device"])
def test_row_sources(oracle, source):
    """Peer rows from host arrays and from device tensors: what add_remote_reports_from gives (the
    parity test's source)."""
    interval, mp = CASES[0]
    assert_pair(run_pair(interval, mp, CHUNKS[CASES[0]], (4096, 4096), source=source), interval, mp)


def test_packet_feed_last_recv_is_the_feeds_ack_row(oracle):
    interval, mp = CASES[0]
    engs = run_pair(interval, mp, CHUNKS[CASES[0]], (4096, 4096), feed=True)
    assert_pair(engs, interval, mp)
    rows, arr, refs = matches(interval, mp)
    for k, e in enumerate(engs):
        assert (e.packet_results(0, CALLS)[1] == arr[k]).all()


def test_full_event_list(oracle):
    """max_events 16 where 64 are raised: the count is exact, 16 distinct records of the oracle's
    are kept, the summaries are exact."""
    interval, mp = CASES[2]
    rows, arr, refs = matches(interval, mp)
    engs = run_pair(interval, mp, (80, 80), (16, 16))
    for k, e in enumerate(engs):
        want = oracle_events(refs, k)
        assert len(want) == 64 and e.compare_reports(CALLS, 0) == 64
        got = events_of(e)
        assert len(got) == 16 and len(set(got)) == 16 and set(got) <= set(want)
        assert len(e.desync_events(10, 100)[0]) == 6 and len(e.desync_events(16, 4)[0]) == 0
        m, _ = model_run(interval, mp, k)
        assert_state(e, m)


def test_lost_row(oracle):
    """input_capacity 24, every third session's arrivals stalled from call 10 on (for good: its input
    rows are never needed again, so the session itself goes on) while the peer's rows keep coming:
    GGRS_DESYNC_ROW_LOST for those sessions after the launch the model names, nothing raised by them
    afterwards; every other session goes on as the model does.  A status word: no access leaves the
    ring."""
    from ggrs_amd._lib import GGRS_DESYNC_ROW_LOST
    _, peer, arrive, stalled, cap = lost_row_case(recover=False)
    calls, S_ = arrive.shape
    e = engine(0, 8, 2, S_ * calls, cap=cap, S_=S_)
    m = M.Engine(S_, 2, cap)
    seen = []
    for c0 in range(0, calls, 8):
        e.add_inputs(c0, np.zeros((8, S_, 2), np.uint8))
        e.add_arrivals(c0, arrive[c0:c0 + 8])
        e.advance_frames(8)
        e.add_remote_reports(c0, peer["frame"][c0:c0 + 8], peer["checksum"][c0:c0 + 8], peer["local_last"][c0:c0 + 8])
        m.add_remote_reports(c0, peer["frame"][c0:c0 + 8], peer["checksum"][c0:c0 + 8], peer["local_last"][c0:c0 + 8])
        total = e.compare_reports(c0, 8)
        m.compare_reports(c0, e.reports(c0, 8), arrive[c0:c0 + 8])
        assert total == len(m.events)
        status = e.desync_state()[0]
        assert (status == m.state()[0]).all(), c0
        seen.append(int((status == GGRS_DESYNC_ROW_LOST).sum()))
    assert GGRS_DESYNC_ROW_LOST == M.ROW_LOST and (m.lost_call[stalled] == 32).all()
    assert seen[3] == 0 and seen[4] == stalled.sum() == seen[-1]
    # (a stalled session itself stops once its own frame's row has left the 24 rows held: its report
    # rows say "no report" from there on, as ggrs_p2p_read_reports returns them)
    assert (e.sessions()[2][~stalled] == 0).all()
    assert events_of(e) == m.events and len(m.events) > S_
    assert all(c < 32 for c, s, f, l, r in m.events if stalled[s])
    assert any(c > 60 for c, s, f, l, r in m.events if not stalled[s])
    assert_state(e, m)


def test_refused_reports(oracle):
    """Frames that are no multiple of the interval, repeated, descending or 0 in the peer's rows."""
    S_ = 70
    _, peer, arrive = refused_case(S_)
    n = arrive.shape[0]
    arrive = np.repeat(np.arange(n, dtype=np.int32)[:, None] - 1, S_, axis=1)
    peer["local_last"][:] = -1  # (travels with nothing: delivered by the next call)
    e = engine(0, 8, 5, 4 * S_, cap=n, S_=S_)
    e.add_inputs(0, np.zeros((n, S_, 2), np.uint8))
    e.add_arrivals(0, arrive)
    e.advance_frames(n)
    m = M.Engine(S_, 5, n)
    for x in (e, m):
        x.add_remote_reports(0, peer["frame"], peer["checksum"], peer["local_last"])
    total = e.compare_reports(0, n)
    m.compare_reports(0, e.reports(0, n), arrive)
    assert total == len(m.events) and events_of(e) == m.events
    refused = m.state()[6]
    assert set(refused.tolist()) == {4, 5}
    assert_state(e, m)


def test_lockstep_sends_no_report(oracle):
    """max_prediction 0: no state is saved, so no report is sent and nothing is raised."""
    S_, n = 70, 40
    arrive = np.repeat(np.arange(n, dtype=np.int32)[:, None] - 1, S_, axis=1)
    engs = [engine(k, 0, 3, 64, cap=n, S_=S_) for k in (0, 1)]
    for e in engs:
        e.add_inputs(0, np.zeros((n, S_, 2), np.uint8))
        e.add_arrivals(0, arrive)
        e.advance_frames(n)
    for k, e in enumerate(engs):
        assert (e.reports(0, n)["frame"] == -1).all()
        e.add_remote_reports_from(engs[1 - k], 0, n)
        assert e.compare_reports(0, n) == 0
        st = e.desync_state()
        assert all((st[i] == 0).all() for i in (0, 1, 6)) and (st[7][0] == -1).all() and (st[8][0] == -1).all()
        assert len(e.desync_events()[0]) == 0


def test_misuse_raises(oracle):
    from ggrs_amd import InvalidRequest, P2PEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    S_, n = 8, 16

    def fresh(schedule=True, interval=4, compare=True):
        e = P2PEngine(S_, num_players=2, local_players=(0,), max_prediction=8, remote_latency=1, input_capacity=32)
        if schedule:
            e.set_arrival_schedule(True)
        if interval:
            e.set_desync_detection(interval)
        if compare:
            e.set_desync_compare(64)
        return e

    def state_error(f, *a, match=None):
        with pytest.raises(GgrsError, match=match) as err:
            f(*a)
        assert err.value.code == GGRS_E_STATE

    def feed(e, c0, k):
        e.add_inputs(c0, np.zeros((k, S_, 2), np.uint8))
        e.add_arrivals(c0, np.repeat(np.arange(c0, c0 + k, dtype=np.int32)[:, None] - 1, S_, axis=1))

    none = dict(frame=np.full((n, S_), -1, np.int32), checksum=np.zeros((n, S_), np.uint16),
                local_last=np.zeros((n, S_), np.int32))
    rows = (none["frame"], none["checksum"], none["local_last"])
    state_error(fresh(schedule=False, compare=False).set_desync_compare, 64)  # a fixed-latency engine
    state_error(fresh(schedule=False, compare=False).compare_reports, 0, 0)
    state_error(fresh(interval=0, compare=False).set_desync_compare, 64)  # without desync detection
    e = fresh(compare=False)
    feed(e, 0, n)
    state_error(e.compare_reports, 0, 1)  # before set_desync_compare
    state_error(e.add_remote_reports, 0, *rows)
    state_error(e.desync_state)
    state_error(e.desync_events)
    for bad in (0, -1, (1 << 26) + 1):
        with pytest.raises(InvalidRequest):
            e.set_desync_compare(bad)
    e.set_desync_compare(8)
    e.set_desync_compare(64)
    with pytest.raises(InvalidRequest):  # call 0 has not run
        e.compare_reports(0, 1)
    e.advance_frames(8)
    state_error(e.set_desync_compare, 64)  # configured after the first call
    assert e.compare_reports(0, 1) == 0  # call 0 needs none of the peer's rows
    state_error(e.compare_reports, 1, 2, match="call 0 ")  # calls 1..2 need the peer's rows 0..1
    with pytest.raises(InvalidRequest):  # the peer's rows in call order
        e.add_remote_reports(1, *(r[:1] for r in rows))
    with pytest.raises(InvalidRequest):  # more rows than the ring holds
        e.add_remote_reports(0, *(np.concatenate([r, r, r]) for r in rows))
    e.add_remote_reports(0, *(r[:3] for r in rows))
    state_error(e.compare_reports, 1, 5, match="call 3 ")  # calls 1..5 need rows 0..4
    with pytest.raises(InvalidRequest):  # out of order
        e.compare_reports(2, 1)
    with pytest.raises(InvalidRequest):  # not yet run
        e.compare_reports(1, 8)
    assert e.compare_reports(1, 3) == 0
    with pytest.raises(InvalidRequest):  # each call once
        e.compare_reports(3, 1)
    assert e.compare_reports(4, 0) == 0
    peer = fresh(compare=False)
    with pytest.raises(InvalidRequest):  # the peer has not run these calls
        e.add_remote_reports_from(peer, 3, 1)
    with pytest.raises(InvalidRequest):
        e.add_remote_reports_from(e, 3, 1)
    state_error(e.add_remote_reports_from, fresh(interval=0, compare=False), 3, 1)  # a peer without report rows
    feed(peer, 0, n)
    peer.advance_frames(5)
    e.add_remote_reports_from(peer, 3, 2)
    assert e.compare_reports(4, 2) == 0


def test_an_engine_without_the_comparison_is_unchanged(oracle):
    """Configuring the comparison changes nothing a session computes: states, rings, sessions, stats
    and report rows after 160 calls equal those of an engine that does not configure it."""
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    interval, mp = CASES[0]
    rows, arr, refs = matches(interval, mp)
    plain, dc = engine(0, mp, interval), engine(0, mp, interval, 64)
    for e in (plain, dc):
        e.add_inputs(0, rows[0])
        e.add_arrivals(0, arr[0])
        for n in CHUNKS[CASES[0]]:
            e.advance_frames(n)
    assert (plain.states() == dc.states()).all()
    for get in (lambda e: e.sessions(), lambda e: e.stats(), lambda e: tuple(e.reports(0, CALLS).values()),
                lambda e: e.ring(1), lambda e: e.ring(S - 1)):
        for a, b in zip(get(plain), get(dc)):
            assert (a == b).all()
    with pytest.raises(GgrsError) as err:
        plain.compare_reports(0, 1)
    assert err.value.code == GGRS_E_STATE
