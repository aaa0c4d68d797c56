"""CPU checks of tests/desync_compare_model.py, the reference of the device's checksum comparison
(ggrs_p2p_set_desync_compare / add_remote_reports / compare_reports): against
ggrs_amd.desync.SchedDesyncDetector event for event and table for table after every call -- on the
oracle pair's rows and on synthetic rows that fill both 32-entry tables -- the refused reports, the
lost row and the "rows not yet added" error; and the inputs of the GPU parity test
(tests/test_gpu_desync_compare.py), so that the conditions that test relies on are asserted here on
the model alone."""
import functools

import numpy as np
import pytest

from tests import desync_compare_model as M

S, CALLS = 70, 160
CASES = [(7, 8), (1, 6), (25, 9)]  # (interval, max_prediction)


@functools.lru_cache(maxsize=None)
def matches(interval, mp, S_=S, calls=CALLS, corrupt_every=3):
    """tests/test_gpu_sched_desync.py's build_matches at S sessions: the engines' rows [2][calls][S][P],
    arrivals [2][calls][S] and the oracle's pair run per session."""
    from ggrs_amd import synth
    from oracle import oracle
    oracle.build()
    seed, P = 0x5EED + interval, 2
    rows = np.zeros((2, calls, S_, P), np.uint8)
    arr = np.zeros((2, calls, S_), np.int32)
    refs = []
    rng = np.random.default_rng(seed)
    for s in range(S_):
        inp = np.stack([synth.gen_inputs(2 * s + k, 1, calls, P, synth.MODEL_HELD, base=seed)[:, 0] for k in (0, 1)])
        a = np.stack([synth.jitter_arrivals(s, 1, calls, mp, stalls=(s + k) % 2 == 0, seed=seed + k)[:, 0]
                      for k in (0, 1)])
        cp, cc = (-1, -1)
        if s % corrupt_every == 1:
            cp, cc = int(rng.integers(0, 2)), int(rng.integers(calls // 5, 3 * calls // 5))
        out = oracle.p2p_sched_desync_pair_run(inp, a, P, mp, (1, 2), 0, interval, corrupt_peer=cp, corrupt_call=cc)
        rows[:, :, s, :] = out["eff_inputs"]
        arr[:, :, s] = out["eff_arrive"]
        refs.append(out)
    return rows, arr, refs


def report_rows(refs, k):
    """Peer k's report rows as P2PEngine.reports returns them, [calls][S] each."""
    return dict(frame=np.stack([o["rep_frame"][k] for o in refs], axis=1).astype(np.int32),
                checksum=np.stack([o["rep_cs"][k] for o in refs], axis=1).astype(np.uint16),
                last_confirmed=np.stack([o["lconf"][k] for o in refs], axis=1).astype(np.int32),
                local_last=np.stack([o["local_last"][k] for o in refs], axis=1).astype(np.int32))


def oracle_events(refs, k):
    """Peer k's events (call, session, frame, local, remote), sorted."""
    return sorted((c, s, f, l, r) for s, o in enumerate(refs) for (p, c, f, l, r) in o["events"] if p == k)


def cut(rows, a, b):
    return {k: v[a:b] for k, v in rows.items()}


@functools.lru_cache(maxsize=None)
def model_run(interval, mp, k, S_=S, calls=CALLS):
    """The model of peer k over the whole run, one launch with every row added: (engine, events)."""
    rows, arr, refs = matches(interval, mp, S_, calls)
    own, peer = report_rows(refs, k), report_rows(refs, 1 - k)
    m = M.Engine(S_, interval, calls)
    m.add_remote_reports(0, peer["frame"], peer["checksum"], peer["local_last"])
    return m, m.compare_reports(0, own, arr[k])


class StubEngine:
    """What SchedDesyncDetector needs of a P2PEngine, over given report rows."""

    def __init__(self, own):
        self.own = own
        self.num_sessions = own["frame"].shape[1]
        self.run = 0

    def set_desync_detection(self, interval):
        self.desync_interval = interval

    def calls(self):
        return self.run

    def reports(self, first, n):
        return cut(self.own, first, first + n)


def against_sched_detector(interval, own, peer, arrive, capacity=None):
    """The model and SchedDesyncDetector call by call over the same rows: every call's events and both
    tables of every session after it.  Returns the model engine."""
    from ggrs_amd.desync import SchedDesyncDetector
    calls, S_ = arrive.shape
    stub = StubEngine(own)
    det = SchedDesyncDetector(stub, interval, addr=7)
    det.note_arrivals(0, arrive)
    m = M.Engine(S_, interval, capacity or calls)
    for c in range(calls):
        if c > 0:  # the peer's rows of call c - 1: all that call c can deliver
            det.receive(c - 1, cut(peer, c - 1, c))
            m.add_remote_reports(c - 1, peer["frame"][c - 1:c], peer["checksum"][c - 1:c], peer["local_last"][c - 1:c])
        stub.run = c + 1
        want = sorted((ev.call, ev.session, ev.frame, ev.local_checksum, ev.remote_checksum) for ev in det.poll())
        got = m.compare_reports(c, cut(own, c, c + 1), arrive[c:c + 1])
        assert got == want, c
        for s, x in enumerate(m.sessions):
            assert x.history == sorted(det.local[s].items()), (c, s)
            assert x.pending == sorted(det.pending[s].items()), (c, s)
            assert x.cursor == det.next_remote[s], (c, s)
    return m


@pytest.mark.parametrize("interval,mp", CASES)
def test_model_matches_the_host_detector_on_the_oracle_pair(oracle, interval, mp):
    rows, arr, refs = matches(interval, mp)
    for k in (0, 1):
        own, peer = report_rows(refs, k), report_rows(refs, 1 - k)
        assert (np.diff(arr[k], axis=0) >= 0).all()  # (arrival rows never fall: the running maximum is the row)
        m = against_sched_detector(interval, own, peer, arr[k])
        assert m.events == oracle_events(refs, k)
        assert all(x.refused == 0 and x.status == 0 for x in m.sessions)
        one, events = model_run(interval, mp, k)  # one launch with every row added: the same
        assert events == m.events
        for a, b in zip(one.state(), m.state()):
            assert (a == b).all()
        for got, want in zip(m.state()[1:6], M.summary_of(m.events, S)):
            assert (got == want).all()


def test_the_parity_inputs_prove_something(oracle):
    """What the issue probed at these shapes: the events per peer, the most per (session, call), only
    the corrupted matches raise any, every rc 0; and the tables are not empty at the end."""
    want = {(7, 8): (275, 272, 1), (1, 6): (1844, 1843, 5), (25, 9): (64, 64, 1)}
    pending_at_the_end = 0
    for (interval, mp), (n0, n1, most) in want.items():
        rows, arr, refs = matches(interval, mp)
        assert all((o["rc"] == 0).all() for o in refs)
        ev = [oracle_events(refs, k) for k in (0, 1)]
        assert (len(ev[0]), len(ev[1])) == (n0, n1)
        per = {}
        for k in (0, 1):
            for c, s, f, l, r in ev[k]:
                per[(k, c, s)] = per.get((k, c, s), 0) + 1
        assert max(per.values()) == most
        assert all(s % 3 == 1 for k in (0, 1) for c, s, f, l, r in ev[k])
        m, _ = model_run(interval, mp, 0)
        assert sum(len(x.history) for x in m.sessions) > S
        pending_at_the_end += sum(len(x.pending) for x in m.sessions)
    assert pending_at_the_end > 0
    m, _ = model_run(1, 6, 0)
    assert max(len(x.history) for x in m.sessions) == M.MAX_HISTORY  # interval 1: the history is pruned


def synthetic(calls, S_, interval, seed):
    """Rows with ascending multiples of the interval that fill both tables: every session reports on
    most calls; its last_confirmed stalls for a stretch of more than 32 reports (the pending table is
    pruned while nothing can be compared) and the local reports stop for another (the history is pruned
    past frames still pending once they resume); one local checksum in eight differs."""
    rng = np.random.default_rng(seed)
    own = dict(frame=np.full((calls, S_), -1, np.int32), checksum=np.zeros((calls, S_), np.uint16),
               last_confirmed=np.zeros((calls, S_), np.int32), local_last=np.zeros((calls, S_), np.int32))
    peer = dict(frame=np.full((calls, S_), -1, np.int32), checksum=np.zeros((calls, S_), np.uint16),
                local_last=np.zeros((calls, S_), np.int32))
    arrive = np.zeros((calls, S_), np.int32)
    for s in range(S_):
        stall0 = int(rng.integers(20, 40))    # last_confirmed stalls over [stall0, stall0 + 45)
        quiet0 = int(rng.integers(100, 120))  # no local report over [quiet0, quiet0 + 50)
        lf = pf = lc = 0
        recv = -1
        for c in range(calls):
            peer["local_last"][c, s] = own["local_last"][c, s] = c
            if c % 11:  # (every eleventh call delivers nothing)
                recv = max(recv, c - 1 - int(rng.integers(0, 3)))
            arrive[c, s] = recv
            if rng.random() < 0.9:  # the peer reports, sometimes skipping a multiple
                pf += interval * int(rng.integers(1, 3))
                peer["frame"][c, s] = pf
                peer["checksum"][c, s] = pf * 7 & 0xFFFF
            if not stall0 <= c < stall0 + 45:
                lc = max(lc, lf - interval * int(rng.integers(0, 3)))
            own["last_confirmed"][c, s] = lc
            if not quiet0 <= c < quiet0 + 50 and rng.random() < 0.9:
                lf += interval * int(rng.integers(1, 3))
                own["frame"][c, s] = lf
                own["checksum"][c, s] = (lf * 7 + int(rng.random() < 0.125)) & 0xFFFF
    return own, peer, arrive


@pytest.mark.parametrize("interval", [1, 4])
def test_model_matches_the_host_detector_with_both_tables_full(interval):
    calls, S_ = 220, 12
    own, peer, arrive = synthetic(calls, S_, interval, 31 + interval)
    m = against_sched_detector(interval, own, peer, arrive)
    assert len(m.events) > 20 and all(x.refused == 0 for x in m.sessions)
    # the rows did what they are for, in every session: reports pruned from a full pending table behind
    # the stalled last_confirmed, and history entries pruned while an older report was still pending
    for x in m.sessions:
        assert x.pruned_pending > 0 and x.pruned_history > 0 and x.pruned_history_past_pending > 0


def test_refused_reports():
    """A frame that is no multiple of the interval, a repeated frame, a descending frame, frame 0: each
    refused and counted, the table untouched; the reports around them are kept."""
    x = M.Session(5)
    for f in (10, 12, 10, 5, 0, 15, 15, 20):
        x.deliver(f, f + 1)
    assert x.pending == [(10, 11), (15, 16), (20, 21)] and x.refused == 5 and x.newest == 20
    x.deliver(-1, 0)  # no report: not refused
    assert x.refused == 5
    own, peer, arrive = refused_case(1)
    m = M.Engine(1, 5, len(arrive))
    m.add_remote_reports(0, peer["frame"], peer["checksum"], peer["local_last"])
    assert m.compare_reports(0, own, arrive) == []
    assert m.sessions[0].pending == x.pending and m.state()[6][0] == 5


def refused_case(S_):
    """The frames of test_refused_reports as the peer's rows (session s: from call s % 8 on, its last
    s % 3 frames left out, so sessions differ), nothing to compare; 17 calls."""
    seq = (10, 12, 10, 5, 0, 15, 15, 20)
    n = len(seq) + 9
    peer = dict(frame=np.full((n, S_), -1, np.int32), checksum=np.zeros((n, S_), np.uint16),
                local_last=np.zeros((n, S_), np.int32))
    for s in range(S_):
        k = s % 8
        peer["frame"][k:k + len(seq), s] = seq[:len(seq) - s % 3] + (-1,) * (s % 3)
        peer["checksum"][:, s] = (peer["frame"][:, s] + 1).astype(np.uint16)
    own = dict(frame=np.full((n, S_), -1, np.int32), checksum=np.zeros((n, S_), np.uint16),
               last_confirmed=np.zeros((n, S_), np.int32), local_last=np.zeros((n, S_), np.int32))
    return own, peer, np.zeros((n, S_), np.int32)


def test_pending_never_exceeds_32():
    """Nothing comparable: the 33rd report drops those below frame - 31 interval, and at most 31
    survive whatever gaps the frames have."""
    x = M.Session(3)
    f = 0
    rng = np.random.default_rng(3)
    for _ in range(400):
        f += 3 * int(rng.integers(1, 4))
        x.deliver(f, 1)  # (asserts the bound itself)
        assert len(x.pending) <= M.MAX_HISTORY and x.pending[-1][0] == f
    assert x.refused == 0 and x.pruned_pending > 100


def lost_row_case(S_=70, calls=96, capacity=24, interval=2, recover=True):
    """Synthetic rows for the lost row: every third session's arrivals stall at frame 9 over calls
    10..49 (recover False: to the end) while the peer's local_last keeps rising, so its cursor stays at the row of call 10; rows are
    added and compared 8 calls at a time over a ring of 24."""
    own = dict(frame=np.full((calls, S_), -1, np.int32), checksum=np.zeros((calls, S_), np.uint16),
               last_confirmed=np.zeros((calls, S_), np.int32), local_last=np.zeros((calls, S_), np.int32))
    peer = dict(frame=np.full((calls, S_), -1, np.int32), checksum=np.zeros((calls, S_), np.uint16),
                local_last=np.zeros((calls, S_), np.int32))
    arrive = np.zeros((calls, S_), np.int32)
    for c in range(calls):
        arrive[c] = c - 1
        peer["local_last"][c] = c
        own["local_last"][c] = c
        own["last_confirmed"][c] = max(c - 3, -1)
        if c >= 4 and c % interval == 0:
            f = c - 2
            own["frame"][c] = peer["frame"][c] = f
            own["checksum"][c] = f * 3 & 0xFFFF
            peer["checksum"][c] = (f * 3 + (np.arange(S_) % 5 == 2) * (c > 60 or c < 20)) & 0xFFFF
    stalled = np.arange(S_) % 3 == 0
    arrive[10:50 if recover else calls, stalled] = 9
    return own, peer, arrive, stalled, capacity


def run_in_steps(m, own, peer, arrive, step):
    """Add the peer's rows and compare, `step` calls at a time (the peer a step ahead, as two engines
    advanced together are)."""
    calls = arrive.shape[0]
    for c0 in range(0, calls, step):
        m.add_remote_reports(c0, peer["frame"][c0:c0 + step], peer["checksum"][c0:c0 + step],
                             peer["local_last"][c0:c0 + step])
        m.compare_reports(c0, cut(own, c0, c0 + step), arrive[c0:c0 + step])
    return m


def test_lost_row():
    own, peer, arrive, stalled, cap = lost_row_case()
    m = run_in_steps(M.Engine(arrive.shape[1], 2, cap), own, peer, arrive, 8)
    status = m.state()[0]
    assert (status[stalled] == M.ROW_LOST).all() and (status[~stalled] == 0).all()
    # the cursor sits at row 10 (local_last 10 > 9); the launch of calls 32..39 starts with 40 rows added:
    # 40 - 10 > 24
    assert (m.lost_call[stalled] == 32).all() and all(x.cursor == 10 for x, st in zip(m.sessions, stalled) if st)
    # the stalled sessions raise nothing from there on; the others are those of a run that loses nothing
    big = run_in_steps(M.Engine(arrive.shape[1], 2, arrive.shape[0]), own, peer, arrive, 8)
    assert all(c < 32 for c, s, f, l, r in m.events if stalled[s])
    assert [e for e in m.events if not stalled[e[1]]] == [e for e in big.events if not stalled[e[1]]]
    assert any(stalled[e[1]] and e[0] >= 32 for e in big.events) and any(stalled[e[1]] for e in m.events)
    assert (big.state()[0] == 0).all()


def test_peer_rows_not_yet_added():
    own, peer, arrive, _, _ = lost_row_case()
    m = M.Engine(arrive.shape[1], 2, 64)
    m.add_remote_reports(0, peer["frame"][:7], peer["checksum"][:7], peer["local_last"][:7])
    with pytest.raises(M.StateError, match="call 7 "):
        m.compare_reports(0, cut(own, 0, 9), arrive[:9])  # calls 0..8 need the peer's rows 0..7
    assert m.next == 0 and all(x.cursor == 0 for x in m.sessions)  # nothing was taken
    m.compare_reports(0, cut(own, 0, 8), arrive[:8])  # calls 0..7 need rows 0..6
    assert m.next == 8
