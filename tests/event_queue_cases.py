"""The inputs of the event-queue tests (tests/test_event_queue_model.py on the CPU,
tests/test_gpu_event_queue.py and tests/test_gpu_spectator_event_queue.py on the GPU): synthesized rows,
the model's run over them in pieces, and for every case the proof -- on the model's output -- that it
reaches the states it claims to test."""
import numpy as np

from tests import event_queue_model as M

S, CALLS, CAPACITY = 130, 160, 128   # two full waves and a two-lane tail; the smallest ring
RMASK = 2                            # two players, player 0 local
INTERRUPTED_MS, SPEC_INTERRUPTED_MS = 1500, 2000  # the polls' disconnect_timeout - disconnect_notify_start
PIECES = (1, 7, 64, 88)

# ggrs_event_record_t, restated
RECORD = np.dtype([("kind", "u1"), ("endpoint", "u1"), ("reserved", "<u2"), ("call", "<i4"), ("payload", "<u8")])


def pieces_of(pieces, calls):
    """(first call, calls) of the invocations: `pieces` calls at a time, cycling."""
    done, i = 0, 0
    while done < calls:
        n = min(pieces[i % len(pieces)], calls - done)
        yield done, n
        done, i = done + n, i + 1


def general(K, S_=S, calls=CALLS, seed=11):
    """Five kinds of session, s % 5: 0 quiet; 1 endpoint events at nearly every call (the trim at 100);
    2 the same for 100 calls, then desync and wait records alone (above 100); 3 a mix with spectator
    events; 4 a WaitRecommendation at every call and desync records, nothing handled (the ring
    overflows).  No session has more than 64 desync records."""
    rng = np.random.default_rng(seed + K)
    prof = np.arange(S_) % 5
    early = (np.arange(calls) < 100)[:, None]

    def per(p):
        return np.array(p)[prof][None, :]

    u = rng.random((6, calls, S_))
    p_net = np.where((prof == 2)[None, :] & ~early, 0.0, per([0.02, 0.9, 0.9, 0.3, 0.0]))
    net = np.where(u[0] < p_net, rng.integers(1, 16, (calls, S_)), 0).astype(np.uint8)
    p_hd = np.where((prof == 2)[None, :] & ~early, 0.0, per([0.5, 0.5, 0.5, 0.3, 0.0]))
    handled = (u[1] < p_hd).astype(np.uint8) * rng.integers(1, 256, (calls, S_)).astype(np.uint8)
    skip = np.where(u[2] < per([0.02, 0.05, 0.3, 0.05, 1.0]), rng.integers(1, 9, (calls, S_)), 0)
    skip = np.where(u[3] < 0.05, -rng.integers(0, 3, (calls, S_)), skip).astype(np.int32)
    skip[:, prof == 4] = np.abs(skip[:, prof == 4]) + 1
    disc_req = (u[4] < per([0.01, 0.0, 0.0, 0.01, 0.0])).astype(np.uint8)
    events = np.where(u[5] < per([0.01, 0.01, 0.0, 0.01, 0.0]), rng.integers(1, 4, (calls, S_)), 0).astype(np.uint8)
    spec = np.zeros((calls, K, S_), np.uint8)
    if K:
        hit = rng.random((calls, K, S_)) < np.array([0.0, 0.1, 0.0, 0.2, 0.0])[prof][None, None, :]
        spec = np.where(hit, rng.integers(1, 16, (calls, K, S_)), 0).astype(np.uint8)
    ds = []
    for s in range(S_):
        count, lo = {0: 2, 1: 0, 2: 30, 3: 5, 4: 40}[int(prof[s])], 100 if prof[s] == 2 else 0
        for c in rng.integers(lo, calls, count):
            ds.append((int(c), s, int(rng.integers(0, 10000)), int(rng.integers(0, 65536)), int(rng.integers(0, 65536))))
    # a call with three records of one session, two of them of one frame
    ds += [(150, 2, 700, 5, 6), (150, 2, 700, 5, 7), (150, 2, 70, 1, 2)]
    return dict(S=S_, calls=calls, K=K, events=events, disc_req=disc_req, handled=handled, net=net, spec_net=spec,
                skip=skip, desync=desync_arrays(ds, rng))


def desync_arrays(records, rng=None):
    """(call, session, frame, local, remote) arrays, shuffled with rng."""
    records = list(records)
    if rng is not None:
        records = [records[i] for i in rng.permutation(len(records))]
    cols = list(zip(*records)) if records else [[]] * 5
    return tuple(np.array(c, t) for c, t in zip(cols, (np.int32, np.int32, np.int32, np.uint16, np.uint16)))


def in_order(desync):
    o = np.lexsort((desync[2], desync[0], desync[1]))
    return tuple(a[o] for a in desync)


def desync_of(case, c0, n):
    """The records of calls c0 .. c0 + n - 1 (an invocation is given its own calls' records)."""
    d = case["desync"]
    keep = (d[0] >= c0) & (d[0] < c0 + n)
    return tuple(a[keep] for a in d)


def run_model(case, pieces=None, capacity=CAPACITY, spectator=False, drain_at=None, max_records=None):
    """The model over the case's rows in invocations of `pieces` calls (None: one).  drain_at: after the
    invocation that ends at this call, drain max_records; the drained list is returned as well."""
    m = M.EventQueueModel(case["S"], capacity, case.get("K", 0), RMASK, INTERRUPTED_MS, SPEC_INTERRUPTED_MS, spectator)
    drained = None
    for c0, n in pieces_of(pieces or (case["calls"],), case["calls"]):
        sl = slice(c0, c0 + n)
        if spectator:
            m.collect(c0, n, handled=case["handled"][sl], net=case["net"][sl])
        else:
            m.collect(c0, n, case["events"][sl], case["disc_req"][sl], case["handled"][sl], case["net"][sl],
                      case["spec_net"][sl] if case["K"] else None, case["skip"][sl], desync_of(case, c0, n))
        if drain_at == c0 + n:
            drained = m.drain(max_records)
    return (m, drained) if drain_at is not None else m


def queue_array(m, capacity=CAPACITY):
    """The model's queues as ggrs_*_read_event_queue_state returns them, [capacity][S]."""
    out = np.zeros((capacity, m.S), RECORD)
    for s, q in enumerate(m.sessions):
        for i, (kind, endpoint, call, payload) in enumerate(q.q):
            out[i, s] = (kind, endpoint, 0, call, payload)
    return out


def drained_array(records):
    out = np.zeros(len(records), np.dtype([("session", "<i4")] + [(n, RECORD.fields[n][0]) for n in RECORD.names]))
    for i, (s, kind, endpoint, call, payload) in enumerate(records):
        out[i] = (s, kind, endpoint, 0, call, payload)
    return out


def words(m):
    return (np.array(m.lengths(), np.int32), np.array([q.dropped for q in m.sessions], np.int32),
            np.array([q.status for q in m.sessions], np.int32), np.array([q.closed_call for q in m.sessions], np.int32))


def general_reaches_its_edges(case, m):
    """Every state the parity claims: a queue cut at 100, one above 100, a ring that overflowed, each
    way of closing, a suppressed Disconnected -- and no session over the staging bound."""
    length, dropped, status, closed = words(m)
    assert (length == M.MAX_EVENT_QUEUE_SIZE).any() and (length > M.MAX_EVENT_QUEUE_SIZE).any(), length
    assert (dropped > 0).any() and (length == CAPACITY).any()
    assert (length == 0).any() or (length < 10).any()
    assert (status == 0).all() and not m.over_stage
    dr, ev, net = case["disc_req"] != 0, (case["events"] & RMASK) != 0, (case["net"] & M.NET_DISCONNECTED) != 0
    how = {"disc_req": 0, "own": 0, "timeout": 0, "suppressed": 0, "open": 0}
    for s in range(case["S"]):
        c = closed[s]
        if c < 0:
            how["open"] += 1
            continue
        how["disc_req" if dr[c, s] else "own" if ev[c, s] else "timeout"] += 1
        assert dr[c, s] or ev[c, s] or net[c, s]
        how["suppressed"] += int(dr[c + 1:, s].any() or net[c + 1:, s].any())
    assert all(v > 0 for v in how.values()), how


def hand_sequences():
    """The sequences derived by hand from the reference, one session each, at capacity 128:
    0: 101 endpoint events leave the newest 100;
    1: a queue of 100 takes three DesyncDetected and one WaitRecommendation (104), stays at 104 over a
       call with nothing handled, and is cut to 100 by a call whose only endpoint activity is a handled
       Input;
    2: on top of 100, four calls of 10 desync records each with nothing handled: 140 pushed into a ring
       of 128, the oldest 12 dropped;
    3: 65 desync records in one call: over the staging bound of an invocation;
    4: one call with everything: Resumed, the requested Disconnected, Interrupted, (no second
       Disconnected), two spectators' events, two desync records in frame order, a WaitRecommendation;
    5: the host's own disconnect, then a disconnect request: nothing;
    6: a disconnect request, then the timeout: one Disconnected."""
    S_, calls, K = 7, 110, 2
    z = lambda dt=np.uint8: np.zeros((calls, S_), dt)  # noqa: E731
    events, disc_req, handled, net, skip = z(), z(), z(), z(), z(np.int32)
    spec = np.zeros((calls, K, S_), np.uint8)
    ds = []
    # sessions 0, 1, 2: a Resumed / Interrupted pair alternates over calls 0 .. 99 (100 events)
    for s in (0, 1, 2):
        net[:100:2, s] = M.NET_INTERRUPTED
        net[1:100:2, s] = M.NET_RESUMED
    net[100, 0] = M.NET_INTERRUPTED
    ds += [(100, 1, 30, 1, 2), (100, 1, 10, 3, 4), (100, 1, 20, 5, 6)]
    skip[100, 1] = 3
    handled[102, 1] = 1   # (call 101: nothing at all)
    for c in range(100, 104):
        ds += [(c, 2, 7 * f, f, c) for f in range(10)]
    ds += [(5, 3, f, 1, 2) for f in range(65)]
    net[3, 4] = M.NET_RESUMED | M.NET_INTERRUPTED | M.NET_DISCONNECTED | M.NET_SHUTDOWN
    disc_req[3, 4] = 1
    events[3, 4] = RMASK
    handled[3, 4] = 1
    spec[3, 0, 4] = M.NET_DISCONNECTED | M.NET_RESUMED
    spec[3, 1, 4] = M.NET_INTERRUPTED
    ds += [(3, 4, 9, 1, 2), (3, 4, 2, 3, 4)]
    skip[3, 4] = 5
    events[2, 5] = RMASK
    disc_req[6, 5] = 1
    net[9, 5] = M.NET_DISCONNECTED
    disc_req[2, 6] = 1
    events[2, 6] = RMASK  # (the wire envelope sets the bit with the request)
    net[8, 6] = M.NET_DISCONNECTED
    return dict(S=S_, calls=calls, K=K, events=events, disc_req=disc_req, handled=handled, net=net, spec_net=spec,
                skip=skip, desync=desync_arrays(ds, np.random.default_rng(5)))


def sparse(S_, busy_every=37, calls=3):
    """Events in one session of busy_every: the drain's scan crosses its block level with mostly empty
    blocks."""
    net = np.zeros((calls, S_), np.uint8)
    net[:, ::busy_every] = M.NET_INTERRUPTED | M.NET_RESUMED
    skip = np.zeros((calls, S_), np.int32)
    skip[1, ::busy_every] = 2
    z = np.zeros((calls, S_), np.uint8)
    return dict(S=S_, calls=calls, K=0, events=z, disc_req=z, handled=z, net=net, spec_net=None, skip=skip,
                desync=desync_arrays([]))


def spectator_case(S_=S, calls=CALLS, seed=23):
    """Spectator sessions, s % 3: 0 quiet, 1 an event at nearly every call, 2 a mix."""
    rng = np.random.default_rng(seed)
    prof = np.arange(S_) % 3
    p = np.array([0.03, 0.95, 0.4])[prof][None, :]
    net = np.where(rng.random((calls, S_)) < p, rng.integers(1, 16, (calls, S_)), 0).astype(np.uint8)
    handled = (rng.random((calls, S_)) < 0.5).astype(np.uint8)
    return dict(S=S_, calls=calls, K=0, handled=handled, net=net)
