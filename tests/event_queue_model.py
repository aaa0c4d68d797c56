"""The sessions' GgrsEvent queue, restated in plain Python from the reference (no code shared with the
kernels): P2PSession::event_queue as advance_frame fills it (src/sessions/p2p_session.rs:265-357) --
poll_remote_clients' handle_event with its trim to MAX_EVENT_QUEUE_SIZE (:430-469, :846-902),
compare_local_checksums_against_peers (:904-937) and check_wait_recommendation (:804-817), which push
without a trim -- and SpectatorSession::handle_event (src/sessions/p2p_spectator_session.rs:199-239).

A record is (kind, endpoint, call, payload).  One VecDeque per session, bounded by the ring's capacity
(the stated divergence: a push into a full ring drops the oldest record and counts it)."""
from collections import deque

MAX_EVENT_QUEUE_SIZE = 100  # p2p_session.rs:27
STAGE_D = 64                # desync records a session takes from one invocation
DISCONNECTED, NETWORK_INTERRUPTED, NETWORK_RESUMED, WAIT_RECOMMENDATION, DESYNC_DETECTED = 1, 2, 3, 4, 5
NET_INTERRUPTED, NET_RESUMED, NET_DISCONNECTED, NET_SHUTDOWN = 1, 2, 4, 8
EVENTS_LOST = -27


def desync_payload(frame, local, remote):
    return (frame & 0xffffffff) | ((local | remote << 16) << 32)


class SessionQueue:
    def __init__(self, capacity):
        self.capacity = capacity
        self.q = deque()
        self.dropped = 0
        self.status = 0
        self.closed_call = -1

    def push(self, kind, endpoint, call, payload=0):
        if len(self.q) == self.capacity:  # the ring is full (the reference's VecDeque grows)
            self.q.popleft()
            self.dropped += 1
        self.q.append((kind, endpoint, call, payload))

    def trim(self):  # the end of handle_event, :898-901
        while len(self.q) > MAX_EVENT_QUEUE_SIZE:
            self.q.popleft()

    def handle(self, kind, endpoint, call, payload=0):  # a handle_event that forwards to the user
        self.push(kind, endpoint, call, payload)
        self.trim()

    def remote_endpoint(self, c, net, disc_req, closes, interrupted_ms):
        """The events of the endpoint whose closing the session remembers, in the order its
        event_queue holds them: handle_message's Resumed (protocol.rs:547-551), on_input's Disconnected
        (:569-574), poll's Interrupted and Disconnected (:350-366)."""
        if net & NET_RESUMED:
            self.handle(NETWORK_RESUMED, 0, c)
        if disc_req:
            if self.closed_call < 0:  # state != Disconnected && !disconnect_event_sent
                self.handle(DISCONNECTED, 0, c)
        if (disc_req or closes) and self.closed_call < 0:
            self.closed_call = c  # disconnect_player_at_frame -> endpoint.disconnect(), no event of its own
        if net & NET_INTERRUPTED:
            self.handle(NETWORK_INTERRUPTED, 0, c, interrupted_ms)
        if net & NET_DISCONNECTED and self.closed_call < 0:
            self.handle(DISCONNECTED, 0, c)
            self.closed_call = c

    def spectator_endpoint(self, c, k, net, interrupted_ms):
        if net & NET_RESUMED:
            self.handle(NETWORK_RESUMED, 1 + k, c)
        if net & NET_INTERRUPTED:
            self.handle(NETWORK_INTERRUPTED, 1 + k, c, interrupted_ms)
        if net & NET_DISCONNECTED:
            self.handle(DISCONNECTED, 1 + k, c)

    def p2p_call(self, c, events=0, disc_req=0, handled=0, net=0, spec_net=(), skip=0, desync=(), rmask=0,
                 interrupted_ms=0, spec_interrupted_ms=0):
        """Call c of a P2PSession.  desync: the call's (frame, local, remote) records."""
        # a. poll_remote_clients: the remote endpoint, then the spectators in ascending order
        self.remote_endpoint(c, net, disc_req, (events & rmask) != 0, interrupted_ms)
        for k, sn in enumerate(spec_net):
            self.spectator_endpoint(c, k, sn, spec_interrupted_ms)
        if handled:  # Event::Input: handled, nothing pushed, the trim runs
            self.trim()
        # b. compare_local_checksums_against_peers: ascending frame order, no trim
        for frame, local, remote in sorted(desync, key=lambda r: (r[0], r[1] | r[2] << 16)):
            self.push(DESYNC_DETECTED, 0, c, desync_payload(frame, local, remote))
        # c. check_wait_recommendation, no trim
        if skip > 0:
            self.push(WAIT_RECOMMENDATION, 0, c, skip)

    def spectator_call(self, c, handled=0, net=0, interrupted_ms=0):
        """Call c of a SpectatorSession: its host endpoint's events; GGRS_NET_DISCONNECTED stands for
        both causes of the one Disconnected."""
        self.remote_endpoint(c, net, 0, False, interrupted_ms)
        if handled:
            self.trim()


class EventQueueModel:
    """S sessions' queues and the unit's interface: collect() is one invocation, drain() the drain."""

    def __init__(self, num_sessions, capacity, num_spectators=0, rmask=0, interrupted_ms=0, spec_interrupted_ms=0,
                 spectator=False):
        self.S, self.K, self.rmask = num_sessions, num_spectators, rmask
        self.ims, self.sims, self.spectator = interrupted_ms, spec_interrupted_ms, spectator
        self.sessions = [SessionQueue(capacity) for _ in range(num_sessions)]
        self.over_stage = set()  # sessions whose queue is unspecified: more than STAGE_D records in one invocation

    def collect(self, first_call, n, events=None, disc_req=None, handled=None, net=None, spec_net=None, skip=None,
                desync=None):
        """Rows are [n][S] (spec_net [n][K][S]) sequences or None; desync (call, session, frame, local,
        remote) sequences in any order."""
        per = {}
        if desync is not None:
            for c, s, f, lo, re in zip(*desync):
                c, s = int(c), int(s)
                if first_call <= c < first_call + n and 0 <= s < self.S:
                    per.setdefault(s, {}).setdefault(c, []).append((int(f), int(lo), int(re)))
        for s, by_call in per.items():
            if sum(len(v) for v in by_call.values()) > STAGE_D:
                self.sessions[s].status = EVENTS_LOST
                self.over_stage.add(s)

        def at(rows, k, s):
            return 0 if rows is None else int(rows[k][s])

        for s, q in enumerate(self.sessions):
            mine = per.get(s, {})
            for k in range(n):
                c = first_call + k
                if self.spectator:
                    q.spectator_call(c, at(handled, k, s), at(net, k, s), self.ims)
                else:
                    sn = () if spec_net is None else tuple(int(spec_net[k][j][s]) for j in range(self.K))
                    q.p2p_call(c, at(events, k, s), at(disc_req, k, s), at(handled, k, s), at(net, k, s), sn,
                               at(skip, k, s), mine.get(c, ()), self.rmask, self.ims, self.sims)

    def drain(self, max_records):
        """(records as (session, kind, endpoint, call, payload), n_left): whole sessions in ascending
        order while they fit; the first that does not fit and all later ones keep their queues."""
        out, used = [], 0
        for s, q in enumerate(self.sessions):
            if used + len(q.q) > max_records:
                break
            out += [(s,) + r for r in q.q]
            used += len(q.q)
            q.q.clear()
        return out, sum(len(q.q) for q in self.sessions)

    def lengths(self):
        return [len(q.q) for q in self.sessions]
