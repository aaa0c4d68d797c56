"""Python restatement of the P2P engine's device-side checksum comparison
(ggrs_p2p_set_desync_compare / add_remote_reports / compare_reports, csrc/p2p_desync.hip) -- the
reference the device is compared against.  A helper, not a test file; it lives here because oracle/
is frozen.

Session: one session in the kernel's form -- local_checksum_history and pending_checksums as two
insertion-ordered lists of at most 32 (frame, checksum) entries, the cursor into the peer's report
rows, the newest frame received from the peer, last_recv, the status word and the summary.  step()
is one call in include/ggrs_amd.h's order: delivery (UdpProtocol::on_checksum_report,
protocol.rs:663-682), the local report (check_checksum_send_interval's history push,
p2p_session.rs:965-970), the comparison (compare_local_checksums_against_peers, :904-937).
Engine: S sessions behind the C ABI's calls -- the ring of the peer's rows, the "rows not yet added"
error, the lost row -- driven by report rows and arrival rows, never by the engine.
"""
import numpy as np

NULL_FRAME = -1
MAX_HISTORY = 32  # MAX_CHECKSUM_HISTORY_SIZE, protocol.rs:27
ROW_LOST = -21    # GGRS_DESYNC_ROW_LOST


class StateError(Exception):
    """GGRS_E_STATE of ggrs_p2p_compare_reports: the peer's rows of a call are missing."""


class Session:
    def __init__(self, interval):
        self.interval = interval
        self.history = []   # [(frame, checksum)], ascending frames, at most 32
        self.pending = []   # the same for the peer's reports
        self.cursor = 0     # the peer's rows delivered so far
        self.newest = NULL_FRAME  # the newest frame received from the peer
        self.last_recv = NULL_FRAME
        self.status = 0
        self.refused = 0
        self.n_events = 0
        self.first = (-1, -1, 0, 0)  # the first event's (call, frame, local, remote)
        # (for the tests' own conditions, not part of the state: entries a full table dropped)
        self.pruned_pending = self.pruned_history = self.pruned_history_past_pending = 0

    def deliver(self, frame, checksum):
        """on_checksum_report for one row of the peer's."""
        if frame < 0:
            return
        if frame == 0 or frame % self.interval or frame <= self.newest:
            self.refused += 1  # (the stated divergence: the reference accepts any frame)
            return
        if len(self.pending) >= MAX_HISTORY:
            oldest = frame - (MAX_HISTORY - 1) * self.interval
            k = 0
            while k < len(self.pending) and self.pending[k][0] < oldest:  # (ascending: a prefix)
                k += 1
            del self.pending[:k]
            self.pruned_pending += k
        assert len(self.pending) < MAX_HISTORY  # distinct multiples in [frame - 31 I, frame): 31 at most
        self.pending.append((frame, checksum))
        self.newest = frame

    def report(self, frame, checksum):
        """The local report of a call enters local_checksum_history."""
        if len(self.history) >= MAX_HISTORY:
            oldest = frame - (MAX_HISTORY - 1) * self.interval
            k = 0
            while k < len(self.history) and self.history[k][0] < oldest:
                k += 1
            del self.history[:max(k, 1)]  # (the engine's own reports are ascending multiples: k >= 1)
            self.pruned_history += max(k, 1)
            self.pruned_history_past_pending += bool(self.pending and self.pending[0][0] < self.history[0][0])
        self.history.append((frame, checksum))

    def compare(self, call, last_confirmed):
        """compare_local_checksums_against_peers: [(frame, local, remote)] of the call's events."""
        events, keep, h = [], [], 0
        for frame, remote in self.pending:  # ascending frames
            hit = False
            if frame < last_confirmed:
                while h < len(self.history) and self.history[h][0] < frame:
                    h += 1
                hit = h < len(self.history) and self.history[h][0] == frame
            if not hit:
                keep.append((frame, remote))
                continue
            local = self.history[h][1]
            if local != remote:
                events.append((frame, local, remote))
                if self.n_events == 0:
                    self.first = (call, frame, local, remote)
                self.n_events += 1
        self.pending = keep
        return events

    def step(self, call, recv, peer_rows, rep_frame, rep_ck, last_confirmed, feed=False):
        """Local call `call`; recv: the call's arrival word (feed: the feed's ack word); peer_rows(g)
        -> the peer's (frame, checksum, local_last) of its call g."""
        if self.status:
            return []
        self.last_recv = recv if feed else max(self.last_recv, recv)
        while self.cursor < call:
            frame, ck, ll = peer_rows(self.cursor)
            if ll > self.last_recv:
                break
            self.deliver(frame, ck)
            self.cursor += 1
        if rep_frame >= 0:
            self.report(rep_frame, rep_ck)
        return self.compare(call, last_confirmed)

    def tables(self):
        """(history, pending) as ggrs_p2p_read_desync_state returns them: [2][32], frames then
        checksums, -1 / 0 past the entries."""
        out = []
        for tab in (self.history, self.pending):
            a = np.zeros((2, MAX_HISTORY), np.int32)
            a[0] = -1
            for i, (f, c) in enumerate(tab):
                a[0, i], a[1, i] = f, c
            out.append(a)
        return out


class Engine:
    """S sessions behind ggrs_p2p_add_remote_reports / ggrs_p2p_compare_reports."""

    def __init__(self, S, interval, capacity, feed=False):
        self.S, self.cap, self.feed = S, capacity, feed
        self.sessions = [Session(interval) for _ in range(S)]
        self.ring = [None] * capacity  # the peer's rows, slot call % capacity
        self.added = 0
        self.next = 0
        self.lost_call = np.full(S, -1, np.int64)
        self.events = []  # (call, session, frame, local, remote)

    def add_remote_reports(self, first_call, frames, checksums, local_last):
        assert first_call == self.added
        for k in range(len(frames)):
            self.ring[(first_call + k) % self.cap] = (np.asarray(frames[k]), np.asarray(checksums[k]),
                                                      np.asarray(local_last[k]))
        self.added += len(frames)

    def compare_reports(self, first_call, own, recv):
        """own: the local report rows (P2PEngine.reports) of calls first_call .., recv [n][S] the
        arrival rows (or the feed's ack rows).  Returns the launch's events."""
        n = len(recv)
        assert first_call == self.next
        if n and self.added < first_call + n - 1:
            raise StateError(f"the peer's report rows of call {self.added} have not been added")
        out = []
        for s, x in enumerate(self.sessions):
            if not x.status and self.added - x.cursor > self.cap:
                x.status = ROW_LOST  # the ring no longer holds the row at the cursor
                self.lost_call[s] = first_call
            rows = lambda g, s=s: tuple(int(a[s]) for a in self.ring[g % self.cap])  # noqa: E731
            for k in range(n):
                c = first_call + k
                for f, l, r in x.step(c, int(recv[k][s]), rows, int(own["frame"][k][s]), int(own["checksum"][k][s]),
                                      int(own["last_confirmed"][k][s]), self.feed):
                    out.append((c, s, f, l, r))
        self.next = first_call + n
        out.sort()
        self.events += out
        return out

    def state(self):
        """What ggrs_p2p_read_desync_state returns: status, n_events, first_call, first_frame,
        first_local, first_remote, refused [S]; history, pending [2][32][S]."""
        x = self.sessions
        cols = [np.array([v.status for v in x]), np.array([v.n_events for v in x])]
        cols += [np.array([v.first[i] for v in x]) for i in range(4)]
        cols.append(np.array([v.refused for v in x]))
        tabs = [v.tables() for v in x]
        cols.append(np.stack([t[0] for t in tabs], axis=2))
        cols.append(np.stack([t[1] for t in tabs], axis=2))
        return cols


def summary_of(events, S):
    """(n_events, first_call, first_frame, first_local, first_remote) [S] from a list of (call,
    session, frame, local, remote): the first event is the one of the lowest (call, frame)."""
    out = [np.zeros(S, np.int64)] + [np.full(S, -1, np.int64) for _ in range(2)] + [np.zeros(S, np.int64) for _ in range(2)]
    for c, s, f, l, r in sorted(events):
        if out[0][s] == 0:
            out[1][s], out[2][s], out[3][s], out[4][s] = c, f, l, r
        out[0][s] += 1
    return out
