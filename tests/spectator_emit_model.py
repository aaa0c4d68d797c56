"""Python restatement of the P2P engine's spectator emit (ggrs_p2p_set_spectator_emit /
emit_spectator_packets / read_spectator_emit_state, csrc/p2p_spec_emit.hip) over the oracle's wire
codec (oracle.codec_encode) -- the reference the device's send side towards spectators is compared
against.  A helper, not a test file; it lives here because oracle/ is frozen.

P2PSession::send_confirmed_inputs_to_spectators (src/sessions/p2p_session.rs:716-745) with
SyncLayer::confirmed_inputs (sync_layer.rs:296-310), per session and call c, as include/ggrs_amd.h
restates them:
  confirmed(): the call's confirmed_frame() (:542-553) and connect status, from the arrival table,
     the events and the frames the calls queued (packet_emit_model.pushes over the oracle's per-call
     `advanced`): the minimum over connected players of the local players' last queued frame before
     this call's add_local_input and of the remote players' last received frame, under the connect
     status after the call's poll (an Event::Disconnected freezes the player's last_frame);
  confirmed_row(): frame f's row as it is pushed -- player k's byte zero when disconnected[k] &&
     last_frame[k] < f, else a remote player's byte of input row f, a local player's byte of the row
     of the call that queued frame f;
  Endpoint: one spectator endpoint, packet_emit_model.Sender taking several pushes per call (pop, the
     pushes with the overflow check after each, one packet for the call);
  the note: 0, or GGRS_SPECTATOR_NOTE of the (c mod m)-th of the m disconnected players.
run(): a whole table of calls for S sessions and K endpoints -> emit_spectator_packets' outputs, the
confirmed rows and arrival table (what SpectatorEngine.add_inputs / add_arrivals take) and the final
state.
"""
import numpy as np

from oracle import oracle as O
from tests import packet_emit_model as E
from tests import spectator_model as SM

NULL_FRAME = -1
EMIT_DISCONNECTED, EMIT_ROW_LOST = E.EMIT_DISCONNECTED, -20


class Endpoint:
    def __init__(self, P, max_pending):
        self.P, self.max_pending = P, max_pending
        self.last_acked = (NULL_FRAME, bytes(P))
        self.pending = []  # (frame, bytes), consecutive frames
        self.status, self.closed_call = 0, -1

    def step(self, c, ack=NULL_FRAME, pushes=(), resend=False, lost=False):
        """-> (start_frame, packet bytes); (-1, b"") when nothing goes out."""
        if self.status:
            return -1, b""
        while self.pending and self.pending[0][0] <= ack:
            self.last_acked = self.pending.pop(0)
        if lost:
            self.status, self.closed_call = EMIT_ROW_LOST, c
            return -1, b""
        for frame, data in pushes:
            assert frame == (self.pending[-1][0] if self.pending else self.last_acked[0]) + 1
            self.pending.append((int(frame), bytes(data)))
            if len(self.pending) > self.max_pending:
                self.status, self.closed_call = EMIT_DISCONNECTED, c
                return -1, b""
        if self.pending and (pushes or resend):
            return self.pending[0][0], O.codec_encode(self.last_acked[1], [b for _, b in self.pending])
        return -1, b""


class Host:
    """One session's send_confirmed_inputs_to_spectators: rows [calls][P] u8 its input rows, arrive /
    events / pushed [calls] its columns of the tables."""

    def __init__(self, rows, arrive, events, pushed, local_mask):
        self.rows, self.arrive, self.events, self.pushed = rows, arrive, events, pushed
        self.P = rows.shape[1]
        self.local = [(local_mask >> k) & 1 for k in range(self.P)]
        self.next = 0
        self.delivered, self.local_last = NULL_FRAME, NULL_FRAME
        self.disc = [False] * self.P
        self.last_frame = [NULL_FRAME] * self.P
        self.queued_at = {}  # frame -> the call whose add_local_input queued it

    def confirmed(self, c):
        """The call's poll and confirmed_frame(); then its add_local_input."""
        self.delivered = max(self.delivered, int(self.arrive[c]))
        for k in range(self.P):
            if (self.events[c] >> k) & 1 and not self.local[k] and not self.disc[k]:
                self.disc[k], self.last_frame[k] = True, self.delivered
        live = [self.local_last if self.local[k] else self.delivered for k in range(self.P) if not self.disc[k]]
        conf = min(live)
        if self.pushed[c] != NULL_FRAME:
            self.local_last = int(self.pushed[c])
            self.queued_at[self.local_last] = c
        return conf

    def confirmed_row(self, f):
        out = bytearray(self.P)
        for k in range(self.P):
            if self.disc[k] and self.last_frame[k] < f:
                continue  # blank_input
            if not self.local[k]:
                out[k] = self.rows[f, k]
            elif f in self.queued_at:  # (the frames below the input delay were never queued: blank)
                out[k] = self.rows[self.queued_at[f], k]
        return bytes(out)

    def reads_row(self, f):
        """Whether frame f's row takes a byte from input row f: a remote player's that is not blank."""
        return any(not self.local[k] and not (self.disc[k] and self.last_frame[k] < f) for k in range(self.P))

    def note(self, c):
        gone = [k for k in range(self.P) if self.disc[k]]
        if not gone:
            return 0
        k = gone[c % len(gone)]
        return SM.note(k, self.last_frame[k])


class Session:
    """One session's host with its K endpoints, stepped call by call."""

    def __init__(self, rows, arrive, events, pushed, local_mask, K, max_pending, stop_call=-1):
        self.host = Host(rows, arrive, events, pushed, local_mask)
        self.eps = [Endpoint(rows.shape[1], max_pending) for _ in range(K)]
        self.stop_call, self.lost = stop_call, False

    def call(self, c, acks=None, resend=None, held_from=0):
        """-> (confirmed, note, the pushed [(frame, bytes)], [(start, data)] per endpoint); held_from:
        the oldest input row still held when the call is emitted."""
        K = len(self.eps)
        if 0 <= self.stop_call <= c:
            return NULL_FRAME, 0, [], [(-1, b"")] * K
        host = self.host
        conf, pushes = host.confirmed(c), []
        if not self.lost:
            if any(f < held_from and host.reads_row(f) for f in range(host.next, conf + 1)):
                self.lost = True
            else:
                pushes = [(f, host.confirmed_row(f)) for f in range(host.next, conf + 1)]
                host.next = max(host.next, conf + 1)
        sent = [ep.step(c, NULL_FRAME if acks is None else int(acks[k]), pushes,
                        bool(resend is not None and resend[k]), self.lost) for k, ep in enumerate(self.eps)]
        return conf, host.note(c), pushes, sent


def run(rows, arrive, events, pushed, local_mask, K, max_pending, stride, ack_in=None, resend=None, stop_call=None,
        held_from=None):
    """rows [calls][S][P] u8, arrive / events / pushed [calls][S], ack_in [calls][K][S] i32, resend
    [calls][K][S] u8, stop_call [S] (-1: none), held_from [calls]: the oldest input row still held
    when call c is emitted (None: every row).  Returns dict(start, length [calls][K][S], packets
    [calls][K][S][stride], notes, confirmed, npush [calls][S], conf_rows [calls + 16][S][P]
    (frame-indexed; zeros from next on), next [S], last_acked, pending, status, closed_call [K][S])."""
    calls, S, P = rows.shape
    out = dict(start=np.full((calls, K, S), -1, np.int32), length=np.zeros((calls, K, S), np.int32),
               packets=np.zeros((calls, K, S, stride), np.uint8), notes=np.zeros((calls, S), np.int32),
               confirmed=np.full((calls, S), NULL_FRAME, np.int32), npush=np.zeros((calls, S), np.int32),
               conf_rows=np.zeros((calls + 16, S, P), np.uint8), next=np.zeros(S, np.int32),
               last_acked=np.zeros((K, S), np.int32), pending=np.zeros((K, S), np.int32),
               status=np.zeros((K, S), np.int32), closed_call=np.zeros((K, S), np.int32))
    for s in range(S):
        ses = Session(rows[:, s], arrive[:, s], events[:, s], pushed[:, s], local_mask, K, max_pending,
                      -1 if stop_call is None else int(stop_call[s]))
        for c in range(calls):
            conf, note, pushes, sent = ses.call(c, None if ack_in is None else ack_in[c, :, s],
                                                None if resend is None else resend[c, :, s],
                                                0 if held_from is None else int(held_from[c]))
            out["confirmed"][c, s], out["notes"][c, s], out["npush"][c, s] = conf, note, len(pushes)
            for f, data in pushes:
                out["conf_rows"][f, s] = np.frombuffer(data, np.uint8)
            for k, (start, data) in enumerate(sent):
                out["start"][c, k, s], out["length"][c, k, s] = start, len(data)
                out["packets"][c, k, s, :len(data)] = np.frombuffer(data, np.uint8)
        out["next"][s] = ses.host.next
        for k, ep in enumerate(ses.eps):
            out["last_acked"][k, s], out["pending"][k, s] = ep.last_acked[0], len(ep.pending)
            out["status"][k, s], out["closed_call"][k, s] = ep.status, ep.closed_call
    return out


def confirmed_table(arrive, events, pushed, local_mask, P):
    """[calls][S] every call's confirmed_frame() (Host.confirmed), stopped sessions included."""
    calls, S = arrive.shape
    out = np.full((calls, S), NULL_FRAME, np.int32)
    for s in range(S):
        host = Host(np.zeros((calls, P), np.uint8), arrive[:, s], events[:, s], pushed[:, s], local_mask)
        for c in range(calls):
            out[c, s] = host.confirmed(c)
    return out


def acks(confirmed, K, seed, silent=(), silence=(90, 120)):
    """ack_in [calls][K][S] and resend [calls][K][S] from the model's confirmed table: each endpoint
    acks the frame confirmed 1..6 calls ago (a spectator cannot ack what was not sent), nothing at
    four calls in ten, nothing for calls silence[0]..silence[1] in every fourth session of every
    endpoint (pending grows), an ack beyond the newest pending frame in every seventh session at call
    150 (when the run is that long); endpoints in `silent` never ack.  Sparse resend flags."""
    calls, S = confirmed.shape
    rng = np.random.default_rng(seed)
    newest = np.maximum.accumulate(confirmed, axis=0)
    ack = np.full((calls, K, S), NULL_FRAME, np.int32)
    for k in range(K):
        lag = rng.integers(1, 7, (calls, S))
        src = np.maximum(np.arange(calls)[:, None] - lag, 0)
        a = newest[src, np.arange(S)[None, :]].astype(np.int32)
        a[np.arange(calls)[:, None] < lag] = NULL_FRAME
        a[rng.random((calls, S)) < 0.4] = NULL_FRAME
        a[silence[0]:silence[1], (1 + k) % 4::4] = NULL_FRAME
        if calls > 150:
            a[150, 3::7] = newest[150, 3::7] + 5
        if k in silent:
            a[:] = NULL_FRAME
        ack[:, k] = a
    resend = (rng.random((calls, K, S)) < 0.1).astype(np.uint8)
    return ack, resend


def link_tables(calls, K, S, seed, max_delay=3, loss=0.2, blackout_every=6, blackout_len=12, tail=8):
    """delay [calls][K][S] in 1..max_delay calls and drop [calls][K][S] bool for the host's packets --
    random loss, a blackout of blackout_len calls in every blackout_every-th session of each endpoint,
    nothing lost or late in the last `tail` calls -- and ack_drop [calls][K][S] for the spectators'
    InputAcks (one call on the way, lost one time in five); resend flags at calls with c % 4 == s % 4."""
    rng = np.random.default_rng(seed)
    delay = rng.integers(1, max_delay + 1, (calls, K, S)).astype(np.int32)
    drop = rng.random((calls, K, S)) < loss
    for k in range(K):
        for s in range(k, S, blackout_every):
            b0 = int(rng.integers(calls // 4, calls // 2))
            drop[b0:b0 + blackout_len, k, s] = True
    drop[calls - tail:] = False
    delay[calls - tail:] = 1
    ack_drop = rng.random((calls, K, S)) < 0.2
    ack_drop[calls - tail:] = False
    resend = np.broadcast_to((np.arange(calls)[:, None] % 4 == np.arange(S)[None, :] % 4)[:, None, :],
                             (calls, K, S)).astype(np.uint8)
    return delay, drop, ack_drop, resend


def route(c, delay, drop, sent_start):
    """The host call whose packet a spectator's poll of call c takes: the newest of the calls c2 < c
    with a packet that arrives now (c2 + delay[c2] == c) and was not dropped, or -1.  delay, drop,
    sent_start: one (endpoint, session)'s [calls] columns; delays are at most 4 calls."""
    src = -1
    for c2 in range(max(0, c - 4), c):
        if c2 + delay[c2] == c and not drop[c2] and sent_start[c2] >= 0:
            src = c2
    return src


def link_run(rows, arrive, events, pushed, local_mask, K, max_pending, delay, drop, ack_drop, resend, receivers,
             stop_call=-1):
    """One session's host and its K spectators' endpoints in a closed loop: tick c = the host's call
    c (acks: each spectator's last_recv after its call c - 1, unless ack_drop[c][k]), then every
    spectator's poll of call c (route()).  delay / drop / ack_drop / resend [calls][K]; receivers: K
    spectator_feed_model.Receiver.  Returns dict(start [calls][K], data [calls][K] (bytes), notes
    [calls], pushes {frame: bytes}, recv [calls][K] each receiver's last_recv after its call, took
    [calls][K] the host call whose packet it took (-1), session)."""
    calls = rows.shape[0]
    ses = Session(rows, arrive, events, pushed, local_mask, K, max_pending, stop_call)
    start = np.full((calls, K), -1, np.int32)
    data = [[b""] * K for _ in range(calls)]
    notes = np.zeros(calls, np.int32)
    recv = np.full((calls, K), NULL_FRAME, np.int32)
    took = np.full((calls, K), -1, np.int32)
    pushes = {}
    for c in range(calls):
        acks = [NULL_FRAME if c == 0 or ack_drop[c, k] else int(recv[c - 1, k]) for k in range(K)]
        _, notes[c], new, sent = ses.call(c, acks, resend[c])
        pushes.update(new)
        for k in range(K):
            start[c, k], data[c][k] = sent[k]
            src = route(c, delay[:, k], drop[:, k], start[:, k])
            took[c, k] = src
            if src >= 0:
                receivers[k].receive(c, int(start[src, k]), data[src][k])
            recv[c, k] = receivers[k].last
    return dict(start=start, data=data, notes=notes, pushes=pushes, recv=recv, took=took, session=ses)


def schedules(S, calls, mp, seed, local_mask, P, disconnect_every=5, second_every=0):
    """[calls][S] arrivals and events: per session its own network -- stalls of up to mp calls with
    bursts (2 of 3 sessions; mp above the session's max_prediction gives bursts that confirm more
    frames than that in one call), or a fixed latency -- a disconnect of one remote player in every
    disconnect_every-th session, and of a second one 20 calls later in every second_every-th."""
    arrive = np.zeros((calls, S), np.int32)
    events = np.zeros((calls, S), np.uint8)
    remote = [k for k in range(P) if not (local_mask >> k) & 1]
    rng = np.random.default_rng(seed)
    for s in range(S):
        kind = s % 3
        if kind == 2:
            arrive[:, s] = np.maximum(np.arange(calls) - int(rng.integers(1, 6)), -1)
        else:
            arrive[:, s] = O.stall_schedule(calls, mp, seed * 1000 + s, stall_every=40 if kind == 0 else 10 ** 9)
        if disconnect_every and s % disconnect_every == 0:
            c = int(rng.integers(calls // 4, calls // 2))
            events[c, s] = 1 << remote[s % len(remote)]
            if second_every and s % second_every == 0 and len(remote) > 1:
                events[c + 20, s] = 1 << remote[(s + 1) % len(remote)]
    return arrive, events


def pushed_table(rows, arrive, events, P, mask, delay, mp, sparse=False):
    """(pushed [calls][S], stop_call [S]) from the oracle's P2PSession: the frame each call queued
    (packet_emit_model.pushes over its per-call `advanced`), the call at which it panics (-1)."""
    calls, S = arrive.shape
    pushed = np.full((calls, S), NULL_FRAME, np.int32)
    stop = np.full(S, -1, np.int32)
    for s in range(S):
        out = O.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=mask,
                              input_delay=delay, max_prediction=mp, sparse_saving=sparse)
        if out["rc"] != 0:
            stop[s] = out["result"].frames_done
        n = calls if stop[s] < 0 else stop[s]
        pushed[:n, s] = E.pushes(out["advanced"][:n], delay)
    return pushed, stop
