"""Python restatement of the P2P engine's packet emit (ggrs_p2p_set_packet_emit / emit_packets,
csrc/p2p_emit.hip) over the oracle's wire codec (oracle.codec_encode) -- the reference the device's
send side is compared against.  A helper, not a test file; it lives here because oracle/ is frozen.

Sender: one session's endpoint, UdpProtocol::send_input / send_pending_output / pop_pending_output
(src/network/protocol.rs:378-391, :421-487) as include/ggrs_amd.h restates them.  Per call, in order:
  1. ack: pop every pending input with frame <= ack; last_acked = the last one popped;
  2. close: an Event::Disconnected of a remote player closes the stream (EMIT_CLOSED), nothing is
     emitted from this call on;
  3. push: the call's accepted local input (frame, B bytes); more than max_pending pending closes
     the stream (EMIT_DISCONNECTED), the overflowing call emits nothing;
  4. packet: when a frame was pushed, or the resend flag is set and something is pending:
     (first pending frame, codec_encode(last_acked bytes, pending...));
  6. a stopped session takes no step.
(5, ack_frame, is the receive side's last_recv_frame: the callers below carry it.)

pushes(): which calls queue a local input, from the oracle's per-call `advanced`.
run(): a whole table of calls for S sessions -> emit_packets' outputs.
pair_run(): two peers, each a Sender + a packet_feed_model.Receiver + the session's frame counters,
joined through per-direction delay and drop tables.
"""
import numpy as np

from oracle import oracle as O
from tests import packet_feed_model as F

NULL_FRAME = -1
EMIT_CLOSED, EMIT_DISCONNECTED = -18, -19


class Sender:
    def __init__(self, B, max_pending):
        self.B, self.max_pending = B, max_pending
        self.last_acked = (NULL_FRAME, bytes(B))
        self.pending = []  # (frame, bytes), consecutive frames
        self.status, self.closed_call = 0, -1
        self.max_seen = 0

    def step(self, c, ack=NULL_FRAME, close=False, push=None, resend=False, stopped=False):
        """-> (start_frame, packet bytes); (-1, b"") when nothing goes out."""
        if stopped or self.status:
            return -1, b""
        while self.pending and self.pending[0][0] <= ack:
            self.last_acked = self.pending.pop(0)
        if close:
            self.status, self.closed_call = EMIT_CLOSED, c
            return -1, b""
        if push is not None:
            assert not self.pending or push[0] == self.pending[-1][0] + 1
            self.pending.append((int(push[0]), bytes(push[1])))
            if len(self.pending) > self.max_pending:
                self.status, self.closed_call = EMIT_DISCONNECTED, c
                return -1, b""
            self.max_seen = max(self.max_seen, len(self.pending))
        if self.pending and (push is not None or resend):
            return self.pending[0][0], O.codec_encode(self.last_acked[1], [b for _, b in self.pending])
        return -1, b""


def local_columns(num_players, local_mask):
    return [k for k in range(num_players) if (local_mask >> k) & 1]


def pushes(advanced, input_delay):
    """[calls] the frame each call's add_local_input queued, NULL_FRAME where it was dropped
    (input_queue.rs:170-186: only the frame after the last queued one is taken), from the session's
    per-call `advanced` (current_frame rises where it is set)."""
    out = np.full(len(advanced), NULL_FRAME, np.int32)
    cur, ll = 0, NULL_FRAME
    for c, adv in enumerate(advanced):
        qf = cur + input_delay
        if ll == NULL_FRAME or qf == ll + 1:
            ll = qf
            out[c] = qf
        cur += int(adv)
    return out


def run(rows, pushed, local_mask, max_pending, stride, ack_in=None, resend=None, events=None, recv=None,
        stop_call=None):
    """rows [calls][S][P] u8, pushed [calls][S] (pushes() per session), ack_in [calls][S] i32, resend
    [calls][S] u8, events [calls][S] u8, recv [calls][S] the endpoint's last_recv_frame after each
    call, stop_call [S] (-1: none).  Returns dict(start, length, packets, ack, last_acked, pending,
    status, closed_call, max_seen)."""
    calls, S, P = rows.shape
    cols = local_columns(P, local_mask)
    rbits = ~local_mask & ((1 << P) - 1)
    out = dict(start=np.full((calls, S), -1, np.int32), length=np.zeros((calls, S), np.int32),
               packets=np.zeros((calls, S, stride), np.uint8), ack=np.full((calls, S), NULL_FRAME, np.int32),
               last_acked=np.zeros(S, np.int32), pending=np.zeros(S, np.int32), status=np.zeros(S, np.int32),
               closed_call=np.zeros(S, np.int32), max_seen=np.zeros(S, np.int32))
    for s in range(S):
        snd = Sender(len(cols), max_pending)
        last_recv = NULL_FRAME
        for c in range(calls):
            stopped = stop_call is not None and 0 <= stop_call[s] <= c
            push = None
            if pushed[c, s] != NULL_FRAME:
                push = (int(pushed[c, s]), rows[c, s, cols].tobytes())
            start, data = snd.step(c, NULL_FRAME if ack_in is None else int(ack_in[c, s]),
                                   bool(events is not None and events[c, s] & rbits), push,
                                   bool(resend is not None and resend[c, s]), stopped)
            if recv is not None and not stopped:
                last_recv = int(recv[c, s])
            out["start"][c, s], out["length"][c, s], out["ack"][c, s] = start, len(data), last_recv
            out["packets"][c, s, :len(data)] = np.frombuffer(data, np.uint8)
        out["last_acked"][s], out["pending"][s] = snd.last_acked[0], len(snd.pending)
        out["status"][s], out["closed_call"][s], out["max_seen"][s] = snd.status, snd.closed_call, snd.max_seen
    return out


def link_tables(S, calls, seed, max_delay=4, loss=0.25, blackout_every=5, blackout_len=20, tail=0):
    """Per direction: delay [calls][S] in 1..max_delay calls, drop [calls][S] bool -- random loss, a
    blackout of blackout_len calls in every blackout_every-th session (both directions: the caller
    uses one blackout window per session), nothing lost in the last `tail` calls -- and the resend
    flags, set at calls with c % 4 == s % 4."""
    rng = np.random.default_rng(seed)
    delay = rng.integers(1, max_delay + 1, (2, calls, S)).astype(np.int32)
    drop = rng.random((2, calls, S)) < loss
    for s in range(0, S, blackout_every):
        b0 = int(rng.integers(calls // 4, calls // 2))
        drop[:, b0:b0 + blackout_len, s] = True
    if tail:
        drop[:, calls - tail:] = False
        delay[:, calls - tail:] = 1
    resend = (np.arange(calls)[:, None] % 4 == np.arange(S)[None, :] % 4).astype(np.uint8)
    return delay, drop, resend


def route(c, delay, drop, sent_start, sent_ack):
    """What a peer's poll of call c receives from the other's messages of calls < c (one per call: the
    Input packet if any, and ack_frame; the message of call c' arrives at call c' + delay[c'] unless
    dropped): (the call whose packet is taken -- the newest surviving one -- or -1, the newest
    surviving ack_frame).  delay, drop, sent_start, sent_ack: one session's [calls] columns."""
    src, ack = -1, NULL_FRAME
    for c2 in range(max(0, c - 8), c):
        if c2 + delay[c2] == c and not drop[c2]:
            if sent_start[c2] >= 0:
                src = c2
            ack = max(ack, int(sent_ack[c2]))
    return src, ack


class Peer:
    """One side of a session for pair_run: its input rows (the local column its own, the remote
    column filled by its receiver), the session's frame counters (advance_frame's decisions under
    the prediction threshold, as p2p_sched.hip's control pass for a connected two-player session),
    a Sender and a Receiver."""

    def __init__(self, rows, local, max_prediction, max_pending, stride, cap):
        self.rows, self.local, self.mp = rows, local, max_prediction
        self.remote = rows[:, 1 - local:2 - local]  # a view: the receiver writes the rows
        self.recv = F.Receiver(self.remote, max_prediction, max_pending, stride, cap, row_hi=lambda c: c)
        self.snd = Sender(1, max_pending)
        self.cur, self.ll, self.skipped = 0, NULL_FRAME, 0
        calls = rows.shape[0]
        self.start = np.full(calls, -1, np.int32)
        self.ack = np.full(calls, NULL_FRAME, np.int32)
        self.arrive = np.full(calls, NULL_FRAME, np.int32)
        self.data = [b""] * calls
        self.sent = {}  # frame -> the byte sent for it

    def call(self, c, start, data, ack_in, resend):
        _, self.arrive[c] = self.recv.receive(c, start, data)
        confirmed = min(self.ll, self.recv.last)
        lc = min(confirmed, self.cur)
        push = None
        qf = self.cur
        if self.ll == NULL_FRAME or qf == self.ll + 1:
            self.ll = qf
            push = (qf, self.rows[c, self.local:self.local + 1].tobytes())
            self.sent[qf] = push[1]
        if (self.cur if lc == NULL_FRAME else self.cur - lc) < self.mp:
            self.cur += 1
        else:
            self.skipped += 1
        self.start[c], self.data[c] = self.snd.step(c, ack_in, False, push, resend)
        self.ack[c] = self.recv.last


def pair_run(rows_a, rows_b, delay, drop, resend, max_prediction=8, max_pending=64, cap=128):
    """One session between peer A (local player 0) and peer B (local player 1), stepped call by call:
    each call receives what the other emitted earlier (route()), advances, emits.  rows_a / rows_b
    [calls][2] u8 (only the local column is read; the remote one is overwritten), delay / drop
    [2][calls] (direction 0: A -> B), resend [calls].  Returns the two Peers."""
    stride = F.max_packet_bytes(1, max_pending)
    calls = rows_a.shape[0]
    A = Peer(rows_a, 0, max_prediction, max_pending, stride, cap)
    B = Peer(rows_b, 1, max_prediction, max_pending, stride, cap)
    for c in range(calls):
        src_a, ack_a = route(c, delay[1], drop[1], B.start, B.ack)  # B -> A
        src_b, ack_b = route(c, delay[0], drop[0], A.start, A.ack)
        A.call(c, *((B.start[src_a], B.data[src_a]) if src_a >= 0 else (-1, b"")), ack_a, bool(resend[c]))
        B.call(c, *((A.start[src_b], A.data[src_b]) if src_b >= 0 else (-1, b"")), ack_b, bool(resend[c]))
    return A, B
