"""Python restatement of the P2P engine's packet feed (ggrs_p2p_set_packet_feed / receive_packets,
csrc/p2p_ingest.hip) over the oracle's wire codec (oracle.codec_encode / codec_decode) -- the
reference the device feed is compared against.  A helper, not a test file; it lives here because
oracle/ is frozen.

Two pieces, stepped together call by call for one session at a time:

A sender.  For a schedule (rows, arrive) it sends a packet at every call where `arrive` rises: the
frames start .. arrive[c] with start = acked + 1 - overlap, where acked is the receiver's
last_recv_frame (UdpProtocol::send_pending_output re-sends everything unacknowledged,
src/network/protocol.rs:450-480) and overlap is random in 0..3, clipped at frame 0 and at the
receiver's 2 max_prediction retention; at most max_packet_inputs frames.  The packet is encoded
against the true remote bytes of frame start - 1 (zeros before frame 0).  Damage per (call,
session): "truncate", "random" (random bytes), "withhold", "duplicate" (the previous packet once
more), "old_reference" (a start whose reference the receiver no longer keeps), "gap" (a start past
last_recv + 1), "ahead" (frames beyond the call) and "overlong" (max_packet_inputs + 1 frames); and the
kinds of tests/codec_cases.py's recode (RECODE): the same inputs in other bytes -- runs split, zero-length
runs, padded varints, input_sizes = Some(zero deltas), bytes after the stream -- which deliver as the
packet would have, and Some(..) with uneven or negative sizes over the same stream, which are dropped
with UNSUPPORTED / E_DELTA.  A recoded packet that outgrows the stride goes out as it was.

A receiver: UdpProtocol::on_input (:564-642) as include/ggrs_amd.h restates it --
  1. gap: last_recv != NULL and last_recv + 1 < start (the assert!, :588-590), or a first packet with
     start != 0: the session stops at this call with E_PRECONDITION;
  2. reference: zeros while last_recv == NULL, else frame start - 1 from the rows; older than
     last_recv - 2 max_prediction (:636-639): NO_REFERENCE, a silent drop; kept but its row slot
     holds another frame: stop, E_PRECONDITION;
  3. decode, all or nothing: the codec's error code, UNSUPPORTED, or E_CAP past max_packet_inputs;
  4. frames <= last_recv skipped; a last frame beyond the call stops with E_INVALID; a frame whose
     row slot holds another frame stops with E_PRECONDITION; else the bytes go into the rows;
  5. arrive[c] = last_recv (a stopping call: a frame after the call -- the packet's last one, or
     c + 1 -- which is how the arrival table stops a session at a call).
"""
import ctypes

import numpy as np

from oracle import oracle as O
from tests import codec_cases as C

NULL_FRAME = -1
E_INVALID, E_PRECONDITION = -1, -2
CODEC_E_CAP, CODEC_E_INVALID, CODEC_UNSUPPORTED = -4, -5, -6
NO_REFERENCE, STOPPED = -16, -17
DAMAGE = ("truncate", "random", "withhold", "duplicate", "old_reference", "gap")
RECODE = C.ACCEPTING + C.REJECTING  # applied only where a caller's damage dict names them


def max_packet_bytes(B, W):
    """ggrs_codec_max_packet_bytes"""
    L = B * W
    return (1 + 8 + L + (L + 1) // 2 + 10 + 15) // 16 * 16


def remote_columns(num_players, local_mask):
    return [k for k in range(num_players) if not (local_mask >> k) & 1]


_scratch = {}


def codec_decode(reference, data, max_inputs=1 << 16):
    """oracle.codec_decode (oracle_codec_decode, the same capacities) with its output buffers kept
    between calls: allocating 16 MB per packet is most of that function's time."""
    L = O.lib()
    O._codec_bind(L)
    if not _scratch:
        _scratch.update(out=np.zeros(1 << 24, np.uint8), lens=np.zeros(max_inputs, np.int32))
    out, lens = _scratch["out"], _scratch["lens"]
    ref, d = O._u8(reference), O._u8(data)
    n = ctypes.c_int32()
    rc = L.oracle_codec_decode(O._ptr(ref, ctypes.c_uint8), len(reference), O._ptr(d, ctypes.c_uint8), len(data),
                               O._ptr(out, ctypes.c_uint8), out.size, O._ptr(lens, ctypes.c_int32), lens.size,
                               ctypes.byref(n))
    if rc != 0:
        return rc, None
    ends = np.cumsum(lens[:n.value])
    return 0, [out[e - k:e].tobytes() for e, k in zip(ends, lens[:n.value])]


class Receiver:
    """One session's endpoint.  `remote` [frames][B] is its view of the input rows' remote columns
    (recv_inputs); row_hi(c) the newest row added when call c's packet is received, `cap` the rows'
    ring length."""

    def __init__(self, remote, max_prediction, max_packet_inputs, stride, cap=None, row_hi=None):
        self.remote, self.mp, self.W, self.stride = remote, max_prediction, max_packet_inputs, stride
        self.B = remote.shape[1]
        self.cap = cap if cap is not None else 1 << 30
        self.row_hi = row_hi if row_hi is not None else (lambda c: remote.shape[0] - 1)
        self.last = NULL_FRAME
        self.stop_call, self.error = None, 0

    def held(self, f, c):
        hi = self.row_hi(c)
        return hi - self.cap < f <= hi

    def _stop(self, c, error, marker):
        self.stop_call, self.error = c, error
        return STOPPED, marker

    def receive(self, c, start, data):
        """-> (status, arrive[c])"""
        if self.stop_call is not None or start < 0:
            return 0, self.last
        last = self.last
        if (start != 0) if last == NULL_FRAME else (last + 1 < start):
            return self._stop(c, E_PRECONDITION, c + 1)
        ref = bytes(self.B)
        if last != NULL_FRAME:
            rf = start - 1
            if rf < last - 2 * self.mp:
                return NO_REFERENCE, last
            if rf >= 0:
                if not self.held(rf, c):
                    return self._stop(c, E_PRECONDITION, c + 1)
                ref = self.remote[rf].tobytes()
        if len(data) > self.stride:
            return CODEC_E_INVALID, last
        rc, inputs = codec_decode(ref, data)
        if rc < 0:
            return rc, last
        if any(len(x) != self.B for x in inputs):
            return CODEC_UNSUPPORTED, last
        if len(inputs) > self.W:
            return CODEC_E_CAP, last
        lastf = start + len(inputs) - 1
        if not inputs or lastf <= last:
            return 0, last
        if lastf > c:
            return self._stop(c, E_INVALID, lastf)
        first = max(start, last + 1)
        if not all(self.held(f, c) for f in range(first, lastf + 1)):
            return self._stop(c, E_PRECONDITION, c + 1)
        for f in range(first, lastf + 1):
            self.remote[f] = np.frombuffer(inputs[f - start], np.uint8)
        self.last = lastf
        return 1, lastf


def _encode(true_remote, start, upto):
    ref = true_remote[start - 1].tobytes() if start > 0 else bytes(true_remote.shape[1])
    return O.codec_encode(ref, [true_remote[f].tobytes() for f in range(start, upto + 1)])


def run(rows, arrive, local_mask, max_prediction, max_packet_inputs=64, stride=None, seed=0, damage=None,
        cap=None, row_hi=None, overlap=True):
    """rows [calls][S][P] u8, arrive [calls][S] i32 (non-decreasing, <= the call).  damage: {(call,
    session): kind}.  Returns a dict: start, length [calls][S] i32 and packets [calls][S][stride] u8
    (receive_packets' arguments), arrive (the effective table), rows (the rows as the receiver holds
    them: the up-front engine's input), status and ack [calls][S], stop_call [S] (-1: none) and
    error [S], and applied: {(call, session): kind} for the damage that took place."""
    calls, S, P = rows.shape
    cols = remote_columns(P, local_mask)
    B, W, mp = len(cols), max_packet_inputs, max_prediction
    stride = stride or max_packet_bytes(B, W)
    damage = damage or {}
    out = dict(start=np.full((calls, S), -1, np.int32), length=np.zeros((calls, S), np.int32),
               packets=np.zeros((calls, S, stride), np.uint8), arrive=np.zeros((calls, S), np.int32),
               rows=rows.copy(), status=np.zeros((calls, S), np.int32), ack=np.zeros((calls, S), np.int32),
               stop_call=np.full(S, -1, np.int32), error=np.zeros(S, np.int32), applied={}, stride=stride)
    rng = np.random.default_rng(seed)
    for s in range(S):
        true_remote = np.ascontiguousarray(rows[:, s, cols])
        recv = Receiver(true_remote.copy(), mp, W, stride, cap, row_hi)
        prev_packet, sent_upto = None, NULL_FRAME
        for c in range(calls):
            start, data = -1, b""
            if recv.stop_call is None and arrive[c, s] > sent_upto:
                sent_upto = int(arrive[c, s])
                acked = recv.last
                ov = int(rng.integers(0, 4)) if overlap else 0
                start = 0 if acked == NULL_FRAME else max(0, acked + 1 - min(ov, 2 * mp))
                upto = min(sent_upto, start + W - 1)
                kind = damage.get((c, s))
                if kind == "old_reference" and acked - 2 * mp - 1 >= 1:
                    start = acked - 2 * mp - 1 - int(rng.integers(0, 2))
                    upto = min(upto, start + W - 1)
                elif kind == "gap":
                    start = acked + 2
                    upto = max(start, min(upto, c))
                    upto = min(upto, calls - 1)
                elif kind == "ahead" and c + 1 < calls:
                    upto = c + 1
                elif kind == "overlong" and sent_upto >= start + W:
                    upto = start + W
                elif kind in ("old_reference", "ahead", "overlong"):
                    kind = None
                data = _encode(true_remote, start, upto)
                fresh = (start, data)
                if kind == "truncate":
                    data = data[:int(rng.integers(0, len(data)))]
                elif kind == "random":
                    data = rng.integers(0, 256, int(rng.integers(1, stride + 1)), dtype=np.uint8).tobytes()
                elif kind == "withhold":
                    start, data = -1, b""
                elif kind == "duplicate":
                    if prev_packet is None:
                        kind = None
                    else:
                        start, data = prev_packet
                elif kind in RECODE:
                    data, kind = recoded(data, kind, B, stride, (seed, c, s))
                if kind:
                    out["applied"][(c, s)] = kind
                if kind not in ("duplicate", "withhold"):
                    prev_packet = fresh
            assert len(data) <= stride
            status, arr = recv.receive(c, start, data)
            out["start"][c, s], out["length"][c, s] = start, len(data)
            out["packets"][c, s, :len(data)] = np.frombuffer(data, np.uint8)
            out["status"][c, s], out["arrive"][c, s], out["ack"][c, s] = status, arr, recv.last
        out["rows"][:, s, cols] = recv.remote
        if recv.stop_call is not None:
            out["stop_call"][s], out["error"][s] = recv.stop_call, recv.error
    return out


def recoded(data, kind, B, stride, key):
    """codec_cases.recode with a generator of its own (the sender's random overlaps stay what they are
    without it): -> (bytes, kind), or (data, None) where the kind has no other form of this packet
    within the stride."""
    new = C.recode(data, kind, np.random.default_rng(list(key)), B)
    return (data, None) if new is None or new == data or len(new) > stride else (new, kind)


def recode_list(arrive, seed, every=3, per_session=5):
    """One kind of RECODE per `every`-th session, the kinds in turn, at `per_session` of the calls where
    the session's schedule rises (where the sender sends)."""
    calls, S = arrive.shape
    rng = np.random.default_rng(seed)
    damage = {}
    for i, s in enumerate(range(0, S, every)):
        rises = np.nonzero(arrive[1:, s] > arrive[:-1, s])[0] + 1
        for c in rng.choice(rises, min(per_session, len(rises)), replace=False):
            damage[(int(c), s)] = RECODE[i % len(RECODE)]
    return damage


def recode_case(P, local_mask, S=66, calls=160, max_prediction=8, seed=3):
    """The recode tests' inputs (tests/test_packet_feed_model.py on the CPU, tests/test_gpu_p2p_packets.py
    on the device): rows, a schedule per session (stalls with bursts, jitter), the recode list."""
    rows = np.stack([O.gen_inputs(O.session_seed(s, 0x4EC0 + P), calls, P, 1) for s in range(S)], axis=1)
    arrive = np.stack([O.stall_schedule(calls, max_prediction, seed * 1000 + s, stall_every=40 if s % 2 else 10 ** 9)
                       for s in range(S)], axis=1).astype(np.int32)
    return rows, arrive, recode_list(arrive, seed)


def damage_list(arrive, max_prediction, seed, every=7):
    """One damaged packet in every `every`-th session, the kinds in turn (DAMAGE and "ahead"), at the
    first call from a random one in the second quarter of the run where the session's schedule
    rises (where the sender sends)."""
    calls, S = arrive.shape
    kinds = DAMAGE + ("ahead",)
    rng = np.random.default_rng(seed)
    damage = {}
    for i, s in enumerate(range(0, S, every)):
        c = int(rng.integers(max(calls // 4, 3 * max_prediction + 8), calls // 2))
        rises = np.nonzero(arrive[c:, s] > arrive[c - 1:-1, s])[0]
        if len(rises):
            damage[(c + int(rises[0]), s)] = kinds[i % len(kinds)]
    return damage


def damage_case(S=130, calls=200, P=2, local_mask=0b01, max_prediction=8, seed=5):
    """The damage test's inputs (tests/test_packet_feed_model.py on the CPU, tests/test_gpu_p2p_packets.py
    on the device): rows, a schedule per session (stalls with bursts, jitter), the damage list."""
    rows = np.stack([O.gen_inputs(O.session_seed(s, 0xD4A), calls, P, 1) for s in range(S)], axis=1)
    arrive = np.stack([O.stall_schedule(calls, max_prediction, seed * 1000 + s, stall_every=40 if s % 2 else 10 ** 9)
                       for s in range(S)], axis=1).astype(np.int32)
    return rows, arrive, damage_list(arrive, max_prediction, seed)
