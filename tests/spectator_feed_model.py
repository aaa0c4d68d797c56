"""Python restatement of the spectator engine's packet feed (ggrs_spectator_set_packet_feed /
receive_packets / read_packet_results, csrc/spectator_ingest.hip, and the kFeed form of
spectator_kernel) over the oracle's wire codec (oracle.codec_encode / codec_decode) and
tests/spectator_model.py's Spectator -- the reference the device feed is compared against.  A helper,
not a test file; it lives here because oracle/ is frozen.

Three pieces, for one session at a time:

A sender: the host's endpoint towards one spectator.  host_upto[c] is the newest confirmed frame the
host has sent by the spectator's call c -- the host's own clock, not bounded by c.  At every call with
something unacknowledged it sends the frames start .. upto with start = acked + 1 - overlap, acked the
receiver's last_recv_frame (UdpProtocol::send_pending_output re-sends everything unacknowledged,
src/network/protocol.rs:450-480), overlap random in 0..3 clipped at frame 0, at most
max_packet_inputs frames, encoded against the host's frame start - 1 (zeros before frame 0).  One
input is all players' bytes in player order.  Damage per (call, session): "truncate", "random"
(random bytes), "withhold", "duplicate" (the previous packet once more), "old_reference" (a start
whose reference the receiver no longer keeps), "gap" (a start past last_recv + 1) and "overlong"
(max_packet_inputs + 1 frames); and packet_feed_model.RECODE's kinds (tests/codec_cases.py's recode: the
same inputs in other bytes, or Some(..) sizes the feed refuses), applied as packet_feed_model.run does.

A receiver: UdpProtocol::on_input (:564-642) as include/ggrs_amd.h restates it for the spectators --
  1. gap: last_recv != NULL and last_recv + 1 < start (the assert!, :588-590), or a first packet with
     start != 0: the session stops at this call with E_PRECONDITION, status STOPPED;
  2. reference: zeros while last_recv == NULL, else frame start - 1 of the session's own rows; older
     than last_recv - 2 max_prediction (:636-639): NO_REFERENCE, a silent drop (the rule and its
     corner at start == 0 are packet_feed_model.Receiver's);
  3. decode, all or nothing: the codec's error code, UNSUPPORTED, or E_CAP past max_packet_inputs;
  4. frames <= last_recv skipped, the later ones stored, last_recv = the packet's last frame; no
     bound by the call;
  5. the call's recv_upto word and ack are last_recv (STOP_WORD from the stopping call on).

The spectators: spectator_model.Spectator stepped over the feed's words, with the per-session window
rule: a launch holds, for session s, the rows (L - cap, L], L the receiver's last_recv when the launch
starts (after every receive queued before it) -- Spectator.call's (row_lo, row_hi) = (L - cap + 1,
L + 1).  A session the feed stopped at call c stops there with E_PRECONDITION.
"""
import functools

import numpy as np

from oracle import oracle as O
from tests import packet_feed_model as PF
from tests import spectator_model as SM

NULL_FRAME = -1
E_PRECONDITION, E_TOO_FAR_BEHIND = SM.E_PRECONDITION, SM.E_TOO_FAR_BEHIND
CODEC_E_CAP, CODEC_E_INVALID, CODEC_UNSUPPORTED = PF.CODEC_E_CAP, PF.CODEC_E_INVALID, PF.CODEC_UNSUPPORTED
NO_REFERENCE, STOPPED = PF.NO_REFERENCE, PF.STOPPED
STOP_WORD = -2 ** 31  # the recv_upto word of a stopped session (kSpecFeedStop)
DAMAGE = ("truncate", "random", "withhold", "duplicate", "old_reference", "gap", "overlong")
max_packet_bytes = PF.max_packet_bytes


class Receiver:
    """One session's endpoint; rows [frames][P] is its recv_inputs (the engine's input rows)."""

    def __init__(self, frames, num_players, max_prediction, max_packet_inputs, stride):
        self.rows = np.zeros((frames, num_players), np.uint8)
        self.P, self.mp, self.W, self.stride = num_players, max_prediction, max_packet_inputs, stride
        self.last = NULL_FRAME
        self.stop_call = None

    def receive(self, c, start, data):
        """-> status"""
        if self.stop_call is not None or start < 0:
            return 0
        last = self.last
        if (start != 0) if last == NULL_FRAME else (last + 1 < start):
            self.stop_call = c
            return STOPPED
        ref = bytes(self.P)
        if last != NULL_FRAME:
            rf = start - 1
            if rf < last - 2 * self.mp:
                return NO_REFERENCE
            if rf >= 0:
                ref = self.rows[rf].tobytes()
        if len(data) > self.stride:
            return CODEC_E_INVALID
        rc, inputs = PF.codec_decode(ref, data)
        if rc < 0:
            return rc
        if any(len(x) != self.P for x in inputs):
            return CODEC_UNSUPPORTED
        if len(inputs) > self.W:
            return CODEC_E_CAP
        lastf = start + len(inputs) - 1
        if not inputs or lastf <= last:
            return 0
        for f in range(max(start, last + 1), lastf + 1):
            self.rows[f] = np.frombuffer(inputs[f - start], np.uint8)
        self.last = lastf
        return 1


def _encode(true_rows, start, upto):
    ref = true_rows[start - 1].tobytes() if start > 0 else bytes(true_rows.shape[1])
    return O.codec_encode(ref, [true_rows[f].tobytes() for f in range(start, upto + 1)])


def run_feed(rows, host_upto, max_prediction=8, max_packet_inputs=64, stride=None, seed=0, damage=None, overlap=True):
    """rows [frames][S][P] u8: the hosts' confirmed inputs; host_upto [calls][S] i32 (non-decreasing, <
    frames - max_packet_inputs - 2).  damage: {(call, session): kind}.  Returns a dict: start, length
    [calls][S] i32 and packets [calls][S][stride] u8 (receive_packets' arguments), status and ack
    [calls][S], recv [calls][S] (the recv_upto words: ack, STOP_WORD from a stopping call on), rows
    [frames][S][P] as the receivers hold them, stop_call [S] (-1: none), applied {(call, session):
    kind} for the damage that took place, stride."""
    frames, S, P = rows.shape
    calls = host_upto.shape[0]
    W, mp = max_packet_inputs, max_prediction
    damage = damage or {}
    if stride is None:
        stride = max_packet_bytes(P, W + 1 if "overlong" in damage.values() else W)
    out = dict(start=np.full((calls, S), -1, np.int32), length=np.zeros((calls, S), np.int32),
               packets=np.zeros((calls, S, stride), np.uint8), status=np.zeros((calls, S), np.int32),
               ack=np.zeros((calls, S), np.int32), recv=np.zeros((calls, S), np.int32),
               rows=np.zeros_like(rows), stop_call=np.full(S, -1, np.int32), applied={}, stride=stride)
    rng = np.random.default_rng(seed)
    for s in range(S):
        true_rows = np.ascontiguousarray(rows[:, s])
        recv = Receiver(frames, P, mp, W, stride)
        prev_packet = None
        for c in range(calls):
            start, data = -1, b""
            if recv.stop_call is None and host_upto[c, s] > recv.last:
                acked = recv.last
                ov = int(rng.integers(0, 4)) if overlap else 0
                start = 0 if acked == NULL_FRAME else max(0, acked + 1 - min(ov, 2 * mp))
                upto = min(int(host_upto[c, s]), start + W - 1)
                kind = damage.get((c, s))
                if kind == "old_reference" and acked - 2 * mp - 1 >= 1:
                    start = acked - 2 * mp - 1 - int(rng.integers(0, 2))
                    upto = min(upto, start + W - 1)
                elif kind == "gap":
                    start = acked + 2
                    upto = max(start, min(upto, start + W - 1))
                elif kind == "overlong":
                    upto = start + W
                elif kind == "old_reference":
                    kind = None
                data = _encode(true_rows, start, upto)
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
                elif kind in PF.RECODE:
                    data, kind = PF.recoded(data, kind, P, stride, (seed, c, s))
                if kind:
                    out["applied"][(c, s)] = kind
                if kind not in ("duplicate", "withhold"):
                    prev_packet = fresh
            assert len(data) <= stride
            out["status"][c, s] = recv.receive(c, start, data)
            out["start"][c, s], out["length"][c, s] = start, len(data)
            out["packets"][c, s, :len(data)] = np.frombuffer(data, np.uint8)
            out["ack"][c, s] = recv.last
            out["recv"][c, s] = recv.last if recv.stop_call is None else STOP_WORD
        out["rows"][:, s] = recv.rows
        if recv.stop_call is not None:
            out["stop_call"][s] = recv.stop_call
    return out


def receive_then_advance(calls, piece):
    """The live loop's launches: receive `piece` calls, advance them, ..."""
    ops = []
    for c0 in range(0, calls, piece):
        n = min(piece, calls - c0)
        ops += [("recv", n), ("adv", n)]
    return ops


def run_spectators(feed, notes, cap, max_frames_behind=10, catchup_speed=1, ops=None):
    """Every session's spectator over the feed's words.  ops: [("recv", n) | ("adv", n)], the order of
    receive_packets and advance_frames (default: everything received, then one launch); cap: the
    engine's input_capacity.  Returns dict(current_frame, last_recv, waited, error [S], states
    [S][state bytes], advanced [calls][S] u8, checksums [calls][S] u16)."""
    calls, S = feed["recv"].shape
    P = feed["rows"].shape[2]
    ops = ops or [("recv", calls), ("adv", calls)]
    out = dict(current_frame=np.zeros(S, np.int32), last_recv=np.zeros(S, np.int32), waited=np.zeros(S, np.int32),
               error=np.zeros(S, np.int32), states=np.zeros((S, 36 + 20 * P), np.uint8),
               advanced=np.zeros((calls, S), np.uint8), checksums=np.zeros((calls, S), np.uint16))
    for s in range(S):
        sp = SM.Spectator(P, max_frames_behind, catchup_speed)
        rows = np.ascontiguousarray(feed["rows"][:, s])
        received = done = 0
        for op, n in ops:
            if op == "recv":
                received += n
                continue
            assert done + n <= received, "advance_frames needs the calls' packets received"
            L = int(feed["ack"][received - 1, s])  # the window: rows (L - cap, L]
            for c in range(done, done + n):
                adv = 0
                if feed["stop_call"][s] == c and not sp.stopped:
                    sp.error = E_PRECONDITION
                elif not sp.stopped:
                    adv = sp.call(int(feed["recv"][c, s]), 0 if notes is None else int(notes[c, s]), rows,
                                  L - cap + 1, L + 1)
                out["advanced"][c, s], out["checksums"][c, s] = adv, sp.checksum
            done += n
        assert done == calls
        out["current_frame"][s], out["last_recv"][s] = sp.current_frame, sp.last_recv
        out["waited"][s], out["error"][s], out["states"][s] = sp.waited, sp.error, sp.state
    return out


def damage_list(host_upto, max_prediction, seed, every=7):
    """One damaged packet in every `every`-th session, the kinds in turn, at the first call from a
    random one in the second quarter of the run where the session's schedule rises (where the sender
    sends)."""
    calls, S = host_upto.shape
    rng = np.random.default_rng(seed)
    damage = {}
    for i, s in enumerate(range(0, S, every)):
        c = int(rng.integers(max(calls // 4, 3 * max_prediction + 8), calls // 2))
        rises = np.nonzero(host_upto[c:, s] > host_upto[c - 1:-1, s])[0]
        if len(rises):
            damage[(c + int(rises[0]), s)] = DAMAGE[i % len(DAMAGE)]
    return damage


def host_inputs(S, frames, P, base):
    """[frames][S][P]: every host's confirmed inputs (oracle.gen_inputs per session)."""
    return np.stack([O.gen_inputs(O.session_seed(s, base), frames, P) for s in range(S)], axis=1)


def clock_schedules(S, calls, seed):
    """host_upto [calls][S] of hosts on their own clocks: session s's host runs (0.5, 1, 1.5)[s % 3]
    frames per call; s % 4 == 1: twice, the network is silent for 12 calls, then everything the host
    produced meanwhile arrives at once (a burst the spectator catches up on); s % 13 == 5: silent for
    70 calls, after which the frames come in full packets, call after call, faster than a spectator
    catches up: it is lost."""
    rng = np.random.default_rng(seed)
    c = np.arange(calls)
    out = np.zeros((calls, S), np.int32)
    for s in range(S):
        rate = (0.5, 1.0, 1.5)[s % 3]
        r = np.floor(rate * (c + 1) + rng.integers(0, 2, calls)).astype(np.int64) - 1
        if s % 4 == 1:
            for t in (40 + s % 9, 120 + s % 11):
                if t + 12 < calls:
                    r[t:t + 12] = r[t - 1]
        if s % 13 == 5 and calls > 130:
            r[50:120] = r[49]
        out[:, s] = np.maximum.accumulate(r)
    return out


# ---- the cases tests/test_spectator_feed_model.py (CPU) and tests/test_gpu_spectator_packets.py share

@functools.lru_cache(maxsize=None)
def parity_case(P, S=130, calls=200, frames=512, W=64):
    """Hosts within one window (input_capacity 512): spectator_model.schedules' networks and notes.
    -> (rows, recv_upto, notes, feed)"""
    rows = host_inputs(S, frames, P, 0x5FEE + P)
    recv, notes = SM.schedules(S, calls, P, 11 + P)
    return rows, recv, notes, run_feed(rows, recv, 8, W, seed=P)


CLOCK = dict(P=2, cap=64, W=32, mp=8, mfb=10, speed=3)


@functools.lru_cache(maxsize=None)
def clock_case(S=130, calls=200):
    """Hosts on different clocks over input_capacity 64.  -> (rows, host_upto, feed)"""
    k = CLOCK
    rows = host_inputs(S, 2 * calls, k["P"], 0xC10C)
    host_upto = clock_schedules(S, calls, 3)
    return rows, host_upto, run_feed(rows, host_upto, k["mp"], k["W"], seed=17)


DAMAGED = dict(P=2, cap=256, W=24, mp=8, mfb=10, speed=3)
RECODED = dict(P=2, cap=512, W=24, mp=8, mfb=10, speed=3)


@functools.lru_cache(maxsize=None)
def damage_case(S=130, calls=200, seed=5):
    """One damaged packet in every 7th session.  -> (rows, host_upto, damage, feed)"""
    k = DAMAGED
    rows = host_inputs(S, calls + 64, k["P"], 0xD4A)
    host_upto = np.stack([O.stall_schedule(calls, k["mp"], seed * 1000 + s, stall_every=40 if s % 2 else 10 ** 9)
                          for s in range(S)], axis=1).astype(np.int32)
    damage = damage_list(host_upto, k["mp"], seed)
    return rows, host_upto, damage, run_feed(rows, host_upto, k["mp"], k["W"], seed=9, damage=damage)


@functools.lru_cache(maxsize=None)
def recode_case(S=66, calls=160, seed=4):
    """One of packet_feed_model.RECODE's kinds in every 3rd session, at several of its calls; the hosts
    stay within one window, so a table-fed engine can hold the same rows.
    -> (rows, host_upto, damage, feed, the feed of the same packets as the sender encoded them)"""
    k = RECODED
    rows = host_inputs(S, calls + 64, k["P"], 0x4EC0)
    host_upto = np.stack([O.stall_schedule(calls, k["mp"], seed * 1000 + s, stall_every=40 if s % 2 else 10 ** 9)
                          for s in range(S)], axis=1).astype(np.int32)
    damage = PF.recode_list(host_upto, seed)
    return (rows, host_upto, damage, run_feed(rows, host_upto, k["mp"], k["W"], seed=21, damage=damage),
            run_feed(rows, host_upto, k["mp"], k["W"], seed=21))
