"""P2P rollback decision over the engine's C ABI (include/ggrs_amd.h, ggrs_p2p_*).

One P2PEngine holds S sessions of one peer.  Each call of advance_frames(n) runs n x
P2PSession::advance_frame (src/sessions/p2p_session.rs:265-426) + the ex_game handler for every
session: the remote players' inputs of frame f - remote_latency arrive, mispredictions found by
InputQueue (src/input_queue.rs:190-230) roll the session back (adjust_gamestate, :658-714), the
current frame is saved and advanced with synchronized inputs (remote players predicted,
src/lib.rs:390-406).  The device decides per session whether and how far to roll back.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import InvalidRequest

PREDICT_REPEAT_LAST, PREDICT_DEFAULT = 0, 1


class P2PConfig(ctypes.Structure):
    _fields_ = [
        ("num_sessions", ctypes.c_int32),
        ("num_players", ctypes.c_int32),
        ("local_mask", ctypes.c_int32),
        ("input_delay", ctypes.c_int32),
        ("max_prediction", ctypes.c_int32),
        ("remote_latency", ctypes.c_int32),
        ("predictor", ctypes.c_int32),
        ("input_capacity", ctypes.c_int32),
        ("trace_capacity", ctypes.c_int32),
        ("device", ctypes.c_int32),
    ]


_bound = False


def _bind(L):
    global _bound
    if _bound:
        return
    vp = ctypes.c_void_p
    P = ctypes.POINTER
    i32 = ctypes.c_int32
    L.ggrs_p2p_engine_create.argtypes = [P(P2PConfig), P(vp)]
    L.ggrs_p2p_engine_destroy.argtypes = [vp]
    L.ggrs_p2p_engine_config.argtypes = [vp, P(P2PConfig)]
    L.ggrs_p2p_add_inputs.argtypes = [vp, i32, i32, vp]
    L.ggrs_p2p_advance_frames.argtypes = [vp, i32]
    L.ggrs_p2p_current_frame.argtypes = [vp, P(i32)]
    L.ggrs_p2p_calls.argtypes = [vp, P(i32)]
    L.ggrs_p2p_synchronize.argtypes = [vp]
    L.ggrs_p2p_read_state.argtypes = [vp, i32, vp]
    L.ggrs_p2p_read_states.argtypes = [vp, vp]
    L.ggrs_p2p_read_ring.argtypes = [vp, i32, vp, vp, vp]
    L.ggrs_p2p_read_stats.argtypes = [vp, vp, vp]
    L.ggrs_p2p_read_queues.argtypes = [vp, vp]
    L.ggrs_p2p_read_trace.argtypes = [vp, i32, i32, vp]
    L.ggrs_p2p_timing_reset.argtypes = [vp]
    L.ggrs_p2p_timing_stop.argtypes = [vp]
    L.ggrs_p2p_timing_read.argtypes = [vp, P(ctypes.c_float), P(i32)]
    L.ggrs_p2p_set_desync_detection.argtypes = [vp, i32]
    L.ggrs_p2p_local_checksums.argtypes = [vp, i32, vp, i32]
    L.ggrs_p2p_compare_checksums.argtypes = [vp, i32, vp, i32, vp, P(i32)]
    L.ggrs_p2p_debug_desync.argtypes = [vp, i32, i32]
    L.ggrs_p2p_set_sparse_saving.argtypes = [vp, i32]
    L.ggrs_p2p_set_unstaged.argtypes = [vp, i32]
    L.ggrs_p2p_set_arrival_schedule.argtypes = [vp, i32]
    L.ggrs_p2p_add_arrivals.argtypes = [vp, i32, i32, vp, vp]
    L.ggrs_p2p_add_peer_reports.argtypes = [vp, i32, i32, vp]
    L.ggrs_p2p_read_sessions.argtypes = [vp, vp, vp, vp]
    L.ggrs_p2p_read_reports.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.ggrs_p2p_set_packet_feed.argtypes = [vp, i32, i32]
    L.ggrs_p2p_receive_packets.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32]
    L.ggrs_p2p_read_packet_results.argtypes = [vp, i32, i32, vp, vp]
    L.ggrs_p2p_set_packet_emit.argtypes = [vp, i32, i32]
    L.ggrs_p2p_emit_packets.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
    L.ggrs_p2p_read_emit_state.argtypes = [vp, vp, vp, vp, vp]
    L.ggrs_p2p_set_spectator_emit.argtypes = [vp, i32, i32, i32]
    L.ggrs_p2p_emit_spectator_packets.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
    L.ggrs_p2p_read_spectator_emit_state.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ggrs_p2p_set_time_sync.argtypes = [vp, i32]
    L.ggrs_p2p_time_sync.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, i32]
    L.ggrs_p2p_read_time_sync_state.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ggrs_p2p_set_desync_compare.argtypes = [vp, i32]
    L.ggrs_p2p_add_remote_reports.argtypes = [vp, i32, i32, vp, vp, vp, i32]
    L.ggrs_p2p_add_remote_reports_from.argtypes = [vp, vp, i32, i32]
    L.ggrs_p2p_compare_reports.argtypes = [vp, i32, i32, P(i32)]
    L.ggrs_p2p_read_desync_events.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, P(i32)]
    L.ggrs_p2p_read_desync_state.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    u64 = ctypes.c_uint64
    L.ggrs_p2p_set_endpoint_poll.argtypes = [vp, u64, u64, u64]
    L.ggrs_p2p_poll_endpoints.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
    L.ggrs_p2p_read_endpoint_state.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.ggrs_p2p_set_spectator_poll.argtypes = [vp, u64, u64, u64]
    L.ggrs_p2p_poll_spectator_endpoints.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
    L.ggrs_p2p_read_spectator_endpoint_state.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.ggrs_p2p_set_event_queue.argtypes = [vp, i32]
    L.ggrs_p2p_collect_events.argtypes = [vp, i32, i32] + [vp] * 6 + [i32] + [vp] * 5 + [i32]
    L.ggrs_p2p_drain_events.argtypes = [vp, i32, vp, vp, P(i32), P(i32), i32]
    L.ggrs_p2p_read_event_queue_state.argtypes = [vp, vp, vp, vp, vp, vp]
    for name in _lib.EXPORTS:
        if name.startswith("ggrs_p2p_"):
            getattr(L, name).restype = ctypes.c_int
    _bound = True


def peer_report(player, reporter, frame):
    """GGRS_PEER_REPORT: remote player `reporter`'s endpoint reports remote player `player`
    disconnected with last frame `frame`."""
    return 16 | player | reporter << 2 | (frame + 1) << 5


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class P2PEngine:
    """S sessions of one peer: local players `local_players`, every other player remote."""

    def __init__(self, num_sessions, num_players=2, local_players=(0,), input_delay=0,
                 max_prediction=8, remote_latency=4, predictor=PREDICT_REPEAT_LAST,
                 input_capacity=0, trace_capacity=0, device=0):
        self._L = _lib.lib()
        _bind(self._L)
        mask = 0
        for p in local_players:
            mask |= 1 << p
        cfg = P2PConfig(num_sessions, num_players, mask, input_delay, max_prediction, remote_latency,
                        predictor, input_capacity, trace_capacity, device)
        h = ctypes.c_void_p()
        _lib.check(self._L.ggrs_p2p_engine_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.num_sessions, self.num_players, self.local_mask = num_sessions, num_players, mask
        self.input_delay, self.max_prediction = input_delay, max_prediction
        self.remote_latency, self.predictor = remote_latency, predictor
        self.ring_len = max_prediction + 1
        self.state_bytes = 36 + 20 * num_players

    def close(self):
        if getattr(self, "_h", None):
            self._L.ggrs_p2p_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_inputs(self, first_frame, inputs):
        """inputs [n][S][P]: row g = local players' add_local_input of call g, remote players'
        input of frame g."""
        a = np.ascontiguousarray(inputs, np.uint8)
        if a.ndim != 3 or a.shape[1:] != (self.num_sessions, self.num_players):
            raise InvalidRequest(-1, f"inputs must be [n][{self.num_sessions}][{self.num_players}]")
        _lib.check(self._L.ggrs_p2p_add_inputs(self._h, first_frame, a.shape[0], _vp(a)))

    def advance_frames(self, n=1):
        _lib.check(self._L.ggrs_p2p_advance_frames(self._h, n))

    def current_frame(self):
        v = ctypes.c_int32()
        _lib.check(self._L.ggrs_p2p_current_frame(self._h, ctypes.byref(v)))
        return v.value

    def calls(self):
        """advance_frame calls made (current_frame() is the session's frame: the same in rollback
        mode, behind it in lockstep mode)."""
        v = ctypes.c_int32()
        _lib.check(self._L.ggrs_p2p_calls(self._h, ctypes.byref(v)))
        return v.value

    def synchronize(self):
        _lib.check(self._L.ggrs_p2p_synchronize(self._h))

    def state(self, session):
        out = np.zeros(self.state_bytes, np.uint8)
        _lib.check(self._L.ggrs_p2p_read_state(self._h, session, _vp(out)))
        return out

    def states(self):
        """state(session) for every session, one transfer: [num_sessions][state_bytes]."""
        out = np.zeros((self.num_sessions, self.state_bytes), np.uint8)
        _lib.check(self._L.ggrs_p2p_read_states(self._h, _vp(out)))
        return out

    def ring(self, session):
        frames = np.zeros(self.ring_len, np.int32)
        cks = np.zeros(self.ring_len, np.uint16)
        states = np.zeros((self.ring_len, self.state_bytes), np.uint8)
        _lib.check(self._L.ggrs_p2p_read_ring(self._h, session, _vp(frames), _vp(cks), _vp(states)))
        return frames, cks, states

    def queues(self):
        """[4][P][S] int32: every session's InputQueue prediction frame, prediction input, first
        incorrect frame and last requested frame."""
        out = np.zeros((4, self.num_players, self.num_sessions), np.int32)
        _lib.check(self._L.ggrs_p2p_read_queues(self._h, _vp(out)))
        return out

    def stats(self):
        rb = np.zeros(self.num_sessions, np.int32)
        rs = np.zeros(self.num_sessions, np.int64)
        _lib.check(self._L.ggrs_p2p_read_stats(self._h, _vp(rb), _vp(rs)))
        return rb, rs

    def trace(self, first_frame, n):
        out = np.zeros((n, self.num_sessions), np.uint16)
        _lib.check(self._L.ggrs_p2p_read_trace(self._h, first_frame, n, _vp(out)))
        return out

    def timing_reset(self):
        _lib.check(self._L.ggrs_p2p_timing_reset(self._h))

    def timing_stop(self):
        """Record the span's end behind the last launch without waiting (timing_read reports it)."""
        _lib.check(self._L.ggrs_p2p_timing_stop(self._h))

    def timing_read(self):
        ms, n = ctypes.c_float(), ctypes.c_int32()
        _lib.check(self._L.ggrs_p2p_timing_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    # ---- desync detection (include/ggrs_amd.h, ggrs_p2p_*_desync*/checksums)
    def set_desync_detection(self, interval):
        """DesyncDetection::On{interval} (0 = Off) for every session; before the first call."""
        _lib.check(self._L.ggrs_p2p_set_desync_detection(self._h, interval))
        self.desync_interval = interval

    def local_checksums(self, frame, out=None):
        """This peer's checksum report of `frame` for every session: numpy [S] u16, or into a
        device tensor `out` (torch, uint16/int16, S elements)."""
        if out is not None and hasattr(out, "data_ptr"):
            _lib.check(self._L.ggrs_p2p_local_checksums(self._h, frame, ctypes.c_void_p(out.data_ptr()), 1))
            return out
        a = np.zeros(self.num_sessions, np.uint16)
        _lib.check(self._L.ggrs_p2p_local_checksums(self._h, frame, _vp(a), 0))
        return a

    def compare_checksums(self, frame, remote):
        """Sessions whose local report of `frame` differs from `remote` ([S] u16 numpy, or a device
        tensor): numpy array of session indices (compared on the device)."""
        words = np.zeros((self.num_sessions + 63) // 64, np.uint64)
        n = ctypes.c_int32()
        if hasattr(remote, "data_ptr"):
            ptr, dev = ctypes.c_void_p(remote.data_ptr()), 1
        else:
            remote = np.ascontiguousarray(remote, np.uint16)
            ptr, dev = _vp(remote), 0
        _lib.check(self._L.ggrs_p2p_compare_checksums(self._h, frame, ptr, dev, _vp(words), ctypes.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.int64)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.num_sessions]
        return np.nonzero(bits)[0]

    def debug_desync(self, session, frame):
        """Test hook: session's AdvanceFrame from `frame` flips a bit, on every (re)simulation."""
        _lib.check(self._L.ggrs_p2p_debug_desync(self._h, session, frame))

    def set_sparse_saving(self, on=True):
        """SessionBuilder::with_sparse_saving_mode for every session; before the first call."""
        _lib.check(self._L.ggrs_p2p_set_sparse_saving(self._h, int(bool(on))))
        self.sparse_saving = bool(on)

    # ---- arrival schedules (include/ggrs_amd.h, ggrs_p2p_*arrival*; p2p_sched.hip)
    def set_arrival_schedule(self, on=True):
        """Per-session remote-arrival tables instead of the fixed remote_latency (before the first
        call): each session rolls back to its own earliest misprediction, stops advancing at the
        prediction threshold (p2p_session.rs:393-423), and handles disconnects (:618-655)."""
        _lib.check(self._L.ggrs_p2p_set_arrival_schedule(self._h, int(bool(on))))
        self.arrival_schedule = bool(on)

    def add_arrivals(self, first_call, arrive_upto, events=None):
        """arrive_upto [n][S] int32: the newest remote frame each session's poll delivered at calls
        first_call .. first_call + n - 1; events [n][S] uint8 (bit k: Event::Disconnected for
        remote player k at that call, after its arrivals) or None."""
        a = np.ascontiguousarray(arrive_upto, np.int32)
        if a.ndim != 2 or a.shape[1] != self.num_sessions:
            raise InvalidRequest(-1, f"arrive_upto must be [n][{self.num_sessions}]")
        ev = None
        if events is not None:
            ev = np.ascontiguousarray(events, np.uint8)
            if ev.shape != a.shape:
                raise InvalidRequest(-1, "events must have arrive_upto's shape")
        _lib.check(self._L.ggrs_p2p_add_arrivals(self._h, first_call, a.shape[0], _vp(a), _vp(ev)))

    def add_peer_reports(self, first_call, reports):
        """reports [n][S] int32 (peer_report(player, reporter, frame) or 0): the peers' disconnect
        reports received by calls first_call .. first_call + n - 1 (after their add_arrivals); each
        stands until its reporter disconnects (update_player_disconnects, p2p_session.rs:748-783)."""
        r = np.ascontiguousarray(reports, np.int32)
        if r.ndim != 2 or r.shape[1] != self.num_sessions:
            raise InvalidRequest(-1, f"reports must be [n][{self.num_sessions}]")
        _lib.check(self._L.ggrs_p2p_add_peer_reports(self._h, first_call, r.shape[0], _vp(r)))

    def sessions(self):
        """(frames, skipped, errors) [S] int32 each: every session's current frame, its calls that
        did not advance (prediction threshold), and its error (0, or where the reference panics)."""
        out = [np.zeros(self.num_sessions, np.int32) for _ in range(3)]
        _lib.check(self._L.ggrs_p2p_read_sessions(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    def reports(self, first_call, n_calls):
        """Desync detection under arrival schedules: dict of [n][S] arrays for calls first_call ..
        first_call + n - 1 -- frame (the checksum report check_checksum_send_interval sent, -1
        none), checksum, last_confirmed (the frame compare_local_checksums_against_peers compared
        against) and local_last (the local players' last queued frame after the call)."""
        shape = (n_calls, self.num_sessions)
        out = dict(frame=np.zeros(shape, np.int32), checksum=np.zeros(shape, np.uint16),
                   last_confirmed=np.zeros(shape, np.int32), local_last=np.zeros(shape, np.int32))
        _lib.check(self._L.ggrs_p2p_read_reports(self._h, first_call, n_calls, _vp(out["frame"]),
                                                  _vp(out["checksum"]), _vp(out["last_confirmed"]),
                                                  _vp(out["local_last"])))
        return out

    # ---- packet feed (include/ggrs_amd.h, ggrs_p2p_*packet*; p2p_ingest.hip)
    def set_packet_feed(self, max_packet_inputs=64, packet_stride=None):
        """The remote inputs enter as the wire packets each call's poll received (receive_packets)
        instead of as rows known in advance; after set_arrival_schedule, before the first call.
        packet_stride defaults to codec.max_packet_bytes(remote players, max_packet_inputs)."""
        remote = self.num_players - bin(self.local_mask).count("1")
        if packet_stride is None:
            packet_stride = int(self._L.ggrs_codec_max_packet_bytes(max(remote, 1), max_packet_inputs))
        _lib.check(self._L.ggrs_p2p_set_packet_feed(self._h, max_packet_inputs, packet_stride))
        self.max_packet_inputs, self.packet_stride, self.remote_players = max_packet_inputs, packet_stride, remote

    def receive_packets(self, first_call, start_frame, packet_len, packets, events=None):
        """The packets polled by calls first_call .. first_call + n - 1 (their input rows already
        added): start_frame [n][S] int32 (negative: no packet), packet_len [n][S] int32, packets
        [n][S][packet_stride] uint8, events [n][S] uint8 or None (add_arrivals' events) -- numpy
        arrays, or torch tensors on the engine's device (read in place by the launch)."""
        n, S = int(start_frame.shape[0]), self.num_sessions
        stride = getattr(self, "packet_stride", None) or int(packets.shape[-1])
        dev = hasattr(packets, "data_ptr")
        ptrs, keep = _lib.marshal((start_frame, packet_len, packets, events), ((n, S), (n, S), (n, S, stride), (n, S)),
                                  ("int32", "int32", "uint8", "uint8"), dev)
        _lib.check(self._L.ggrs_p2p_receive_packets(self._h, first_call, n, *ptrs, int(dev)))

    def packet_results(self, first_call, n_calls):
        """(status, ack_frame) [n][S] int32 for received calls among the last input_capacity: status 1
        delivered new frames, 0 no packet / nothing new, a GGRS_CODEC_* code, GGRS_PACKET_NO_REFERENCE
        or GGRS_PACKET_STOPPED; ack_frame the endpoint's last_recv_frame after the call."""
        status = np.zeros((n_calls, self.num_sessions), np.int32)
        ack = np.zeros((n_calls, self.num_sessions), np.int32)
        _lib.check(self._L.ggrs_p2p_read_packet_results(self._h, first_call, n_calls, _vp(status), _vp(ack)))
        return status, ack

    # ---- packet emit (include/ggrs_amd.h, ggrs_p2p_*emit*; p2p_emit.hip)
    def set_packet_emit(self, max_pending_inputs=64, out_stride=None):
        """The sessions' outgoing Input message bodies are built on the device (emit_packets); after
        set_arrival_schedule, before the first call.  out_stride defaults to
        codec.max_packet_bytes(local players, max_pending_inputs)."""
        local = bin(self.local_mask).count("1")
        if out_stride is None:
            out_stride = int(self._L.ggrs_codec_max_packet_bytes(max(local, 1), max_pending_inputs))
        _lib.check(self._L.ggrs_p2p_set_packet_emit(self._h, max_pending_inputs, out_stride))
        self.max_pending_inputs, self.out_stride, self.local_players = max_pending_inputs, out_stride, local

    def emit_packets(self, first_call, n_calls, ack_in=None, resend=None, out=None):
        """The packets sent by calls first_call .. first_call + n_calls - 1 (already run, emitted in
        order, each once): ack_in [n][S] int32 (the newest ack_frame each call's poll received,
        NULL_FRAME none) and resend [n][S] uint8 (the retry timer fired) or None.  Returns
        (start_frame [n][S] int32, -1 no packet; packet_len [n][S] int32; ack_frame [n][S] int32;
        packets [n][S][out_stride] uint8) as numpy arrays -- or, with out = such a tuple of torch
        tensors on the engine's device (ack_in and resend then device tensors too), fills and returns
        them; the launch runs on the engine's stream (synchronize() before another stream reads)."""
        n, S = int(n_calls), self.num_sessions
        stride = getattr(self, "out_stride", None)
        if stride is None:
            _lib.check(self._L.ggrs_p2p_emit_packets(self._h, first_call, n, None, None, None, None, None, None, 0))
        shapes = ((n, S), (n, S), (n, S), (n, S), (n, S), (n, S, stride))
        return self._emit(self._L.ggrs_p2p_emit_packets, first_call, n, ack_in, resend, out, shapes)

    def _emit(self, entry, first_call, n, ack_in, resend, out, shapes):
        """An emit call of either kind: [ack_in, resend, start, len, per-call word, packets]."""
        dtypes = ("int32", "uint8", "int32", "int32", "int32", "uint8")
        dev = out is not None
        outs = list(out) if dev else [np.zeros(shape, dt) for shape, dt in zip(shapes[2:], dtypes[2:])]
        ptrs, keep = _lib.marshal([ack_in, resend] + outs, shapes, dtypes, dev)
        _lib.check(entry(self._h, first_call, n, *ptrs, int(dev)))
        return tuple(outs)

    def emit_state(self):
        """(last_acked, pending, status, closed_call) [S] int32 each: last_acked_input's frame, the
        pending inputs, 0 / GGRS_EMIT_CLOSED / GGRS_EMIT_DISCONNECTED, and the closing call (-1)."""
        out = [np.zeros(self.num_sessions, np.int32) for _ in range(4)]
        _lib.check(self._L.ggrs_p2p_read_emit_state(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    # ---- spectator emit (include/ggrs_amd.h, ggrs_p2p_*spectator*; p2p_spec_emit.hip)
    def set_spectator_emit(self, num_spectators=1, max_pending_inputs=64, out_stride=None):
        """The sessions' confirmed inputs go out to num_spectators (1..4) spectator endpoints per
        session as Input message bodies built on the device (emit_spectator_packets); after
        set_arrival_schedule, before the first call.  out_stride defaults to
        codec.max_packet_bytes(num_players, max_pending_inputs)."""
        if out_stride is None:
            out_stride = int(self._L.ggrs_codec_max_packet_bytes(self.num_players, max_pending_inputs))
        _lib.check(self._L.ggrs_p2p_set_spectator_emit(self._h, num_spectators, max_pending_inputs, out_stride))
        self.num_spectators, self.spectator_max_pending, self.spectator_stride = (num_spectators, max_pending_inputs,
                                                                                  out_stride)

    def emit_spectator_packets(self, first_call, n_calls, ack_in=None, resend=None, out=None):
        """The packets calls first_call .. first_call + n_calls - 1 (already run, emitted in order,
        each once) send to the spectators: ack_in [n][K][S] int32 (the newest InputAck of spectator k,
        NULL_FRAME none) and resend [n][K][S] uint8 (its retry timer fired) or None.  Returns
        (start_frame [n][K][S] int32, -1 no packet; packet_len [n][K][S] int32; notes [n][S] int32,
        the GGRS_SPECTATOR_NOTE words of SpectatorEngine.receive_packets; packets
        [n][K][S][out_stride] uint8) as numpy arrays -- or, with out = such a tuple of torch tensors
        on the engine's device (ack_in and resend then device tensors too), fills and returns them;
        the launch runs on the engine's stream (synchronize() before another stream reads)."""
        n, S = int(n_calls), self.num_sessions
        stride, K = getattr(self, "spectator_stride", None), getattr(self, "num_spectators", 1)
        if stride is None:
            _lib.check(self._L.ggrs_p2p_emit_spectator_packets(self._h, first_call, n, None, None, None, None, None,
                                                               None, 0))  # (the library's own error)
            raise _lib.GgrsError(_lib.GGRS_E_STATE, "emit_spectator_packets needs set_spectator_emit")
        shapes = ((n, K, S), (n, K, S), (n, K, S), (n, K, S), (n, S), (n, K, S, stride))
        return self._emit(self._L.ggrs_p2p_emit_spectator_packets, first_call, n, ack_in, resend, out, shapes)

    def read_spectator_emit_state(self):
        """(next_spectator_frame [S], last_acked [K][S], pending [K][S], status [K][S], closed_call
        [K][S]) int32: per endpoint last_acked_input's frame, the pending inputs, 0 /
        GGRS_EMIT_DISCONNECTED / GGRS_EMIT_ROW_LOST, and the closing call (-1)."""
        S, K = self.num_sessions, getattr(self, "num_spectators", 1)
        out = [np.zeros(S, np.int32)] + [np.zeros((K, S), np.int32) for _ in range(4)]
        _lib.check(self._L.ggrs_p2p_read_spectator_emit_state(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    # ---- time sync (include/ggrs_amd.h, ggrs_p2p_*time_sync*; p2p_time_sync.hip)
    def set_time_sync(self, fps=60):
        """Every session's frames_ahead and WaitRecommendation are computed on the device (time_sync);
        after set_arrival_schedule, before the first call.  fps in 1..1000 (the reference's default)."""
        _lib.check(self._L.ggrs_p2p_set_time_sync(self._h, fps))
        self.fps = fps

    def time_sync(self, first_call, n_calls, rtt_ms=None, remote_advantage=None, out=None):
        """Time sync of calls first_call .. first_call + n_calls - 1 (already run, taken in order, each
        once): rtt_ms [n][S] int32 (the round trip a QualityReply measured at the call, negative: none)
        and remote_advantage [n][S] int32 (the frame_advantage of a QualityReport received at the call,
        GGRS_TIME_SYNC_KEEP: none) or None.  Returns (local_advantage, frames_ahead, skip_frames) [n][S]
        int32 as numpy arrays -- or, with out = such a tuple of torch tensors on the engine's device
        (rtt_ms and remote_advantage then device tensors too), fills and returns them; the launch runs
        on the engine's stream (synchronize() before another stream reads).  skip_frames > 0 is the
        call's GgrsEvent::WaitRecommendation."""
        n, S = int(n_calls), self.num_sessions
        dev = out is not None
        outs = list(out) if dev else [np.zeros((n, S), np.int32) for _ in range(3)]
        ptrs, keep = _lib.marshal([rtt_ms, remote_advantage] + outs, ((n, S),) * 5, ("int32",) * 5, dev)
        _lib.check(self._L.ggrs_p2p_time_sync(self._h, first_call, n, *ptrs, int(dev)))
        return tuple(outs)

    def time_sync_state(self):
        """(local_advantage, remote_advantage, rtt_ms, next_recommended_sleep, closed_call) [S] int32
        each (closed_call -1: the endpoint is open) and windows [2][30][S] int32, the local window then
        the remote one."""
        S = self.num_sessions
        out = [np.zeros(S, np.int32) for _ in range(5)] + [np.zeros((2, 30, S), np.int32)]
        _lib.check(self._L.ggrs_p2p_read_time_sync_state(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    # ---- checksum comparison (include/ggrs_amd.h, ggrs_p2p_*desync_compare/reports*; p2p_desync.hip)
    def set_desync_compare(self, max_events=4096):
        """The peer's checksum reports are kept and compared on the device (add_remote_reports,
        compare_reports); after set_arrival_schedule and set_desync_detection(interval > 0), before the
        first call.  max_events: the records of the device's event list."""
        _lib.check(self._L.ggrs_p2p_set_desync_compare(self._h, max_events))
        self.max_desync_events = max_events

    def add_remote_reports(self, first_call, frames, checksums, local_last):
        """The peer's reports() rows of its calls first_call .. (in call order from 0): frame [n][S]
        int32, checksum [n][S] uint16 and local_last [n][S] int32 -- numpy arrays, or torch tensors on
        the engine's device (checksum int16 or uint16), copied on the engine's stream."""
        n, S = int(frames.shape[0]), self.num_sessions
        dev = hasattr(frames, "data_ptr")
        ck = "uint16"
        if dev and str(checksums.dtype) == "torch.int16":
            ck = "int16"  # (the bits of the u16 values)
        ptrs, keep = _lib.marshal((frames, checksums, local_last), ((n, S),) * 3, ("int32", ck, "int32"), dev)
        _lib.check(self._L.ggrs_p2p_add_remote_reports(self._h, first_call, n, *ptrs, int(dev)))

    def add_remote_reports_from(self, peer, first_call, n_calls):
        """The same rows straight from the P2PEngine `peer`'s report rows, device to device."""
        _lib.check(self._L.ggrs_p2p_add_remote_reports_from(self._h, peer._h, first_call, n_calls))

    def compare_reports(self, first_call, n_calls, wait=True):
        """Delivery, the local report and the comparison of calls first_call .. first_call + n_calls - 1
        (already run, in order, each once; the peer's rows through call first_call + n_calls - 2 added).
        Returns the events raised so far in all (wait=False: None, without waiting for the launch)."""
        total = ctypes.c_int32()
        _lib.check(self._L.ggrs_p2p_compare_reports(self._h, first_call, n_calls, ctypes.byref(total) if wait else None))
        return total.value if wait else None

    def desync_events(self, first=0, max_records=None):
        """Records first .. of the device's event list: (call, session, frame [n] int32, local, remote
        [n] uint16)."""
        n = getattr(self, "max_desync_events", 0) if max_records is None else max_records
        out = [np.zeros(n, np.int32) for _ in range(3)] + [np.zeros(n, np.uint16) for _ in range(2)]
        got = ctypes.c_int32()
        _lib.check(self._L.ggrs_p2p_read_desync_events(self._h, first, n, *(_vp(a) for a in out), ctypes.byref(got)))
        return tuple(a[:got.value] for a in out)

    def desync_state(self):
        """(status, n_events, first_call, first_frame, first_local, first_remote, refused) [S] int32
        each and (history, pending) [2][32][S] int32: the tables' frames (-1 past the entries) then
        their checksums."""
        S = self.num_sessions
        out = [np.zeros(S, np.int32) for _ in range(7)] + [np.zeros((2, 32, S), np.int32) for _ in range(2)]
        _lib.check(self._L.ggrs_p2p_read_desync_state(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    # ---- endpoint poll (include/ggrs_amd.h, ggrs_p2p_*endpoint*; p2p_poll.hip)
    def set_endpoint_poll(self, disconnect_timeout_ms=2000, disconnect_notify_start_ms=500, start_ms=0):
        """Every session's UdpProtocol::poll runs on the device (poll_endpoints): the retry and
        quality-report timers, NetworkInterrupted / NetworkResumed and the disconnect timeout; after
        set_arrival_schedule, before the first call.  The defaults are the reference's; every clock of
        the endpoints starts at start_ms.  From then on advance_frames refuses a call not polled."""
        _lib.check(self._L.ggrs_p2p_set_endpoint_poll(self._h, disconnect_timeout_ms, disconnect_notify_start_ms,
                                                      start_ms))
        self.disconnect_timeout_ms, self.disconnect_notify_start_ms = disconnect_timeout_ms, disconnect_notify_start_ms

    def poll_endpoints(self, first_call, n_calls, now_ms, kinds=None, out=None):
        """The polls of calls first_call .. first_call + n_calls - 1 (in order, each once, after their
        arrivals were added or packets received, before they run): now_ms [n] uint64 (never
        decreasing) and kinds [n][S] uint8 (wire.unpack's, None: nothing arrived).  Returns (resend,
        send_ack, send_report, net_events) [n][S] uint8 as numpy arrays -- or, with out = such a tuple
        of torch tensors on the engine's device (now_ms then an int64 device tensor holding the u64's
        bits, kinds a device tensor), fills and returns them; the launch runs on the engine's stream
        (synchronize() before another stream reads).  net_events holds GGRS_NET_* bits; a
        GGRS_NET_DISCONNECTED call has the remote players' bits in its events row on the device."""
        n, S = int(n_calls), self.num_sessions
        dev = out is not None
        outs = list(out) if dev else [np.zeros((n, S), np.uint8) for _ in range(4)]
        ptrs, keep = _lib.marshal([now_ms, kinds] + outs, ((n,),) + ((n, S),) * 5,
                                  ("int64" if dev else "uint64",) + ("uint8",) * 5, dev)
        _lib.check(self._L.ggrs_p2p_poll_endpoints(self._h, first_call, n, *ptrs, int(dev)))
        return tuple(outs)

    def endpoint_state(self):
        """(state [S] int32: GGRS_ENDPOINT_*; last_recv_ms, last_input_recv_ms, last_report_ms,
        shutdown_ms [S] uint64; flags [S] int32: bit 0 disconnect_notify_sent, bit 1
        disconnect_event_sent; closed_call [S] int32: the call that left Running, -1)."""
        S = self.num_sessions
        out = [np.zeros(S, np.int32)] + [np.zeros(S, np.uint64) for _ in range(4)] + [np.zeros(S, np.int32) for _ in range(2)]
        _lib.check(self._L.ggrs_p2p_read_endpoint_state(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    # ---- spectator endpoint poll (include/ggrs_amd.h, "Spectator endpoint poll"; p2p_spec_poll.hip)
    def set_spectator_poll(self, disconnect_timeout_ms=2000, disconnect_notify_start_ms=500, start_ms=0):
        """The sessions' endpoints towards their spectators are polled on the device
        (poll_spectator_endpoints): the 200 ms retry and quality-report timers, NetworkInterrupted /
        NetworkResumed, the disconnect timeout and the way to Shutdown; after set_spectator_emit, before
        the first call.  From then on emit_spectator_packets refuses a call not polled, and an endpoint
        the poll closed gets nothing more."""
        _lib.check(self._L.ggrs_p2p_set_spectator_poll(self._h, disconnect_timeout_ms, disconnect_notify_start_ms,
                                                       start_ms))

    def poll_spectator_endpoints(self, first_call, n_calls, now_ms, kinds=None, close_in=None, out=None):
        """The polls of calls first_call .. first_call + n_calls - 1 (in order, each once): now_ms [n]
        uint64 (never decreasing), kinds [n][K][S] uint8 (wire.unpack's per spectator link, None: nothing
        arrived) and close_in [n][K][S] uint8 (the host's own disconnect_player(spectator), None).
        Returns (resend, send_report, net_events) [n][K][S] uint8 as numpy arrays -- or, with out = such
        a tuple of torch tensors on the engine's device (now_ms then an int64 device tensor holding the
        u64's bits, kinds and close_in device tensors), fills and returns them; the launch runs on the
        engine's stream.  resend is emit_spectator_packets' input."""
        n, S, K = int(n_calls), self.num_sessions, getattr(self, "num_spectators", 1)
        dev = out is not None
        outs = list(out) if dev else [np.zeros((n, K, S), np.uint8) for _ in range(3)]
        ptrs, keep = _lib.marshal([now_ms, kinds, close_in] + outs, ((n,),) + ((n, K, S),) * 5,
                                  ("int64" if dev else "uint64",) + ("uint8",) * 5, dev)
        _lib.check(self._L.ggrs_p2p_poll_spectator_endpoints(self._h, first_call, n, *ptrs, int(dev)))
        return tuple(outs)

    def spectator_endpoint_state(self):
        """endpoint_state()'s tuple for the spectator endpoints, [K][S] each."""
        S, K = self.num_sessions, getattr(self, "num_spectators", 1)
        out = ([np.zeros((K, S), np.int32)] + [np.zeros((K, S), np.uint64) for _ in range(4)]
               + [np.zeros((K, S), np.int32) for _ in range(2)])
        _lib.check(self._L.ggrs_p2p_read_spectator_endpoint_state(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    # ---- event queue (include/ggrs_amd.h, "Event queue"; p2p_events.hip)
    def set_event_queue(self, capacity=128):
        """Every session's GgrsEvent queue is kept on the device (collect_events, drain_events): a ring
        of `capacity` (128..1024) records per session; after set_arrival_schedule, before the first
        call."""
        _lib.check(self._L.ggrs_p2p_set_event_queue(self._h, capacity))
        self.event_capacity = capacity

    def collect_events(self, first_call, n_calls, events=None, disc_req=None, handled_inputs=None, net_events=None,
                       spec_net_events=None, skip_frames=None, desync=None, on_device=False):
        """What calls first_call .. first_call + n_calls - 1 (in order, each once) push into the
        sessions' event queues, with the reference's trim to 100: events, disc_req, handled_inputs and
        net_events [n][S] uint8, spec_net_events [n][K][S] uint8, skip_frames [n][S] int32, any None
        (nothing happened).  desync: None, the tuple desync_events() returns (call, session, frame
        int32, local, remote uint16), or "engine" for the records compare_reports appended on the
        device.  on_device: every array is a torch tensor on the engine's device (uint16 as int16)."""
        n, S, K = int(n_calls), self.num_sessions, getattr(self, "num_spectators", 0)
        own = isinstance(desync, str)
        if own and desync != "engine":
            raise _lib.InvalidRequest(-1, 'desync is None, a tuple of five arrays or "engine"')
        ds = (None,) * 5 if own or desync is None else tuple(desync)
        nd = -1 if own else (0 if desync is None else int(ds[0].shape[0]))
        if nd == 0:
            ds = (None,) * 5
        u16 = "int16" if on_device else "uint16"
        ptrs, keep = _lib.marshal([events, disc_req, handled_inputs, net_events, spec_net_events, skip_frames, *ds],
                                  ((n, S),) * 4 + ((n, K, S), (n, S)) + ((max(nd, 0),),) * 5,
                                  ("uint8",) * 5 + ("int32",) * 4 + (u16, u16), on_device)
        _lib.check(self._L.ggrs_p2p_collect_events(self._h, first_call, n, *ptrs[:6], nd, *ptrs[6:], int(bool(on_device))))

    def drain_events(self, max_records=None, out=None):
        """Every session's events() at once -> (events, n_left): a structured array (_lib.DRAINED_EVENT:
        session, kind, endpoint, reserved, call, payload) ordered by session, then queue order; those
        queues are left empty.  With max_records too small, whole sessions in ascending order while
        they fit; n_left records stay queued.  out: see _lib.drain_events."""
        if max_records is None:
            max_records = self.num_sessions * getattr(self, "event_capacity", 0)
        return _lib.drain_events(self._L.ggrs_p2p_drain_events, self._h, max_records, out)

    def event_queue_state(self, queue=True):
        """(length, dropped, status, closed_call) [S] int32 each -- status 0 or GGRS_EVENTS_LOST,
        closed_call the call that closed the remote endpoint (-1) -- and, with queue, the queues
        [capacity][S] (_lib.EVENT_RECORD) in queue order, without draining."""
        return _lib.event_queue_state(self._L.ggrs_p2p_read_event_queue_state, self._h, self.num_sessions,
                                      getattr(self, "event_capacity", 0), queue)

    KERNEL_FORMS = {"default": 0, "unstaged": 1, "lockstep": 2, "flat": 3, "chains": 4, "flat_queues": 5,
                    "canonical": 6}

    def set_unstaged(self, on=True):
        """Calls in lockstep with input rows read from global memory (for comparison)."""
        self.set_kernel_form("unstaged" if on else "default")

    def set_kernel_form(self, form):
        """"default" (flat whenever input rows can be staged, with the block's session rings in LDS
        for the launch where they fit; the chains form instead when the sessions fill at most one
        wave per CU), "flat" (each session's calls as its own step sequence, rings in HBM),
        "lockstep" (calls in lockstep, rows staged in LDS), "unstaged" (lockstep, rows from global
        memory), "chains" (every call as a chain of remote_latency + 1 advances from the confirmed
        state, chains pipelined over lanes; plain launches only), "flat_queues" (the flattened form
        with LDS rings stepping the InputQueue bookkeeping) or "canonical" (the flattened form with
        the rollback decision read off the inputs, the default's choice for plain launches, sparse
        saving included)."""
        _lib.check(self._L.ggrs_p2p_set_unstaged(self._h, self.KERNEL_FORMS[form]))
