"""Batched SpectatorSession over the engine's C ABI (include/ggrs_amd.h, ggrs_spectator_*).

One SpectatorEngine holds S spectators, each following one host's confirmed input stream over its
own network.  Each call of advance_frames(n) runs n x SpectatorSession::advance_frame
(src/sessions/p2p_spectator_session.rs:103-129) + the ex_game handler for every session: the
host's frames up to recv_upto arrive (Event::Input, :218-231), a session more than
max_frames_behind frames behind advances catchup_speed frames, one that has nothing to advance
waits (PredictionThreshold, :175-177), one whose host ran 60 frames ahead is lost
(SpectatorTooFarBehind, :180-182).  The device decides per session; kernel: csrc/spectator.hip.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import InvalidRequest

SPECTATOR_BUFFER_SIZE = 60  # p2p_spectator_session.rs:17
DEFAULT_MAX_FRAMES_BEHIND = 10  # builder.rs:22
DEFAULT_CATCHUP_SPEED = 1  # builder.rs:23
TOO_FAR_BEHIND = _lib.GGRS_E_TOO_FAR_BEHIND


class SpectatorConfig(ctypes.Structure):
    _fields_ = [
        ("num_sessions", ctypes.c_int32),
        ("num_players", ctypes.c_int32),
        ("max_frames_behind", ctypes.c_int32),
        ("catchup_speed", ctypes.c_int32),
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
    L.ggrs_spectator_engine_create.argtypes = [P(SpectatorConfig), P(vp)]
    L.ggrs_spectator_engine_destroy.argtypes = [vp]
    L.ggrs_spectator_engine_config.argtypes = [vp, P(SpectatorConfig)]
    L.ggrs_spectator_add_inputs.argtypes = [vp, i32, i32, vp]
    L.ggrs_spectator_add_arrivals.argtypes = [vp, i32, i32, vp, vp]
    L.ggrs_spectator_advance_frames.argtypes = [vp, i32]
    L.ggrs_spectator_calls.argtypes = [vp, P(i32)]
    L.ggrs_spectator_synchronize.argtypes = [vp]
    L.ggrs_spectator_read_sessions.argtypes = [vp, vp, vp, vp, vp]
    L.ggrs_spectator_read_state.argtypes = [vp, i32, vp]
    L.ggrs_spectator_read_states.argtypes = [vp, vp]
    L.ggrs_spectator_read_trace.argtypes = [vp, i32, i32, vp, vp]
    L.ggrs_spectator_timing_reset.argtypes = [vp]
    L.ggrs_spectator_timing_stop.argtypes = [vp]
    L.ggrs_spectator_timing_read.argtypes = [vp, P(ctypes.c_float), P(i32)]
    L.ggrs_spectator_set_packet_feed.argtypes = [vp, i32, i32, i32]
    L.ggrs_spectator_receive_packets.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32]
    L.ggrs_spectator_read_packet_results.argtypes = [vp, i32, i32, vp, vp]
    u64 = ctypes.c_uint64
    L.ggrs_spectator_set_endpoint_poll.argtypes = [vp, u64, u64, u64]
    L.ggrs_spectator_poll_endpoints.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
    L.ggrs_spectator_read_endpoint_state.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ggrs_spectator_set_event_queue.argtypes = [vp, i32]
    L.ggrs_spectator_collect_events.argtypes = [vp, i32, i32, vp, vp, i32]
    L.ggrs_spectator_drain_events.argtypes = [vp, i32, vp, vp, P(i32), P(i32), i32]
    L.ggrs_spectator_read_event_queue_state.argtypes = [vp, vp, vp, vp, vp, vp]
    for name in _lib.EXPORTS:
        if name.startswith("ggrs_spectator_"):
            getattr(L, name).restype = ctypes.c_int
    _bound = True


def spectator_note(player, frame):
    """GGRS_SPECTATOR_NOTE: the host's input message reports `player` disconnected with last frame
    `frame` (protocol.rs:575-585).  0 = no note."""
    return 1 | player << 1 | (frame + 1) << 3


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class SpectatorEngine:
    """S spectator sessions, each of its own host."""

    def __init__(self, num_sessions, num_players=2, max_frames_behind=DEFAULT_MAX_FRAMES_BEHIND,
                 catchup_speed=DEFAULT_CATCHUP_SPEED, input_capacity=0, trace_capacity=0, device=0):
        self._L = _lib.lib()
        _bind(self._L)
        cfg = SpectatorConfig(num_sessions, num_players, max_frames_behind, catchup_speed, input_capacity,
                              trace_capacity, device)
        h = ctypes.c_void_p()
        _lib.check(self._L.ggrs_spectator_engine_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.num_sessions, self.num_players = num_sessions, num_players
        self.max_frames_behind, self.catchup_speed = max_frames_behind, catchup_speed
        self.trace_capacity = trace_capacity
        self.state_bytes = 36 + 20 * num_players

    def close(self):
        if getattr(self, "_h", None):
            self._L.ggrs_spectator_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def config(self):
        cfg = SpectatorConfig()
        _lib.check(self._L.ggrs_spectator_engine_config(self._h, ctypes.byref(cfg)))
        return cfg

    def add_inputs(self, first_frame, inputs):
        """inputs [n][S][P]: the host's confirmed inputs of frames first_frame .. first_frame + n - 1
        (send_confirmed_inputs_to_spectators, p2p_session.rs:716-745), in order from frame 0; the
        engine keeps the newest input_capacity rows."""
        a = np.ascontiguousarray(inputs, np.uint8)
        if a.ndim != 3 or a.shape[1:] != (self.num_sessions, self.num_players):
            raise InvalidRequest(-1, f"inputs must be [n][{self.num_sessions}][{self.num_players}]")
        _lib.check(self._L.ggrs_spectator_add_inputs(self._h, first_frame, a.shape[0], _vp(a)))

    def add_arrivals(self, first_call, recv_upto, notes=None):
        """recv_upto [n][S] int32: the newest host frame each session's poll delivered by calls
        first_call .. first_call + n - 1 (not bounded by the call: the host has its own clock);
        notes [n][S] int32 (spectator_note(player, frame) or 0) or None."""
        a = np.ascontiguousarray(recv_upto, np.int32)
        if a.ndim != 2 or a.shape[1] != self.num_sessions:
            raise InvalidRequest(-1, f"recv_upto must be [n][{self.num_sessions}]")
        nt = None
        if notes is not None:
            nt = np.ascontiguousarray(notes, np.int32)
            if nt.shape != a.shape:
                raise InvalidRequest(-1, "notes must have recv_upto's shape")
        _lib.check(self._L.ggrs_spectator_add_arrivals(self._h, first_call, a.shape[0], _vp(a), _vp(nt)))

    # ---- packet feed (include/ggrs_amd.h, ggrs_spectator_*packet*; spectator_ingest.hip)
    def set_packet_feed(self, max_prediction=8, max_packet_inputs=64, packet_stride=None):
        """The sessions' inputs and arrivals enter as the wire packets each call's poll received from
        the host (receive_packets) instead of add_inputs / add_arrivals; each session follows its host
        on the host's own clock.  Before the first input, arrival and call.  max_prediction is the
        host endpoint's; packet_stride defaults to codec.max_packet_bytes(num_players,
        max_packet_inputs)."""
        if packet_stride is None:
            packet_stride = int(self._L.ggrs_codec_max_packet_bytes(self.num_players, max_packet_inputs))
        _lib.check(self._L.ggrs_spectator_set_packet_feed(self._h, max_prediction, max_packet_inputs, packet_stride))
        self.max_prediction, self.max_packet_inputs, self.packet_stride = max_prediction, max_packet_inputs, packet_stride

    def receive_packets(self, first_call, start_frame, packet_len, packets, notes=None, on_device=None):
        """The newest packet each session's poll received by calls first_call .. first_call + n - 1:
        start_frame [n][S] int32 (negative: no packet), packet_len [n][S] int32, packets
        [n][S][packet_stride] uint8, notes [n][S] int32 (spectator_note(player, frame) or 0) or None --
        numpy arrays, or with on_device=True (the default for tensors) torch tensors on the engine's
        device, read in place by the launch."""
        n, S = int(start_frame.shape[0]), self.num_sessions
        stride = getattr(self, "packet_stride", None) or int(packets.shape[-1])
        dev = hasattr(packets, "data_ptr") if on_device is None else bool(on_device)
        ptrs, keep = _lib.marshal((start_frame, packet_len, packets, notes), ((n, S), (n, S), (n, S, stride), (n, S)),
                                  ("int32", "int32", "uint8", "int32"), dev)
        _lib.check(self._L.ggrs_spectator_receive_packets(self._h, first_call, n, *ptrs, int(dev)))

    def read_packet_results(self, first_call, n_calls):
        """(status, ack_frame) [n][S] int32 for received calls among the last input_capacity: status 1
        delivered new frames, 0 no packet / nothing new, a GGRS_CODEC_* code, GGRS_PACKET_NO_REFERENCE
        or GGRS_PACKET_STOPPED; ack_frame the endpoint's last_recv_frame after the call (the InputAck)."""
        status = np.zeros((n_calls, self.num_sessions), np.int32)
        ack = np.zeros((n_calls, self.num_sessions), np.int32)
        _lib.check(self._L.ggrs_spectator_read_packet_results(self._h, first_call, n_calls, _vp(status), _vp(ack)))
        return status, ack

    # ---- endpoint poll (include/ggrs_amd.h, "Spectator engine: endpoint poll"; spectator_poll.hip)
    def set_endpoint_poll(self, disconnect_timeout_ms=2000, disconnect_notify_start_ms=500, start_ms=0):
        """Every session's host endpoint is polled on the device (poll_endpoints): when to acknowledge,
        when a quality report is due, NetworkInterrupted / NetworkResumed and the one Disconnected;
        before the first arrival and call.  The defaults are the reference's; every clock of the
        endpoints starts at start_ms."""
        _lib.check(self._L.ggrs_spectator_set_endpoint_poll(self._h, disconnect_timeout_ms, disconnect_notify_start_ms,
                                                            start_ms))
        self.disconnect_timeout_ms, self.disconnect_notify_start_ms = disconnect_timeout_ms, disconnect_notify_start_ms

    def poll_endpoints(self, first_call, n_calls, now_ms, kinds=None, events=None, out=None):
        """The polls of calls first_call .. first_call + n_calls - 1 (in order, each once; with the
        packet feed after their packets were received): now_ms [n] uint64 (never decreasing), kinds
        and events [n][S] uint8 (wire.unpack's; None: nothing arrived / no disconnect request).
        Returns (send_ack, send_report, net_events) [n][S] uint8 as numpy arrays -- or, with out = such
        a tuple of torch tensors on the engine's device (now_ms then an int64 device tensor holding the
        u64's bits, kinds and events device tensors), fills and returns them; the launch runs on the
        engine's stream (synchronize() before another stream reads).  net_events holds GGRS_NET_* bits;
        the endpoint never leaves Running, so GGRS_NET_SHUTDOWN never appears."""
        n, S = int(n_calls), self.num_sessions
        dev = out is not None
        outs = list(out) if dev else [np.zeros((n, S), np.uint8) for _ in range(3)]
        ptrs, keep = _lib.marshal([now_ms, kinds, events] + outs, ((n,),) + ((n, S),) * 5,
                                  ("int64" if dev else "uint64",) + ("uint8",) * 5, dev)
        _lib.check(self._L.ggrs_spectator_poll_endpoints(self._h, first_call, n, *ptrs, int(dev)))
        return tuple(outs)

    def endpoint_state(self):
        """(last_recv_ms, last_input_recv_ms, last_report_ms [S] uint64; flags [S] int32: bit 0
        disconnect_notify_sent, bit 1 disconnect_event_sent; disconnected_call [S] int32: the call that
        raised the one Disconnected, -1)."""
        S = self.num_sessions
        out = [np.zeros(S, np.uint64) for _ in range(3)] + [np.zeros(S, np.int32) for _ in range(2)]
        _lib.check(self._L.ggrs_spectator_read_endpoint_state(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    # ---- event queue (include/ggrs_amd.h, "Spectator engine: event queue"; spectator_events.hip)
    def set_event_queue(self, capacity=128):
        """Every session's GgrsEvent queue is kept on the device (collect_events, drain_events): a ring
        of `capacity` (128..1024) records per session; before the first arrival and call."""
        _lib.check(self._L.ggrs_spectator_set_event_queue(self._h, capacity))
        self.event_capacity = capacity

    def collect_events(self, first_call, n_calls, handled_inputs=None, net_events=None, on_device=False):
        """What calls first_call .. first_call + n_calls - 1 (in order, each once) push into the
        sessions' event queues: net_events [n][S] uint8 (poll_endpoints') and handled_inputs [n][S]
        uint8 (the call decoded a new frame), either None.  Every push and every handled Input trims
        the queue to 100.  on_device: torch tensors on the engine's device."""
        n, S = int(n_calls), self.num_sessions
        ptrs, keep = _lib.marshal([handled_inputs, net_events], ((n, S),) * 2, ("uint8",) * 2, on_device)
        _lib.check(self._L.ggrs_spectator_collect_events(self._h, first_call, n, *ptrs, int(bool(on_device))))

    def drain_events(self, max_records=None, out=None):
        """Every session's events() at once -> (events, n_left), as P2PEngine.drain_events."""
        if max_records is None:
            max_records = self.num_sessions * getattr(self, "event_capacity", 0)
        return _lib.drain_events(self._L.ggrs_spectator_drain_events, self._h, max_records, out)

    def event_queue_state(self, queue=True):
        """(length, dropped, status, closed_call) [S] int32 each -- closed_call the call that pushed the
        one Disconnected (-1) -- and, with queue, the queues [capacity][S] in queue order."""
        return _lib.event_queue_state(self._L.ggrs_spectator_read_event_queue_state, self._h, self.num_sessions,
                                      getattr(self, "event_capacity", 0), queue)

    def advance_frames(self, n=1):
        _lib.check(self._L.ggrs_spectator_advance_frames(self._h, n))

    def calls(self):
        v = ctypes.c_int32()
        _lib.check(self._L.ggrs_spectator_calls(self._h, ctypes.byref(v)))
        return v.value

    def synchronize(self):
        _lib.check(self._L.ggrs_spectator_synchronize(self._h))

    def sessions(self):
        """(current_frame, last_recv, waited, errors) [S] int32 each: waited = the calls that
        returned PredictionThreshold; errors 0, TOO_FAR_BEHIND, or the code the session stopped with."""
        out = [np.zeros(self.num_sessions, np.int32) for _ in range(4)]
        _lib.check(self._L.ggrs_spectator_read_sessions(self._h, *(_vp(a) for a in out)))
        return tuple(out)

    def state(self, session):
        out = np.zeros(self.state_bytes, np.uint8)
        _lib.check(self._L.ggrs_spectator_read_state(self._h, session, _vp(out)))
        return out

    def states(self):
        """state(session) for every session, one transfer: [num_sessions][state_bytes]."""
        out = np.zeros((self.num_sessions, self.state_bytes), np.uint8)
        _lib.check(self._L.ggrs_spectator_read_states(self._h, _vp(out)))
        return out

    def trace(self, first_call, n):
        """(advanced [n][S] uint8, checksums [n][S] uint16) of calls first_call .. first_call + n - 1:
        the AdvanceFrame requests each call returned and the state's fletcher16 after it."""
        adv = np.zeros((n, self.num_sessions), np.uint8)
        cks = np.zeros((n, self.num_sessions), np.uint16)
        _lib.check(self._L.ggrs_spectator_read_trace(self._h, first_call, n, _vp(adv), _vp(cks)))
        return adv, cks

    def timing_reset(self):
        _lib.check(self._L.ggrs_spectator_timing_reset(self._h))

    def timing_stop(self):
        """Record the span's end behind the last launch without waiting (timing_read reports it)."""
        _lib.check(self._L.ggrs_spectator_timing_stop(self._h))

    def timing_read(self):
        ms, n = ctypes.c_float(), ctypes.c_int32()
        _lib.check(self._L.ggrs_spectator_timing_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value
