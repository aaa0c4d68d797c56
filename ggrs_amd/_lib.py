"""ctypes binding of the engine's C ABI (include/ggrs_amd.h) -- libggrs_amd.so, built in-tree.

There is no fallback: if the HIP library is missing or fails to load, every entry point raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libggrs_amd.so")
# timing-experiment builds (tools/exp_build.sh) live in ggrs_amd/exp/; only those may replace the library
_EXP = os.environ.get("GGRS_AMD_EXP_LIB")
if _EXP:
    LIB_PATH = os.path.join(HERE, "exp", os.path.basename(_EXP))

ABI_VERSION = 6  # include/ggrs_amd.h GGRS_ABI_VERSION
GGRS_OK = 0
GGRS_E_INVALID = -1
GGRS_E_PRECONDITION = -2
GGRS_E_HIP = -3
GGRS_E_STATE = -4
GGRS_E_TOO_FAR_BEHIND = -5
GGRS_PACKET_NO_REFERENCE, GGRS_PACKET_STOPPED = -16, -17  # ggrs_p2p_read_packet_results's own status codes
GGRS_EMIT_CLOSED, GGRS_EMIT_DISCONNECTED = -18, -19  # ggrs_p2p_read_emit_state's status
GGRS_EMIT_ROW_LOST = -20  # ggrs_p2p_read_spectator_emit_state's own status
GGRS_TIME_SYNC_KEEP = -2 ** 31  # ggrs_p2p_time_sync's remote_advantage: no report at this call
GGRS_DESYNC_ROW_LOST = -21  # ggrs_p2p_read_desync_state's status
# ggrs_p2p_poll_endpoints' net_events bits and ggrs_p2p_read_endpoint_state's state
GGRS_NET_INTERRUPTED, GGRS_NET_RESUMED, GGRS_NET_DISCONNECTED, GGRS_NET_SHUTDOWN = 1, 2, 4, 8
GGRS_ENDPOINT_RUNNING, GGRS_ENDPOINT_DISCONNECTED, GGRS_ENDPOINT_SHUTDOWN = 0, 1, 2
# the event queue's record kinds (ggrs_event_record_t.kind) and ggrs_p2p_read_event_queue_state's status
(GGRS_EVENT_DISCONNECTED, GGRS_EVENT_NETWORK_INTERRUPTED, GGRS_EVENT_NETWORK_RESUMED, GGRS_EVENT_WAIT_RECOMMENDATION,
 GGRS_EVENT_DESYNC_DETECTED) = 1, 2, 3, 4, 5
GGRS_EVENTS_LOST = -27
# ggrs_event_record_t: 16 bytes; a drained list adds the session in front
EVENT_RECORD = np.dtype([("kind", "u1"), ("endpoint", "u1"), ("reserved", "<u2"), ("call", "<i4"), ("payload", "<u8")])
DRAINED_EVENT = np.dtype([("session", "<i4")] + [(n, EVENT_RECORD.fields[n][0]) for n in EVENT_RECORD.names])
# ggrs_wire_unpack's slot_status codes (accepted: tag + 1, empty: 0)
GGRS_WIRE_E_BINCODE, GGRS_WIRE_E_SHAPE, GGRS_WIRE_E_CAP, GGRS_WIRE_E_CLOCK, GGRS_WIRE_E_RANGE = -22, -23, -24, -25, -26
NULL_FRAME = -1
REQ_SAVE, REQ_LOAD, REQ_ADVANCE = 0, 1, 2
STATUS_CONFIRMED, STATUS_PREDICTED, STATUS_DISCONNECTED = 0, 1, 2
LANE_RUNNING, LANE_MISMATCH = 0, 1
PATH_PIPELINED, PATH_SEQUENTIAL, PATH_PIPELINED_CHAINS, PATH_PIPELINED_BATCHED = 0, 1, 2, 3
TOK_SAVE, TOK_ADVANCE, TOK_LOAD, TOK_END = 0, 1, 2, 3
TOKENS_PER_WORD = 16
BATCH_STATUS = 1

# every symbol include/ggrs_amd.h declares (tests check the library exports all of them)
EXPORTS = (
    "ggrs_abi_version", "ggrs_last_error", "ggrs_engine_create", "ggrs_engine_destroy",
    "ggrs_engine_config", "ggrs_add_local_inputs", "ggrs_add_local_inputs_device",
    "ggrs_synctest_advance_frames", "ggrs_handle_requests", "ggrs_synchronize",
    "ggrs_current_frame", "ggrs_read_mismatches", "ggrs_read_save_checksums", "ggrs_read_save_checksums_frames", "ggrs_read_state", "ggrs_read_states",
    "ggrs_read_ring", "ggrs_read_trace", "ggrs_debug_corrupt_on_load", "ggrs_last_launch_ms",
    "ggrs_timing_reset", "ggrs_timing_stop", "ggrs_timing_read", "ggrs_set_synctest_path",
    "ggrs_lane_batch_map", "ggrs_lane_batch_run", "ggrs_handle_requests_lanes", "ggrs_read_lane_frames",
    "ggrs_lane_server", "ggrs_lane_batch_submit", "ggrs_lane_batch_wait", "ggrs_lane_encode", "ggrs_lane_shape",
    "ggrs_lane_batch_lds",
    "ggrs_branch_engine_create", "ggrs_branch_engine_destroy", "ggrs_branch_engine_config",
    "ggrs_branch_add_inputs", "ggrs_branch_speculate", "ggrs_branch_confirm",
    "ggrs_branch_report_bytes", "ggrs_branch_synchronize", "ggrs_branch_trunk_frame",
    "ggrs_branch_read_report", "ggrs_branch_read_desync", "ggrs_branch_read_trunk",
    "ggrs_branch_read_lane", "ggrs_branch_read_cells", "ggrs_branch_timing_reset", "ggrs_branch_timing_stop", "ggrs_branch_timing_read",
    "ggrs_branch_rounds", "ggrs_branch_set_round_launches", "ggrs_branch_set_stream", "ggrs_branch_use_own_stream",
    "ggrs_branch_round", "ggrs_branch_rounds_reports", "ggrs_branch_compare_peer", "ggrs_branch_compare_peer_rows",
    "ggrs_particle_engine_create", "ggrs_particle_engine_destroy", "ggrs_particle_add_local_inputs",
    "ggrs_particle_synctest_advance_frames", "ggrs_particle_synchronize",
    "ggrs_particle_current_frame", "ggrs_particle_read_mismatches", "ggrs_particle_read_state",
    "ggrs_particle_read_saved", "ggrs_particle_debug_corrupt_on_load",
    "ggrs_particle_timing_reset", "ggrs_particle_timing_stop", "ggrs_particle_timing_read",
    "ggrs_p2p_engine_create", "ggrs_p2p_engine_destroy", "ggrs_p2p_engine_config",
    "ggrs_p2p_add_inputs", "ggrs_p2p_advance_frames", "ggrs_p2p_current_frame", "ggrs_p2p_calls",
    "ggrs_p2p_synchronize", "ggrs_p2p_read_state", "ggrs_p2p_read_ring", "ggrs_p2p_read_stats", "ggrs_p2p_read_queues",
    "ggrs_p2p_read_trace", "ggrs_p2p_timing_reset", "ggrs_p2p_timing_stop", "ggrs_p2p_timing_read",
    "ggrs_p2p_set_desync_detection", "ggrs_p2p_local_checksums", "ggrs_p2p_compare_checksums",
    "ggrs_p2p_debug_desync", "ggrs_p2p_set_sparse_saving", "ggrs_p2p_set_unstaged",
    "ggrs_p2p_set_arrival_schedule", "ggrs_p2p_add_arrivals", "ggrs_p2p_read_sessions", "ggrs_p2p_read_reports", "ggrs_p2p_read_states", "ggrs_p2p_add_peer_reports",
    "ggrs_p2p_set_packet_feed", "ggrs_p2p_receive_packets", "ggrs_p2p_read_packet_results",
    "ggrs_p2p_set_packet_emit", "ggrs_p2p_emit_packets", "ggrs_p2p_read_emit_state",
    "ggrs_p2p_set_spectator_emit", "ggrs_p2p_emit_spectator_packets", "ggrs_p2p_read_spectator_emit_state",
    "ggrs_p2p_set_time_sync", "ggrs_p2p_time_sync", "ggrs_p2p_read_time_sync_state",
    "ggrs_p2p_set_desync_compare", "ggrs_p2p_add_remote_reports", "ggrs_p2p_add_remote_reports_from",
    "ggrs_p2p_compare_reports", "ggrs_p2p_read_desync_events", "ggrs_p2p_read_desync_state",
    "ggrs_p2p_set_endpoint_poll", "ggrs_p2p_poll_endpoints", "ggrs_p2p_read_endpoint_state",
    "ggrs_p2p_set_spectator_poll", "ggrs_p2p_poll_spectator_endpoints", "ggrs_p2p_read_spectator_endpoint_state",
    "ggrs_p2p_set_event_queue", "ggrs_p2p_collect_events", "ggrs_p2p_drain_events", "ggrs_p2p_read_event_queue_state",
    "ggrs_spectator_engine_create", "ggrs_spectator_engine_destroy", "ggrs_spectator_engine_config",
    "ggrs_spectator_add_inputs", "ggrs_spectator_add_arrivals", "ggrs_spectator_advance_frames",
    "ggrs_spectator_calls", "ggrs_spectator_synchronize", "ggrs_spectator_read_sessions",
    "ggrs_spectator_read_state", "ggrs_spectator_read_states", "ggrs_spectator_read_trace",
    "ggrs_spectator_timing_reset", "ggrs_spectator_timing_stop", "ggrs_spectator_timing_read",
    "ggrs_spectator_set_packet_feed", "ggrs_spectator_receive_packets", "ggrs_spectator_read_packet_results",
    "ggrs_spectator_set_endpoint_poll", "ggrs_spectator_poll_endpoints", "ggrs_spectator_read_endpoint_state",
    "ggrs_spectator_set_event_queue", "ggrs_spectator_collect_events", "ggrs_spectator_drain_events",
    "ggrs_spectator_read_event_queue_state",
    "ggrs_codec_encode", "ggrs_codec_decode", "ggrs_codec_encode_chunked", "ggrs_codec_decode_chunked", "ggrs_codec_max_packet_bytes", "ggrs_codec_set_direct",
    "ggrs_wire_max_datagram_bytes", "ggrs_wire_unpack", "ggrs_wire_pack",
)


class Config(ctypes.Structure):
    _fields_ = [
        ("num_lanes", ctypes.c_int32),
        ("num_players", ctypes.c_int32),
        ("max_prediction", ctypes.c_int32),
        ("check_distance", ctypes.c_int32),
        ("input_delay", ctypes.c_int32),
        ("input_capacity", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("trace_capacity", ctypes.c_int32),
    ]


class Request(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("frame", ctypes.c_int32)]


class LaneBatch(ctypes.Structure):
    """ggrs_lane_batch_t"""
    _fields_ = [
        ("token_words", ctypes.c_int32),
        ("load_slots", ctypes.c_int32),
        ("adv_rows", ctypes.c_int32),
        ("save_rows", ctypes.c_int32),
        ("tokens", ctypes.POINTER(ctypes.c_uint32)),
        ("load_frames", ctypes.POINTER(ctypes.c_int32)),
        ("inputs", ctypes.POINTER(ctypes.c_uint8)),
        ("status", ctypes.POINTER(ctypes.c_uint8)),
        ("checksums", ctypes.POINTER(ctypes.c_uint16)),
        ("lane_result", ctypes.POINTER(ctypes.c_int32)),
    ]


class GgrsError(Exception):
    """Mirror of GgrsError (src/error.rs:31-57) for errors the engine reports."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class InvalidRequest(GgrsError):
    """GgrsError::InvalidRequest (error.rs:39-43)."""


class PreconditionError(GgrsError):
    """A condition on which the reference panics (assert!), reported instead of unwinding."""


_lib = None


def lib():
    """Load libggrs_amd.so (raises OSError if it has not been built: no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not built: run `python -m ggrs_amd.build` "
                          "(the engine has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        vp = ctypes.c_void_p
        L.ggrs_abi_version.restype = ctypes.c_int32
        L.ggrs_last_error.restype = ctypes.c_char_p
        if L.ggrs_abi_version() != ABI_VERSION:  # a stale build: fail loudly, never misread a signature
            raise OSError(f"{LIB_PATH} implements ABI {L.ggrs_abi_version()}, this package binds ABI "
                          f"{ABI_VERSION}: rebuild with `python -m ggrs_amd.build`")
        L.ggrs_engine_create.argtypes = [P(Config), P(vp)]
        L.ggrs_engine_destroy.argtypes = [vp]
        L.ggrs_engine_config.argtypes = [vp, P(Config)]
        L.ggrs_add_local_inputs.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp]
        L.ggrs_add_local_inputs_device.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp]
        L.ggrs_synctest_advance_frames.argtypes = [vp, ctypes.c_int32]
        L.ggrs_handle_requests.argtypes = [vp, P(Request), ctypes.c_int32, vp, vp]
        L.ggrs_synchronize.argtypes = [vp]
        L.ggrs_current_frame.argtypes = [vp, P(ctypes.c_int32)]
        L.ggrs_read_mismatches.argtypes = [vp, vp, vp, vp]
        L.ggrs_read_save_checksums.argtypes = [vp, ctypes.c_int32, vp]
        L.ggrs_read_save_checksums_frames.argtypes = [vp, vp, ctypes.c_int32, vp]
        L.ggrs_read_state.argtypes = [vp, ctypes.c_int32, vp]
        L.ggrs_read_states.argtypes = [vp, vp]
        L.ggrs_read_ring.argtypes = [vp, ctypes.c_int32, vp, vp, vp]
        L.ggrs_read_trace.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, vp]
        L.ggrs_debug_corrupt_on_load.argtypes = [vp, ctypes.c_int32, ctypes.c_int32]
        L.ggrs_last_launch_ms.argtypes = [vp, P(ctypes.c_float)]
        L.ggrs_timing_reset.argtypes = [vp]
        L.ggrs_timing_stop.argtypes = [vp]
        L.ggrs_set_synctest_path.argtypes = [vp, ctypes.c_int32]
        L.ggrs_timing_read.argtypes = [vp, P(ctypes.c_float), P(ctypes.c_int32)]
        i32 = ctypes.c_int32
        L.ggrs_lane_batch_map.argtypes = [vp, i32, i32, i32, i32, P(LaneBatch)]
        L.ggrs_lane_batch_run.argtypes = [vp, P(LaneBatch), i32, P(i32)]
        L.ggrs_lane_batch_submit.argtypes = [vp, P(LaneBatch), i32]
        L.ggrs_lane_batch_wait.argtypes = [vp, P(i32)]
        L.ggrs_lane_encode.argtypes = [P(LaneBatch), ctypes.c_int64, i32, ctypes.c_int64, vp, i32, vp, vp, i32, P(i32)]
        L.ggrs_lane_shape.argtypes = [vp, i32, vp]
        L.ggrs_lane_batch_lds.argtypes = [vp, i32, i32, i32, i32, P(ctypes.c_int64), P(ctypes.c_int64)]
        L.ggrs_handle_requests_lanes.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.ggrs_read_lane_frames.argtypes = [vp, vp]
        L.ggrs_lane_server.argtypes = [vp, i32]
        for name in EXPORTS:
            if name not in ("ggrs_abi_version", "ggrs_last_error", "ggrs_codec_max_packet_bytes",
                            "ggrs_wire_max_datagram_bytes"):
                getattr(L, name).restype = ctypes.c_int
        _lib = L
    return _lib


def marshal(arrays, shapes, dtypes, device):
    """ctypes arguments for a call's arrays (None stays None) -> (args, keep).  device: torch tensors
    on the engine's device, passed in place -- each must be contiguous, of its shape and dtype; else
    numpy arrays, converted where needed and checked for their shape (keep holds the converted
    arrays, which must outlive the call)."""
    args, keep = [], []
    for a, shape, dt in zip(arrays, shapes, dtypes):
        if a is None:
            args.append(None)
        elif device:
            if (not hasattr(a, "data_ptr") or tuple(a.shape) != tuple(shape) or not a.is_contiguous()
                    or str(a.dtype) != "torch." + dt or not a.is_cuda):
                raise InvalidRequest(-1, f"device arrays must be contiguous {dt} {shape} on the device")
            args.append(ctypes.c_void_p(a.data_ptr()))
        else:
            a = np.ascontiguousarray(a, dt)
            if a.shape != tuple(shape):
                raise InvalidRequest(-1, f"expected shape {shape}, got {a.shape}")
            keep.append(a)
            args.append(ctypes.c_void_p(a.ctypes.data))
    return args, keep


def drain_events(fn, handle, max_records, out=None):
    """ggrs_*_drain_events: (events, n_left).  events is a DRAINED_EVENT array of the records read --
    or, with out = (session int32 [max_records], records uint8 [max_records][16]) torch tensors on the
    engine's device, the count of records written to them."""
    n_read, n_left = ctypes.c_int32(), ctypes.c_int32()
    m = int(max_records)
    if out is not None:
        ptrs, _ = marshal(out, ((m,), (m, 16)), ("int32", "uint8"), True)
        check(fn(handle, m, *ptrs, ctypes.byref(n_read), ctypes.byref(n_left), 1))
        return n_read.value, n_left.value
    sess, recs = np.zeros(m, np.int32), np.zeros(m, EVENT_RECORD)
    check(fn(handle, m, ctypes.c_void_p(sess.ctypes.data), ctypes.c_void_p(recs.ctypes.data), ctypes.byref(n_read),
             ctypes.byref(n_left), 0))
    ev = np.zeros(n_read.value, DRAINED_EVENT)
    ev["session"] = sess[:n_read.value]
    for name in EVENT_RECORD.names:
        ev[name] = recs[name][:n_read.value]
    return ev, n_left.value


def event_queue_state(fn, handle, num_sessions, capacity, queue=True):
    """ggrs_*_read_event_queue_state: (length, dropped, status, closed_call) [S] int32 each and, with
    queue, the queues [capacity][S] as EVENT_RECORD in queue order (zero past a queue's length)."""
    out = [np.zeros(num_sessions, np.int32) for _ in range(4)]
    q = np.zeros((capacity, num_sessions), EVENT_RECORD) if queue else None
    check(fn(handle, *(ctypes.c_void_p(a.ctypes.data) for a in out), ctypes.c_void_p(q.ctypes.data) if queue else None))
    return tuple(out) + ((q,) if queue else ())


def check(rc):
    if rc == GGRS_OK:
        return
    msg = lib().ggrs_last_error().decode(errors="replace")
    if rc == GGRS_E_INVALID:
        raise InvalidRequest(rc, msg)
    if rc == GGRS_E_PRECONDITION:
        raise PreconditionError(rc, msg)
    raise GgrsError(rc, msg)
