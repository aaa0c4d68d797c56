"""The GGRS wire envelope over the C ABI (include/ggrs_amd.h, ggrs_wire_*; csrc/wire.hip): a poll's
raw datagrams -- bincode::serialize(&Message), src/network/messages.rs -- become the arrays
P2PEngine.receive_packets, emit_packets(ack_in), time_sync, add_remote_reports and
SpectatorEngine.receive_packets take, and the engines' output arrays become datagrams, all in device
memory.  Stateless like the codec; buffers are torch tensors (torch is only the allocator), the
launches run on torch's current stream; there is no CPU path.

    out = unpack(dgrams, dgram_len, now_ms, num_statuses=2, remote_mask=0b10, packet_stride=eng.packet_stride)
    eng.receive_packets(c, out["start_frame"], out["packet_len"], out["packets"], out["events"])
    ...
    dgrams, dgram_len = pack(magic, now_ms, 2, eng.out_stride, start_frame=start, packet_len=length,
                             ack_frame=ack, packets=packets, send_report=flags, local_advantage=adv)

64-bit and 16-bit unsigned values travel as the bits of torch.int64 / torch.int16 tensors."""
import ctypes

from . import _lib

INPUT, INPUT_ACK, QUALITY_REPORT, QUALITY_REPLY, CHECKSUM_REPORT, KEEP_ALIVE = range(6)
E_BINCODE, E_SHAPE, E_CAP, E_CLOCK, E_RANGE = (_lib.GGRS_WIRE_E_BINCODE, _lib.GGRS_WIRE_E_SHAPE, _lib.GGRS_WIRE_E_CAP,
                                               _lib.GGRS_WIRE_E_CLOCK, _lib.GGRS_WIRE_E_RANGE)
PACK_SLOTS = 4

# unpack's outputs in the ABI's order: name -> (dtype, shape as a function of n, M, S, num_statuses, packet_stride)
UNPACK_OUTPUTS = (
    ("slot_status", "int32", lambda n, M, S, ns, ps: (n, M, S)),
    ("start_frame", "int32", lambda n, M, S, ns, ps: (n, S)),
    ("packet_len", "int32", lambda n, M, S, ns, ps: (n, S)),
    ("packets", "uint8", lambda n, M, S, ns, ps: (n, S, ps)),
    ("ack_in", "int32", lambda n, M, S, ns, ps: (n, S)),
    ("events", "uint8", lambda n, M, S, ns, ps: (n, S)),
    ("disc_mask", "uint8", lambda n, M, S, ns, ps: (n, S)),
    ("last_frame", "int32", lambda n, M, S, ns, ps: (n, ns, S)),
    ("notes", "int32", lambda n, M, S, ns, ps: (n, S)),
    ("remote_advantage", "int32", lambda n, M, S, ns, ps: (n, S)),
    ("ping", "uint8", lambda n, M, S, ns, ps: (n, S, 16)),
    ("rtt_ms", "int32", lambda n, M, S, ns, ps: (n, S)),
    ("report_frame", "int32", lambda n, M, S, ns, ps: (n, S)),
    ("report_checksum", "int16", lambda n, M, S, ns, ps: (n, S)),
    ("kinds", "uint8", lambda n, M, S, ns, ps: (n, S)),
)
# pack's optional inputs in the ABI's order (packet_stride sits after packets)
PACK_INPUTS = (
    ("start_frame", "int32"), ("packet_len", "int32"), ("ack_frame", "int32"), ("packets", "uint8"),
    ("disc_mask", "uint8"), ("last_frame", "int32"), ("disconnect_requested", "uint8"), ("send_ack", "uint8"),
    ("send_report", "uint8"), ("local_advantage", "int32"), ("kinds", "uint8"), ("ping", "uint8"),
    ("report_frame", "int32"), ("report_checksum", "int16"), ("keep_alive", "uint8"),
)

_bound = False


def _bind(L):
    global _bound
    if _bound:
        return
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    L.ggrs_wire_max_datagram_bytes.argtypes = [i32, i32]
    L.ggrs_wire_max_datagram_bytes.restype = i32
    L.ggrs_wire_unpack.argtypes = [i32, i32, i32, i32, u32, i32, vp, i32, vp, vp, i32] + [vp] * 16
    L.ggrs_wire_pack.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, i32] + [vp] * 12 + [i32, vp, vp]
    _bound = True


def _lib_bound():
    L = _lib.lib()
    _bind(L)
    return L


def _stream(t):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _arg(t, name, dtype, shape):
    """A tensor's device pointer (None stays NULL) after checking what the kernel relies on."""
    if t is None:
        return None
    ok = ("torch." + dtype,) if dtype != "int16" else ("torch.int16", "torch.uint16")
    if not t.is_cuda or not t.is_contiguous() or str(t.dtype) not in ok or tuple(t.shape) != tuple(shape):
        raise _lib.InvalidRequest(_lib.GGRS_E_INVALID, f"{name} must be a contiguous {dtype} tensor {tuple(shape)} on the "
                                  f"device, got {t.dtype} {tuple(t.shape)}")
    return ctypes.c_void_p(t.data_ptr())


def max_datagram_bytes(num_statuses, body_bytes):
    """A dgram_stride every Input message of num_statuses connect statuses and body_bytes bytes fits:
    31 + 5 num_statuses + body_bytes rounded up to a multiple of 16."""
    return int(_lib_bound().ggrs_wire_max_datagram_bytes(num_statuses, body_bytes))


def unpack(dgrams, dgram_len, now_ms, num_statuses, remote_mask, packet_stride, first_call=0, want=None, out=None):
    """dgrams [n][M][S][dgram_stride] uint8, dgram_len [n][M][S] int32 (<= 0: empty slot), now_ms [n]
    int64 (the host's millis_since_epoch at each poll), all on the device -> a dict of device tensors,
    one row per (call, session), the slots of a poll folded in slot order as handle_message would be
    called on them: slot_status [n][M][S]; start_frame, packet_len, packets [n][S][packet_stride] and
    events for receive_packets; ack_in for emit_packets; disc_mask and last_frame [n][num_statuses][S];
    notes for SpectatorEngine.receive_packets (first_call rotates them); remote_advantage and rtt_ms for
    time_sync; ping [n][S][16] for the reply; report_frame and report_checksum (int16: the u16's bits)
    for add_remote_reports; kinds.  want: the names to produce (default all; the others are not
    computed); out: a dict of tensors to fill instead of allocating."""
    import torch
    L = _lib_bound()
    if dgrams.dim() != 4:
        raise _lib.InvalidRequest(_lib.GGRS_E_INVALID, "dgrams must be [n][M][S][dgram_stride]")
    n, M, S, dstride = (int(x) for x in dgrams.shape)
    names = [name for name, _, _ in UNPACK_OUTPUTS]
    want = set(names if want is None else want)
    if want - set(names):
        raise _lib.InvalidRequest(_lib.GGRS_E_INVALID, f"unknown outputs {sorted(want - set(names))}")
    res, ptrs = {}, []
    for name, dtype, shape in UNPACK_OUTPUTS:
        t = None
        if name in want:
            shp = shape(n, M, S, num_statuses, packet_stride)
            t = out[name] if out is not None and name in out else torch.empty(shp, dtype=getattr(torch, dtype),
                                                                              device=dgrams.device)
            res[name] = t
            ptrs.append(_arg(t, name, dtype, shp))
        else:
            ptrs.append(None)
    _lib.check(L.ggrs_wire_unpack(n, S, M, num_statuses, remote_mask, first_call,
                                  _arg(dgrams, "dgrams", "uint8", (n, M, S, dstride)), dstride,
                                  _arg(dgram_len, "dgram_len", "int32", (n, M, S)), _arg(now_ms, "now_ms", "int64", (n,)),
                                  packet_stride, *ptrs, _stream(dgrams)))
    return res


def pack(magic, now_ms, num_statuses, packet_stride, dgram_stride=None, out=None, **arrays):
    """The engines' output arrays of n calls -> (dgrams [n][4][S][dgram_stride] uint8, dgram_len
    [n][4][S] int32): unpack's input with M = 4.  magic [S] int16 (the u16's bits), now_ms [n] int64;
    the keyword arrays are [n][S] device tensors, each optional (absent): start_frame, packet_len,
    ack_frame, packets [n][S][packet_stride] (emit_packets' outputs); disc_mask, last_frame
    [n][num_statuses][S], disconnect_requested; send_ack; send_report and local_advantage (time_sync's);
    kinds and ping [n][S][16] (unpack's); report_frame, report_checksum (int16); keep_alive.  Slot 0:
    Input, else InputAck when send_ack, else KeepAlive when keep_alive and nothing else goes out; 1:
    QualityReport; 2: QualityReply; 3: ChecksumReport.  dgram_stride defaults to
    max_datagram_bytes(num_statuses, packet_stride); out: (dgrams, dgram_len) to fill."""
    import torch
    L = _lib_bound()
    n, S = int(now_ms.shape[0]), int(magic.shape[0])
    unknown = set(arrays) - {name for name, _ in PACK_INPUTS}
    if unknown:
        raise _lib.InvalidRequest(_lib.GGRS_E_INVALID, f"unknown inputs {sorted(unknown)}")
    if dgram_stride is None:
        dgram_stride = max_datagram_bytes(num_statuses, packet_stride)
    if out is None:
        out = (torch.empty((n, PACK_SLOTS, S, dgram_stride), dtype=torch.uint8, device=magic.device),
               torch.empty((n, PACK_SLOTS, S), dtype=torch.int32, device=magic.device))
    shapes = {"packets": (n, S, packet_stride), "last_frame": (n, num_statuses, S), "ping": (n, S, 16)}
    ptrs = {name: _arg(arrays.get(name), name, dtype, shapes.get(name, (n, S))) for name, dtype in PACK_INPUTS}
    order = [name for name, _ in PACK_INPUTS]
    _lib.check(L.ggrs_wire_pack(n, S, num_statuses, _arg(magic, "magic", "int16", (S,)),
                                _arg(now_ms, "now_ms", "int64", (n,)), *(ptrs[k] for k in order[:4]), packet_stride,
                                *(ptrs[k] for k in order[4:]),
                                _arg(out[0], "dgrams", "uint8", (n, PACK_SLOTS, S, dgram_stride)), dgram_stride,
                                _arg(out[1], "dgram_len", "int32", (n, PACK_SLOTS, S)), _stream(magic)))
    return out
