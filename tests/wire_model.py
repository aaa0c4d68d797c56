"""A Python model of the GGRS wire envelope (ggrs_wire_unpack / ggrs_wire_pack, csrc/wire.hip).

What a socket hands a GGRS 0.10.2 host is `bincode::serialize(&Message)` (src/network/udp_socket.rs,
src/network/messages.rs:5-129).  bincode 1.3's top-level serialize: fixed-width little-endian integers,
a u32 enum tag, a u64 Vec length, a bool as one byte that must be 0 or 1, a u128 as 16 bytes; fields in
declaration order; bytes after a complete value are accepted.

    Message           = magic u16 | tag u32 | body
    Input (0)         = n u64 | n x (disconnected u8, last_frame i32) | disconnect_requested u8
                        | start_frame i32 | ack_frame i32 | len u64 | bytes[len]
    InputAck (1)      = ack_frame i32
    QualityReport (2) = frame_advantage i16 | ping u128
    QualityReply (3)  = pong u128
    ChecksumReport (4)= checksum u128 | frame i32
    KeepAlive (5)     = nothing

Three layers, each restating the one below in other words so that they can be held to each other:
  * serialize / deserialize: one Message <-> bytes;
  * Endpoint: the literal fold, handle_message (protocol.rs:534-562) applied to every message of a poll
    in order, on a small endpoint state (pending pops, connect status, advantage, rtt, pending
    checksums);
  * unpack_poll / pack_call: the device unit's reductions of a poll's slots to one row of the dense
    arrays the engines take, and its fixed slots on the way out.

There is no Rust toolchain here and the reference has no serialized-Message vectors, so the layout is
pinned by hand-derived bytes (tests/test_wire_model.py) and by this restatement.
"""
import struct
from collections import namedtuple

NULL_FRAME = -1
INPUT, INPUT_ACK, QUALITY_REPORT, QUALITY_REPLY, CHECKSUM_REPORT, KEEP_ALIVE = range(6)
E_BINCODE, E_SHAPE, E_CAP, E_CLOCK, E_RANGE = -22, -23, -24, -25, -26
TIME_SYNC_KEEP = -2 ** 31
INT32_MAX = 2 ** 31 - 1
PACK_SLOTS = 4

Input = namedtuple("Input", "status disconnect_requested start_frame ack_frame data")  # status: [(bool, i32)]
InputAck = namedtuple("InputAck", "ack_frame")
QualityReport = namedtuple("QualityReport", "frame_advantage ping")
QualityReply = namedtuple("QualityReply", "pong")
ChecksumReport = namedtuple("ChecksumReport", "checksum frame")
KeepAlive = namedtuple("KeepAlive", "")
Message = namedtuple("Message", "magic body")
BODIES = (Input, InputAck, QualityReport, QualityReply, ChecksumReport, KeepAlive)


class BincodeError(Exception):
    pass


def max_datagram_bytes(num_statuses, body_bytes):
    """ggrs_wire_max_datagram_bytes: the longest Input message, rounded up to a multiple of 16"""
    return (31 + 5 * num_statuses + body_bytes + 15) // 16 * 16


def _u128(v):
    return int(v).to_bytes(16, "little")


def serialize(msg):
    """bincode::serialize(&Message)"""
    b = msg.body
    tag = BODIES.index(type(b))
    out = struct.pack("<HI", msg.magic, tag)
    if tag == INPUT:
        out += struct.pack("<Q", len(b.status))
        for disconnected, last_frame in b.status:
            out += struct.pack("<Bi", int(bool(disconnected)), last_frame)
        out += struct.pack("<BiiQ", int(bool(b.disconnect_requested)), b.start_frame, b.ack_frame, len(b.data))
        out += bytes(b.data)
    elif tag == INPUT_ACK:
        out += struct.pack("<i", b.ack_frame)
    elif tag == QUALITY_REPORT:
        out += struct.pack("<h", b.frame_advantage) + _u128(b.ping)
    elif tag == QUALITY_REPLY:
        out += _u128(b.pong)
    elif tag == CHECKSUM_REPORT:
        out += _u128(b.checksum) + struct.pack("<i", b.frame)
    return out


class _Reader:
    def __init__(self, data):
        self.d, self.at = bytes(data), 0

    def take(self, n):
        if n > len(self.d) - self.at:
            raise BincodeError("unexpected end of input")
        v = self.d[self.at:self.at + n]
        self.at += n
        return v

    def num(self, fmt):
        return struct.unpack("<" + fmt, self.take(struct.calcsize("<" + fmt)))[0]

    def boolean(self):
        v = self.take(1)[0]
        if v > 1:
            raise BincodeError("invalid bool byte %d" % v)
        return bool(v)

    def u128(self):
        return int.from_bytes(self.take(16), "little")


def deserialize(data):
    """bincode::deserialize::<Message>: a Message, or BincodeError.  Trailing bytes are accepted."""
    r = _Reader(data)
    magic, tag = r.num("H"), r.num("I")
    if tag == INPUT:
        n = r.num("Q")
        status = []
        for _ in range(n):  # (an absurd n runs out of bytes at once: five bytes an element)
            status.append((r.boolean(), r.num("i")))
        dr, start, ack, m = r.boolean(), r.num("i"), r.num("i"), r.num("Q")
        body = Input(status, dr, start, ack, r.take(m))
    elif tag == INPUT_ACK:
        body = InputAck(r.num("i"))
    elif tag == QUALITY_REPORT:
        body = QualityReport(r.num("h"), r.u128())
    elif tag == QUALITY_REPLY:
        body = QualityReply(r.u128())
    elif tag == CHECKSUM_REPORT:
        ck = r.u128()
        body = ChecksumReport(ck, r.num("i"))
    elif tag == KEEP_ALIVE:
        body = KeepAlive()
    else:
        raise BincodeError("enum tag %d" % tag)
    return Message(magic, body)


def classify(data, length, dgram_stride, num_statuses, packet_stride, now_ms):
    """One slot -> (slot status, Message or None).  length <= 0: empty (0).  The bincode checks come
    first (a length beyond the row is one of them), then the unit's own: too few connect statuses
    (E_SHAPE), bytes longer than a packet row (E_CAP), a pong from the future (E_CLOCK), a checksum
    wider than the engine's 16 bits (E_RANGE).  Accepted: tag + 1."""
    if length <= 0:
        return 0, None
    if length > dgram_stride:
        return E_BINCODE, None
    try:
        msg = deserialize(bytes(data[:length]))
    except BincodeError:
        return E_BINCODE, None
    b = msg.body
    if isinstance(b, Input):
        if len(b.status) < num_statuses:
            return E_SHAPE, None
        if len(b.data) > packet_stride:
            return E_CAP, None
    elif isinstance(b, QualityReply):
        if b.pong > now_ms:  # (covers any of the upper 64 bits: now_ms is a u64)
            return E_CLOCK, None
    elif isinstance(b, ChecksumReport):
        if b.checksum >= 1 << 16:
            return E_RANGE, None
    return BODIES.index(type(b)) + 1, msg


def spectator_note(player, frame):
    """GGRS_SPECTATOR_NOTE in the device's 32-bit arithmetic (a hostile last_frame wraps)"""
    v = (1 | player << 1 | ((frame + 1) & 0xFFFFFFFF) << 3) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


class Endpoint:
    """handle_message's effects (protocol.rs:534-682) on what the device units take over: the literal
    fold the reductions of unpack_poll are held to."""

    def __init__(self, num_statuses, pending=()):
        self.pending = list(pending)  # the frames of pending_output, ascending
        self.status = [[False, NULL_FRAME] for _ in range(num_statuses)]
        self.disconnect_event = False
        self.remote_frame_advantage = None
        self.round_trip_time = None
        self.replies = []  # the pongs queued
        self.pending_checksums = {}
        self.inputs = []  # (start_frame, bytes) of every Input, in arrival order

    def pop_pending_output(self, ack_frame):  # :378-391
        while self.pending and self.pending[0] <= ack_frame:
            self.pending.pop(0)

    def handle_message(self, msg, now_ms):
        b = msg.body
        if isinstance(b, Input):  # on_input :564-585, then the decode the packet feed owns
            self.pop_pending_output(b.ack_frame)
            if b.disconnect_requested:
                self.disconnect_event = True
            else:
                for i, st in enumerate(self.status):
                    st[0] = b.status[i][0] or st[0]
                    st[1] = max(st[1], b.status[i][1])
            self.inputs.append((b.start_frame, b.data))
        elif isinstance(b, InputAck):  # :644-646
            self.pop_pending_output(b.ack_frame)
        elif isinstance(b, QualityReport):  # :649-653
            self.remote_frame_advantage = b.frame_advantage
            self.replies.append(b.ping)
        elif isinstance(b, QualityReply):  # :656-660
            assert now_ms >= b.pong
            self.round_trip_time = now_ms - b.pong
        elif isinstance(b, ChecksumReport):  # :663-682 (the 32-entry pruning is the compare unit's)
            self.pending_checksums[b.frame] = b.checksum


def unpack_poll(slots, dgram_stride, num_statuses, remote_mask, call, packet_stride, now_ms):
    """One (call, session): slots = [(bytes, length)] in slot order -> the row of every output array.
    `call` is first_call + i, which rotates the spectator note."""
    out = dict(slot_status=[], start_frame=-1, packet_len=0, packet=b"", ack_in=NULL_FRAME, events=0, disc_mask=0,
               last_frame=[NULL_FRAME] * num_statuses, notes=0, remote_advantage=TIME_SYNC_KEEP, ping=None,
               rtt_ms=-1, report_frame=NULL_FRAME, report_checksum=0, kinds=0)
    have_input = have_report = False
    for data, length in slots:
        st, msg = classify(data, length, dgram_stride, num_statuses, packet_stride, now_ms)
        out["slot_status"].append(st)
        if msg is None:
            continue
        b = msg.body
        out["kinds"] |= 1 << (st - 1)
        if isinstance(b, Input):
            out["ack_in"] = max(out["ack_in"], b.ack_frame)
            if b.disconnect_requested:
                out["events"] = remote_mask
            else:
                for i in range(num_statuses):
                    out["disc_mask"] |= int(b.status[i][0]) << i
                    out["last_frame"][i] = max(out["last_frame"][i], b.status[i][1])
            if not have_input or b.start_frame >= out["start_frame"]:  # the greatest start, ties to the later
                have_input = True
                out["start_frame"], out["packet_len"], out["packet"] = b.start_frame, len(b.data), bytes(b.data)
        elif isinstance(b, InputAck):
            out["ack_in"] = max(out["ack_in"], b.ack_frame)
        elif isinstance(b, QualityReport):
            out["remote_advantage"], out["ping"] = b.frame_advantage, _u128(b.ping)
        elif isinstance(b, QualityReply):
            out["rtt_ms"] = min(now_ms - b.pong, INT32_MAX)
        elif isinstance(b, ChecksumReport):
            if not have_report or b.frame >= out["report_frame"]:
                have_report = True
                out["report_frame"], out["report_checksum"] = b.frame, b.checksum
    players = [k for k in range(num_statuses) if out["disc_mask"] >> k & 1]
    if players:
        k = players[call % len(players)]
        out["notes"] = spectator_note(k, out["last_frame"][k])
    return out


def clamp_i16(v):
    return max(-32768, min(32767, v))


def pack_call(magic, now_ms, num_statuses, packet_stride, start_frame=None, packet_len=None, ack_frame=None,
              packet=None, disc_mask=None, last_frame=None, disconnect_requested=None, send_ack=None,
              send_report=None, local_advantage=None, kinds=None, ping=None, report_frame=None,
              report_checksum=None, keep_alive=None):
    """One (call, session) -> the four datagrams (b"" = empty slot).  None = the array is absent.
    An Input needs start_frame, packet_len and packets present, start_frame >= 0 and
    0 < packet_len <= packet_stride."""
    out = [b""] * PACK_SLOTS
    ack = NULL_FRAME if ack_frame is None else ack_frame
    if (start_frame is not None and packet_len is not None and packet is not None and start_frame >= 0
            and 0 < packet_len <= packet_stride):
        status = [(bool((disc_mask or 0) >> k & 1), NULL_FRAME if last_frame is None else last_frame[k])
                  for k in range(num_statuses)]
        out[0] = serialize(Message(magic, Input(status, bool(disconnect_requested), start_frame, ack,
                                                 bytes(packet[:packet_len]))))
    elif send_ack:
        out[0] = serialize(Message(magic, InputAck(ack)))
    if send_report:
        out[1] = serialize(Message(magic, QualityReport(clamp_i16(local_advantage or 0), now_ms)))
    if kinds is not None and kinds >> QUALITY_REPORT & 1:
        out[2] = serialize(Message(magic, QualityReply(int.from_bytes(bytes(ping), "little") if ping is not None else 0)))
    if report_frame is not None and report_frame >= 0:
        out[3] = serialize(Message(magic, ChecksumReport(report_checksum or 0, report_frame)))
    if keep_alive and not any(out):
        out[0] = serialize(Message(magic, KeepAlive()))
    return out


# ---- traffic for the tests (CPU and GPU share it)

def random_message(rng, tag, num_statuses, max_body, now_ms=1 << 40, magic=None, extra_statuses=0):
    """A valid message of `tag` that classify accepts under (num_statuses, packet_stride >= max_body, now_ms)."""
    magic = int(rng.integers(0, 1 << 16)) if magic is None else magic
    frame = lambda: int(rng.integers(-1, 1 << 20))  # noqa: E731
    if tag == INPUT:
        status = [(bool(rng.integers(0, 2)), frame()) for _ in range(num_statuses + extra_statuses)]
        data = rng.integers(0, 256, int(rng.integers(0, max_body + 1)), dtype="uint8").tobytes()
        body = Input(status, bool(rng.random() < 0.1), frame(), frame(), data)
    elif tag == INPUT_ACK:
        body = InputAck(frame())
    elif tag == QUALITY_REPORT:
        body = QualityReport(int(rng.integers(-32768, 32768)), int(rng.integers(0, 1 << 62)) << int(rng.integers(0, 66)) & (1 << 128) - 1)
    elif tag == QUALITY_REPLY:
        body = QualityReply(now_ms - int(rng.integers(0, 1 << int(rng.integers(1, 40)))))
    elif tag == CHECKSUM_REPORT:
        body = ChecksumReport(int(rng.integers(0, 1 << 16)), frame())
    else:
        body = KeepAlive()
    return Message(magic, body)


def known_answers():
    """The issue's six hand-derived serializations with magic 0x1234: (Message, bytes)."""
    z14 = bytes(14)
    return [
        (Message(0x1234, KeepAlive()), bytes.fromhex("34 12 05 00 00 00")),
        (Message(0x1234, InputAck(7)), bytes.fromhex("34 12 01 00 00 00 07 00 00 00")),
        (Message(0x1234, QualityReport(-3, 0x0102)), bytes.fromhex("34 12 02 00 00 00 fd ff 02 01") + z14),
        (Message(0x1234, QualityReply(0x0102)), bytes.fromhex("34 12 03 00 00 00 02 01") + z14),
        (Message(0x1234, ChecksumReport(0xBEEF, 20)), bytes.fromhex("34 12 04 00 00 00 ef be") + z14 + bytes.fromhex("14 00 00 00")),
        (Message(0x1234, Input([(False, -1), (True, 5)], False, 3, 2, b"\xaa\xbb")),
         bytes.fromhex("34 12 00 00 00 00 02 00 00 00 00 00 00 00 00 ff ff ff ff 01 05 00 00 00 00 03 00 00 00 02 00 00 00"
                       " 02 00 00 00 00 00 00 00 aa bb")),
    ]


def hostile_cases(num_statuses=2, packet_stride=16, now_ms=1 << 40):
    """(name, datagram bytes, the slot status classify must give) under the given shape: every way a
    datagram is refused, and the accepted neighbours of each (trailing bytes, a long status vector)."""
    ok_input = Message(7, Input([(False, 4), (True, 9)][:num_statuses] + [(False, 1)] * max(0, num_statuses - 2),
                                False, 3, 2, b"\x01\x02\x03"))
    raw = serialize(ok_input)
    n_at, len_at = 6, 14 + 5 * num_statuses + 9
    cases = []
    for msg, data in known_answers():
        tag = BODIES.index(type(msg.body))
        for cut in range(1, len(data)):
            cases.append(("truncated tag %d at %d" % (tag, cut), data[:cut], E_BINCODE))
        want = tag + 1 if tag != INPUT or num_statuses <= 2 else E_SHAPE
        cases.append(("trailing bytes tag %d" % tag, data + b"\xee" * 5, want))
    cases.append(("tag 6", struct.pack("<HI", 1, 6) + bytes(20), E_BINCODE))
    cases.append(("tag 2^31", struct.pack("<HI", 1, 1 << 31) + bytes(20), E_BINCODE))
    cases.append(("status bool 2", raw[:14] + b"\x02" + raw[15:], E_BINCODE))
    cases.append(("disconnect_requested bool 2", raw[:14 + 5 * num_statuses] + b"\x02" + raw[15 + 5 * num_statuses:], E_BINCODE))
    for big in (0xFFFFFFFFFFFFFFFF, 0x100000002):
        cases.append(("status count %x" % big, raw[:n_at] + struct.pack("<Q", big) + raw[n_at + 8:], E_BINCODE))
        cases.append(("bytes length %x" % big, raw[:len_at] + struct.pack("<Q", big) + raw[len_at + 8:], E_BINCODE))
    cases.append(("bytes length one too many", raw[:len_at] + struct.pack("<Q", 4) + raw[len_at + 8:], E_BINCODE))
    short = ok_input.body._replace(status=ok_input.body.status[:num_statuses - 1])
    cases.append(("short status vector", serialize(Message(7, short)), E_SHAPE))
    long_ = ok_input.body._replace(status=ok_input.body.status + [(True, 77), (False, 3)])
    cases.append(("long status vector", serialize(Message(7, long_)), INPUT + 1))
    cases.append(("long status vector, ignored bool 3",
                  serialize(Message(7, long_)).replace(struct.pack("<Bi", 1, 77), struct.pack("<Bi", 3, 77)), E_BINCODE))
    cases.append(("bytes at the cap", serialize(Message(7, ok_input.body._replace(data=bytes(range(packet_stride))))), INPUT + 1))
    cases.append(("bytes over the cap", serialize(Message(7, ok_input.body._replace(data=bytes(packet_stride + 1)))), E_CAP))
    cases.append(("pong now", serialize(Message(7, QualityReply(now_ms))), QUALITY_REPLY + 1))
    cases.append(("pong from the future", serialize(Message(7, QualityReply(now_ms + 1))), E_CLOCK))
    cases.append(("pong upper bits", serialize(Message(7, QualityReply(1 << 64))), E_CLOCK))
    cases.append(("pong top bit", serialize(Message(7, QualityReply(1 << 127))), E_CLOCK))
    cases.append(("checksum 16 bits", serialize(Message(7, ChecksumReport(0xFFFF, 40))), CHECKSUM_REPORT + 1))
    cases.append(("checksum 17 bits", serialize(Message(7, ChecksumReport(0x10000, 40))), E_RANGE))
    cases.append(("checksum upper bits", serialize(Message(7, ChecksumReport(1 << 100, 40))), E_RANGE))
    return cases


# ---- whole batches, as numpy arrays in the device unit's layouts

def slots_to_arrays(polls, M, S, dgram_stride):
    """polls[i][m][s] = a datagram's bytes, or (bytes, stated length) -> (dgrams [n][M][S][stride] u8,
    dgram_len [n][M][S] i32); bytes beyond the row are cut, the stated length kept."""
    import numpy as np
    n = len(polls)
    dgrams = np.zeros((n, M, S, dgram_stride), np.uint8)
    lens = np.zeros((n, M, S), np.int32)
    for i in range(n):
        for m in range(M):
            for s in range(S):
                d = polls[i][m][s]
                d, ln = d if isinstance(d, tuple) else (d, len(d))
                k = min(len(d), dgram_stride)
                dgrams[i, m, s, :k] = np.frombuffer(d[:k], np.uint8)
                lens[i, m, s] = ln
    return dgrams, lens


def unpack_batch(dgrams, lens, now_ms, num_statuses, remote_mask, first_call, packet_stride):
    """unpack_poll over every (call, session) -> the output arrays of ggrs_wire_unpack (packets zero
    past packet_len, ping zero without a report)."""
    import numpy as np
    n, M, S, dstride = dgrams.shape
    i32 = lambda *shape, fill=0: np.full(shape, fill, np.int32)  # noqa: E731
    out = dict(slot_status=i32(n, M, S), start_frame=i32(n, S), packet_len=i32(n, S),
               packets=np.zeros((n, S, packet_stride), np.uint8), ack_in=i32(n, S), events=np.zeros((n, S), np.uint8),
               disc_mask=np.zeros((n, S), np.uint8), last_frame=i32(n, num_statuses, S), notes=i32(n, S),
               remote_advantage=i32(n, S), ping=np.zeros((n, S, 16), np.uint8), rtt_ms=i32(n, S),
               report_frame=i32(n, S), report_checksum=np.zeros((n, S), np.uint16), kinds=np.zeros((n, S), np.uint8))
    for i in range(n):
        for s in range(S):
            slots = [(dgrams[i, m, s].tobytes(), int(lens[i, m, s])) for m in range(M)]
            r = unpack_poll(slots, dstride, num_statuses, remote_mask, first_call + i, packet_stride, int(now_ms[i]))
            out["slot_status"][i, :, s] = r["slot_status"]
            out["packets"][i, s, :r["packet_len"]] = np.frombuffer(r["packet"], np.uint8)
            out["last_frame"][i, :, s] = r["last_frame"]
            if r["ping"] is not None:
                out["ping"][i, s] = np.frombuffer(r["ping"], np.uint8)
            for k in ("start_frame", "packet_len", "ack_in", "events", "disc_mask", "notes", "remote_advantage", "rtt_ms",
                      "report_frame", "report_checksum", "kinds"):
                out[k][i, s] = r[k]
    return out


def pack_batch(magic, now_ms, num_statuses, packet_stride, dgram_stride, **arrays):
    """pack_call over every (call, session): arrays as ggrs_wire_pack takes them ([n][S]; packets
    [n][S][stride], last_frame [n][ns][S], ping [n][S][16]), an absent one left out -> (dgrams
    [n][4][S][dgram_stride] zero past each length, dgram_len [n][4][S])."""
    import numpy as np
    n, S = len(now_ms), len(magic)
    polls = [[[b""] * S for _ in range(PACK_SLOTS)] for _ in range(n)]
    for i in range(n):
        for s in range(S):
            kw = {}
            for k, a in arrays.items():
                if k == "packets":
                    kw["packet"] = a[i, s].tobytes()
                elif k == "last_frame":
                    kw[k] = [int(x) for x in a[i, :, s]]
                elif k == "ping":
                    kw[k] = a[i, s].tobytes()
                else:
                    kw[k] = int(a[i, s])
            for m, d in enumerate(pack_call(int(magic[s]), int(now_ms[i]), num_statuses, packet_stride, **kw)):
                polls[i][m][s] = d
    return slots_to_arrays(polls, PACK_SLOTS, S, dgram_stride)
