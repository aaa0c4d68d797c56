"""Directed packets for the input wire codec (csrc/codec.hip, csrc/codec_device.h): every run length,
header width and reject edge the random suites (tests/test_gpu_codec.py, the feeds' damage cases)
reach by luck or not at all.  A helper, not a test file; numpy only, so the CPU tests
(tests/test_codec_cases.py) and the device tests (tests/test_gpu_codec_directed.py, the packet feeds')
share the same bytes.

Wire format (oracle/codec.c): u8 tag (0: input_sizes None, 1: Some), [u64 n, n x i32 size deltas],
u64 m, m bytes of runs.  A run is a LEB128 header h: h odd -> (h >> 2) bytes of 0xFF (h & 2) or 0x00;
h even -> (h >> 1) literal bytes follow.

Three parts:
  an assembler      varint / fill / lit / packet
  the cases         decode_cases(W, B), encode_cases(W, B)
  recode            a valid tag-0 packet in other bytes that decode alike (or that must be rejected)
and the codec's launch arithmetic restated (swar_ndw, *_lds, decode_form / encode_form), which is how
the tests know which kernel a shape reaches: the ABI does not say.
"""
import struct

import numpy as np

OK, E_BINCODE, E_RLE, E_DELTA, E_CAP, E_INVALID, UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6
VERDICTS = (OK, E_BINCODE, E_RLE, E_DELTA, E_CAP, E_INVALID, UNSUPPORTED)
MAX_DECODED = 1 << 24  # oracle/codec.c CODEC_MAX_DECODED, codec_device.h kMaxDecoded
INT32_MIN = -2 ** 31

# the shapes (W, B) of the device test, by the kernel the default form's DECODE reaches at the default
# stride (decode_form below; tests/test_codec_cases.py asserts this table):
SHAPES = (
    (1, 4), (8, 1), (12, 1), (3, 4), (5, 4), (16, 2),  # run-level, 32-bit masks (NDW 1, 2, 4, 4, 8, 8)
    (32, 2), (16, 4), (64, 1),                         # run-level, 64-bit masks (NDW 16)
    (4, 3), (8, 8),                                    # staged: B outside {1, 2, 4}, whole dwords
    (20, 4), (21, 4),                                  # staged, W*B > 64; (21, 4) is the last under the LDS budget
    (22, 4),                                           # direct under every form: the first over the budget
    (1, 7), (33, 4),                                   # direct: rows not whole dwords / far over the budget
)


# ---- the launch arithmetic of csrc/codec.hip, restated

LDS_BUDGET = 64 * 1024  # kLdsBudget
BLOCK = 256


def max_packet_bytes(B, W):
    """ggrs_codec_max_packet_bytes"""
    L = B * W
    return (1 + 8 + L + (L + 1) // 2 + 10 + 15) // 16 * 16


def odd_dword_pitch(n):
    dw = (n + 3) // 4
    return 4 * (dw + 1 if dw % 2 == 0 else dw)


def swar_ndw(B, W, stride):
    WB = W * B
    if B not in (1, 2, 4) or WB <= 0 or WB > 64 or WB % 4 or stride % 4:
        return 0
    n = 1
    while 4 * n < WB:
        n <<= 1
    return n


def scratch_bytes(W, B):
    """K: the run-level decoder's scratch row (4 * NDW), or W * B where that form does not apply."""
    return 4 * swar_ndw(B, W, 0) or W * B


def decode_swar_lds(ndw, stride):
    return BLOCK * (odd_dword_pitch(stride) + odd_dword_pitch(4 * ndw))


def encode_swar_lds(ndw, stride, chunked=False):
    row = 9 + 12 * ndw
    in_place = (row + 3) // 4 <= 16
    return BLOCK * (odd_dword_pitch(max(stride, row)) + odd_dword_pitch(4 * ndw)
                    + (stride if chunked and not in_place else 0))


def staged_lds(B, W, stride):
    """encode_lds_bytes == decode_lds_bytes; 0: the staged form does not apply"""
    if (W * B) % 4 or stride % 4 or W * B == 0:
        return 0
    return BLOCK * (odd_dword_pitch(W * B) + odd_dword_pitch(stride) + B)


def _form(swar_lds, B, W, stride, form):
    ndw = swar_ndw(B, W, stride)
    if form == "default" and ndw and swar_lds(ndw, stride) <= LDS_BUDGET:
        return "run-level"
    lds = staged_lds(B, W, stride)
    return "staged" if lds and lds <= LDS_BUDGET and form != "direct" else "direct"


def decode_form(W, B, stride=None, form="default"):
    """The kernel ggrs_codec_decode launches for dword-aligned buffers: run-level / staged / direct."""
    return _form(decode_swar_lds, B, W, stride or max_packet_bytes(B, W), form)


def encode_form(W, B, stride=None, form="default"):
    return _form(encode_swar_lds, B, W, stride or max_packet_bytes(B, W), form)


def chunked_ok(W, B, stride, encode=False):
    """Whether ggrs_codec_decode_chunked / _encode_chunked take the shape."""
    ndw = swar_ndw(B, W, stride)
    if not ndw:
        return False
    return (encode_swar_lds(ndw, stride, True) if encode else decode_swar_lds(ndw, stride)) <= LDS_BUDGET


def wide_stride(W, B, need):
    """The second decode stride: `need` rounded up to a dword and wider than the default, clipped to
    the widest row at which the run-level decoder still fits its LDS where that form applies."""
    s = max((need + 3) // 4 * 4, max_packet_bytes(B, W) + 12)
    ndw = swar_ndw(B, W, 0)
    if ndw:
        while decode_swar_lds(ndw, s) > LDS_BUDGET:
            s -= 4
    return s


# ---- the assembler

def varint(v, pad=0):
    """LEB128 of v; pad > 0 appends that many redundant bytes (0x80 ... 0x00) that add nothing."""
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            break
    if pad:
        out[-1] |= 0x80
        out += b"\x80" * (pad - 1) + b"\x00"
    return bytes(out)


def fill(n, ff=False, pad=0):
    return varint((n << 2) | (2 if ff else 0) | 1, pad)


def lit(data, pad=0, claim=None):
    data = bytes(data)
    return varint((len(data) if claim is None else claim) << 1, pad) + data


def packet(runs, sizes=None, m=None, tail=b"", tag=None, n_sizes=None):
    """runs: bytes or a list of runs.  sizes: the i32 size deltas of input_sizes = Some(..); m, tag and
    n_sizes override what the fields would say."""
    stream = runs if isinstance(runs, (bytes, bytearray)) else b"".join(runs)
    out = bytearray([(0 if sizes is None else 1) if tag is None else tag])
    if sizes is not None:
        out += struct.pack("<Q", len(sizes) if n_sizes is None else n_sizes)
        out += b"".join(struct.pack("<i", s) for s in sizes)
    out += struct.pack("<Q", len(stream) if m is None else m) + stream + tail
    return bytes(out)


# ---- decode cases

def _stream_intent(total, W, B):
    """A tag-0 packet whose runs parse and expand to `total` bytes."""
    if total % B:
        return E_DELTA
    return E_CAP if total // B > W else OK


def decode_cases(W, B, stride=None):
    """[(name, intent, ref_bytes, packet_bytes, length)].  intent: the verdict the case is built to
    reach when its row holds it; `stride` (default: the ABI's) only places the lengths outside the row.
    packet_bytes may be longer than length (junk in the row) and length may lie outside the row."""
    WB, K = W * B, scratch_bytes(W, B)
    stride = stride or max_packet_bytes(B, W)
    rng = np.random.default_rng(7919 * W + B)
    cases = []

    def rb(n, lo=0, hi=256):
        return rng.integers(lo, hi, n, dtype=np.uint8).tobytes()

    def add(name, intent, pk, length=None):
        i = len(cases)
        ref = (bytes(B), b"\xff" * B, rb(B), rb(B, 1, 255))[i % 4]
        cases.append((name, intent, ref, pk, len(pk) if length is None else length))

    def runs_of(segments):
        """[(class, n)] -> (runs, total): 'z' 0x00 fill, 'f' 0xFF fill, 'l' literal."""
        out = []
        for cls, n in segments:
            out.append(lit(rb(n, 1, 255)) if cls == "l" else fill(n, cls == "f"))
        return out, sum(n for _, n in segments)

    # single runs
    fills = sorted({0, 1, B, 31, 32, 33, 63, 64, 65, 127, 128, WB - 1, WB, WB + 1, K - 1, K, K + 1, WB + B})
    for n in fills:
        for ff in (False, True):
            for pad in (0, 1 + n % 3):
                add(f"fill{'FF' if ff else '00'}_{n}_pad{pad}", _stream_intent(n, W, B), packet(fill(n, ff, pad)))
    for n in sorted({0, 1, B, 63, 64, WB - 1, WB, WB + 1, K, K + 1}):
        add(f"lit_{n}", _stream_intent(n, W, B), packet(lit(rb(n), n % 2)))
        add(f"lit_{n}_claims_{n + 1}", E_RLE, packet(lit(rb(n), 0, claim=n + 1)))

    # composite streams
    for T in sorted({WB, WB + 1, K, K + 1}):
        intent = _stream_intent(T, W, B)
        for a in "zfl":
            for b in "zfl":
                if a == b:
                    runs, _ = runs_of([(a, T // 2), (a, T - T // 2)])
                    add(f"adjacent_{a}{a}_{T}", intent, packet(runs))
                    continue
                for s in sorted({1, 3, 4, 5, 31, 32, 33, WB - 1}):
                    if 0 < s < T:
                        runs, _ = runs_of([(a, s), (b, T - s)])
                        add(f"pair_{a}{b}_{s}_of_{T}", intent, packet(runs))
        runs, _ = runs_of([("l", 1), ("z", 0), ("f", 0), ("l", 0), ("f", T - 2), ("l", 0), ("z", 1), ("f", 0)])  # T >= 4
        add(f"zero_length_runs_{T}", intent, packet(runs))
        body = bytearray(rb(T))
        body[::3] = b"\x00" * len(body[::3])
        body[1::3] = b"\xff" * len(body[1::3])
        add(f"literal_with_00_FF_{T}", intent, packet(lit(body)))
        alt = [lit(rb(1, 1, 255)) if i % 2 == 0 else fill(1, i % 4 == 3) for i in range(T)]
        add(f"alternating_{T}", intent, packet(alt))

    # varints
    whole = _stream_intent(WB, W, B)
    add("header_10_bytes_fill", whole, packet(fill(WB, True, 10 - len(fill(WB, True)))))
    add("header_10_bytes_literal", whole, packet(lit(rb(WB), 10 - len(varint(WB << 1)))))
    add("header_11_bytes", E_RLE, packet(fill(WB, True, 11 - len(fill(WB, True)))))
    h = bytearray(fill(WB, True))  # a tenth byte whose bits lie past bit 63 add nothing
    h[-1] |= 0x80
    add("header_bits_past_63", whole, packet(bytes(h) + b"\x80" * (9 - len(h)) + b"\x7e"))
    add("header_ff9_01", E_RLE, packet(b"\xff" * 9 + b"\x01"))
    add("header_cut_by_m", E_RLE, packet(fill(WB, False, 3), m=len(fill(WB)) + 1))
    add("header_alone_continues", E_RLE, packet(fill(WB) + b"\x80"))

    # the kMaxDecoded edge
    add("fill_2^24", _stream_intent(MAX_DECODED, W, B), packet(fill(MAX_DECODED)))
    add("fill_2^24+1", E_RLE, packet(fill(MAX_DECODED + 1, True)))
    add("fills_2^23_2^23_B", E_RLE, packet([fill(1 << 23), fill(1 << 23, True), fill(B)]))
    add("literal_claims_2^24+1", E_RLE, packet(lit(rb(3), 0, claim=MAX_DECODED + 1)))

    # framing
    good = packet(runs_of([("l", 1), ("f", WB - 1)])[0]) if WB > 1 else packet(lit(rb(1, 1, 255)))
    for n in range(10):
        add(f"length_{n}", E_BINCODE, good, n)
    add("empty_stream", OK, packet(b""))
    add("tag_2", E_BINCODE, packet(fill(WB), tag=2))
    add("tag_255", E_BINCODE, packet(fill(WB), tag=255))
    add("m_past_the_packet", E_BINCODE, packet(fill(WB), m=len(fill(WB)) + 1))
    add("m_2^63", E_BINCODE, packet(fill(WB), m=1 << 63))
    add("junk_after_m", whole, packet(fill(WB, True), tail=rb(5)))
    add("junk_past_length", whole, good + rb(7), len(good))

    # input_sizes = Some(..)
    def mixed(total):
        if total < 3:
            return [lit(rb(total, 1, 255))]
        return runs_of([("l", 1), ("f", total // 2), ("z", total - 1 - total // 2)])[0]

    add("some_zero_deltas", OK, packet(mixed(WB), sizes=[0] * W))
    add("some_one_input", OK, packet(lit(rb(B)), sizes=[0]))
    add("some_none", OK, packet(b"", sizes=[]))
    add("some_one_too_many", E_CAP, packet(mixed(WB + B), sizes=[0] * (W + 1)))
    uneven = [1, -1] + [0] * (W - 2) if W > 1 else [1]
    add("some_uneven", UNSUPPORTED, packet(mixed(WB + 1), sizes=uneven))
    short = [-1, 1] + [0] * (W - 2) if W > 1 else [-1]
    add("some_uneven_short_first", UNSUPPORTED, packet(mixed(WB - 1), sizes=short))
    add("some_size_0", UNSUPPORTED, packet(b"", sizes=[-B]))
    add("some_size_2B", UNSUPPORTED, packet(mixed(2 * B), sizes=[B]))
    add("some_uneven_and_too_many", UNSUPPORTED, packet(mixed(WB + B + 1), sizes=[1, -1] + [0] * (W - 1)))
    add("some_negative_first", E_DELTA, packet(mixed(WB), sizes=[-B - 1] + [0] * (W - 1)))
    add("some_negative_later", E_DELTA, packet(mixed(WB + B), sizes=[0, -B - 1] + [0] * (W - 1)))
    add("some_i32_wrap", E_DELTA, packet(mixed(WB), sizes=[2 ** 31 - 1 - B, 1]))
    add("some_sum_over", E_DELTA, packet(mixed(WB), sizes=[0] * W + [0]))
    add("some_sum_under", E_DELTA, packet(mixed(WB + B), sizes=[0] * W))
    add("some_sum_under_by_one", E_DELTA, packet(mixed(WB + 1), sizes=[0] * W))
    add("some_n_2^62", E_BINCODE, packet(mixed(WB), sizes=[0] * W, n_sizes=1 << 62))
    body = packet(mixed(WB), sizes=[0] * W)
    fits = (len(body) - 9) // 4
    add("some_n_one_past_the_packet", E_BINCODE, packet(mixed(WB), sizes=[0] * W, n_sizes=fits + 1))
    add("some_n_takes_the_packet", E_BINCODE, packet(mixed(WB), sizes=[0] * W, n_sizes=fits))
    add("some_cut_in_n", E_BINCODE, body, 5)
    add("some_cut_in_sizes", E_BINCODE, body, 9 + 2)

    # lengths outside the row
    for name, n in (("-1", -1), ("INT32_MIN", INT32_MIN), ("stride+1", stride + 1), ("stride+4", stride + 4),
                    ("10^6", 10 ** 6)):
        add(f"length_{name}", E_INVALID, good, n)
    return cases


def row_of(pk, stride):
    """The packet's row: its bytes cut to the stride, zeros after them."""
    row = np.zeros(stride, np.uint8)
    row[:min(len(pk), stride)] = np.frombuffer(pk[:stride], np.uint8)
    return row


def classify(decode, ref, pk, length, W, B, stride):
    """The verdict the ABI owes a packet, from a CPU decoder (oracle.codec_decode's signature), as
    tests/test_gpu_codec.py's hostile test classifies: -> (verdict, inputs or None)."""
    if length < 0 or length > stride:
        return E_INVALID, None
    rc, inputs = decode(ref, row_of(pk, stride)[:length].tobytes())
    if rc < 0:
        return rc, None
    if any(len(x) != B for x in inputs):
        return UNSUPPORTED, None
    if len(inputs) > W:
        return E_CAP, None
    return OK, inputs


# ---- encode cases

def encode_cases(W, B):
    """[(name, ref [B] u8, pending [W][B] u8, count)]: the inputs whose XOR-delta stream (input k XOR
    input k-1, the first against ref) is the named byte pattern; random bytes in pending past count."""
    WB = W * B
    rng = np.random.default_rng(104729 * W + B)
    cases = []

    def stream(segments):
        out = bytearray()
        for cls, n in segments:
            out += rng.integers(1, 255, n, dtype=np.uint8).tobytes() if cls == "l" else (b"\xff" if cls == "f" else b"\x00") * n
        return bytes(out)

    def add(name, x):
        assert len(x) % B == 0 and len(x) <= WB, name
        i, count = len(cases), len(x) // B
        ref = (np.zeros(B, np.uint8), np.full(B, 255, np.uint8), rng.integers(0, 256, B, dtype=np.uint8))[i % 3]
        pend = rng.integers(0, 256, (W, B), dtype=np.uint8)
        prev = ref
        for k in range(count):
            pend[k] = prev ^ np.frombuffer(x[k * B:(k + 1) * B], np.uint8)
            prev = pend[k]
        cases.append((name, ref, pend, count))

    other = {"z": "lf", "f": "lz", "l": "zf"}
    for cls in "zfl":
        for count in sorted({0, 1, W - 1, W}):
            add(f"all_{cls}_{count}", stream([(cls, count * B)]))
    for a in "zfl":
        for b in other[a]:
            for s in range(1, WB):
                add(f"boundary_{a}{b}_{s}", stream([(a, s), (b, WB - s)]))
    for n in (31, 32, 33, 63, 64):
        for cls in "zfl":
            for o in other[cls]:
                if n == WB:
                    continue  # (all_*_W)
                if n < WB:
                    add(f"run_{cls}{n}_start_{o}", stream([(cls, n), (o, WB - n)]))
                    add(f"run_{cls}{n}_end_{o}", stream([(o, WB - n), (cls, n)]))
                if n + 2 <= WB:
                    a = (WB - n) // 2
                    add(f"run_{cls}{n}_middle_{o}", stream([(o, a), (cls, n), (o, WB - n - a)]))
    for a, b in ("lz", "lf", "zf"):
        for first in (a, b):
            second = b if first == a else a
            add(f"alternating_{first}{second}", stream([((first, second)[i % 2], 1) for i in range(WB)]))
    return cases


# ---- the same inputs in other bytes

ACCEPTING = ("split_runs", "zero_runs", "padded_varints", "some_sizes", "trailing_junk")
REJECTING = ("some_uneven", "some_negative")
RECODE_STATUS = {"some_uneven": UNSUPPORTED, "some_negative": E_DELTA}


def parse_runs(stream):
    """A valid run stream -> [(class, payload)]: ('z' | 'f', n) or ('l', bytes)."""
    out, q = [], 0
    while q < len(stream):
        h, shift = 0, 0
        while True:
            b = stream[q]
            q += 1
            h |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        if h & 1:
            out.append(("f" if h & 2 else "z", h >> 2))
        else:
            out.append(("l", bytes(stream[q:q + (h >> 1)])))
            q += h >> 1
    return out


def _emit(runs, pad=lambda: 0):
    return b"".join(lit(v, pad()) if cls == "l" else fill(v, cls == "f", pad()) for cls, v in runs)


def recode(data, kind, rng, input_bytes=None):
    """data: a valid tag-0 packet (bincode framing exact).  -> other bytes: for the ACCEPTING kinds a
    packet that decodes to the same inputs, for the REJECTING ones a tag-1 packet over the same stream
    whose sizes the feeds refuse.  The tag-1 kinds need input_bytes (B) to count the inputs."""
    assert data[0] == 0 and struct.unpack_from("<Q", data, 1)[0] == len(data) - 9, "a valid tag-0 packet"
    stream = data[9:]
    runs = parse_runs(stream)
    total = sum(v if cls != "l" else len(v) for cls, v in runs)
    if kind == "split_runs":
        out = []
        for cls, v in runs:
            n = v if cls != "l" else len(v)
            s = int(rng.integers(1, n)) if n > 1 else n
            out += [(cls, v[:s]), (cls, v[s:])] if cls == "l" else [(cls, s), (cls, n - s)]
        return packet(_emit([r for r in out if (r[1] if r[0] != "l" else len(r[1]))] or out[:1]))
    if kind == "zero_runs":
        out = []
        for r in runs:
            out += [(("z", 0), ("f", 0), ("l", b""))[int(rng.integers(0, 3))], r]
        return packet(_emit(out + [("l", b"")]))
    if kind == "padded_varints":
        return packet(_emit(runs, lambda: int(rng.integers(1, 4))) if runs else b"")
    if kind == "trailing_junk":
        return data + rng.integers(0, 256, int(rng.integers(1, 8)), dtype=np.uint8).tobytes()
    assert input_bytes and total % input_bytes == 0
    n = total // input_bytes
    if kind == "some_sizes":
        return packet(stream, sizes=[0] * n)
    if kind == "some_uneven":  # the first input one byte longer: the same run with one more byte
        return packet(stream + fill(1), sizes=[1, -1] + [0] * (n - 2) if n > 1 else [1] * n) if n else None
    if kind == "some_negative":
        return packet(stream, sizes=[-input_bytes - 1] + [0] * (n - 1)) if n else None
    raise ValueError(kind)
