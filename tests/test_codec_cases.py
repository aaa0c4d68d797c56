"""The directed codec cases (tests/codec_cases.py) on the CPU: what the device tests compare the
kernels with must itself be what it claims.  Every decode case reaches the verdict it was built for,
both CPU restatements (oracle/codec.c, oracle/pycodec.py) agree on it, every verdict class is reached
at every shape, the encode cases round-trip and stay inside ggrs_codec_max_packet_bytes, and recode's
kinds decode as they say.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import pycodec as PC
from tests import codec_cases as C
from tests import packet_feed_model as PF


@functools.lru_cache(maxsize=None)
def decode_cases(W, B, stride=None):
    return C.decode_cases(W, B, stride)


@functools.lru_cache(maxsize=None)
def encode_packets(W, B):
    """[(name, ref, inputs, packet)]: oracle.codec_encode of every encode case."""
    from oracle import oracle as O
    out = []
    for name, ref, pend, count in C.encode_cases(W, B):
        inputs = [pend[k].tobytes() for k in range(count)]
        out.append((name, ref.tobytes(), inputs, O.codec_encode(ref.tobytes(), inputs)))
    return out


def full_stride(W, B):
    """A row that holds every case that is meant to be parsed."""
    return max(len(pk) for name, _, _, pk, _ in decode_cases(W, B))


def strides(W, B):
    """The device test's strides: the ABI's default, the wide one, and the full one where the wide
    one had to be clipped to the run-level decoder's LDS."""
    full = (full_stride(W, B) + 3) // 4 * 4
    return sorted({C.max_packet_bytes(B, W), C.wide_stride(W, B, full), full})


def pycodec_verdict(ref, data, W, B):
    """oracle/pycodec.py's answer in the ABI's classes.  A tag-0 stream of more than 2^20 bytes is
    sized from its run lengths (pycodec.rle_decode), not cut into a million Python objects."""
    try:
        if data[:1] == b"\x00" and len(data) >= 9:
            m = int.from_bytes(data[1:9], "little")
            if m <= len(data) - 9:
                n = len(PC.rle_decode(data[9:9 + m]))
                if n > 1 << 20:
                    return C.E_DELTA if n % B else C.E_CAP  # (n // B > W)
        inputs = PC.decode(ref, data)
    except PC.CodecError as e:
        return {"bincode": C.E_BINCODE, "rle": C.E_RLE, "delta": C.E_DELTA}[str(e).split(":")[0]]
    if any(len(x) != B for x in inputs):
        return C.UNSUPPORTED
    return C.E_CAP if len(inputs) > W else C.OK


def test_dispatch_table():
    """The kernel each shape reaches, from the launch arithmetic of csrc/codec.hip as restated in
    codec_cases: the comment on SHAPES, and what the device test's parametrisation relies on."""
    want = {(1, 4): "run-level", (8, 1): "run-level", (12, 1): "run-level", (3, 4): "run-level", (5, 4): "run-level",
            (16, 2): "run-level", (32, 2): "run-level", (16, 4): "run-level", (64, 1): "run-level",
            (4, 3): "staged", (8, 8): "staged", (20, 4): "staged", (21, 4): "staged",
            (22, 4): "direct", (1, 7): "direct", (33, 4): "direct"}
    assert set(want) == set(C.SHAPES)
    for (W, B), form in want.items():
        assert C.decode_form(W, B) == form, (W, B)
        # "staged" asked for: the staged kernel where it fits, else the direct one, silently
        assert C.decode_form(W, B, form="staged") == ("direct" if form == "direct" else "staged"), (W, B)
        assert C.decode_form(W, B, form="direct") == "direct"
    # the 64-bit-mask ENCODE (NDW 16) is over the LDS budget at every stride: its rows alone are
    # 256 * (204 + 68) bytes.  W*B = 64 encodes through the staged kernel under the default form.
    assert C.encode_swar_lds(16, 12) > C.LDS_BUDGET
    for W, B in C.SHAPES:
        enc = C.encode_form(W, B)
        assert enc == ("staged" if W * B == 64 and B != 8 else want[(W, B)]), (W, B)
    # 32-bit masks up to NDW 8; K > W*B at (12,1), (3,4) and (5,4)
    assert [C.swar_ndw(B, W, 16) for W, B in C.SHAPES[:9]] == [1, 2, 4, 4, 8, 8, 16, 16, 16]
    assert [(W, B) for W, B in C.SHAPES if C.scratch_bytes(W, B) > W * B] == [(12, 1), (3, 4), (5, 4)]
    # the edge of the LDS budget: one row of 4 bytes decides
    assert C.staged_lds(4, 21, C.max_packet_bytes(4, 21)) == 64512 <= C.LDS_BUDGET < C.staged_lds(4, 22, C.max_packet_bytes(4, 22))
    # the wide stride keeps the run-level decoder where the default stride has it
    for W, B in C.SHAPES:
        for s in strides(W, B)[:2]:
            assert s % 4 == 0
            if want[(W, B)] == "run-level":
                assert C.decode_form(W, B, s) == "run-level", (W, B, s)


@pytest.mark.parametrize("W,B", C.SHAPES)
def test_every_decode_case_reaches_its_intent(oracle, W, B):
    cases = decode_cases(W, B)
    assert len({name for name, *_ in cases}) == len(cases)
    full = strides(W, B)[-1]
    for stride in strides(W, B):
        for (name, intent, ref, pk, length), (_, _, _, _, length0) in zip(decode_cases(W, B, stride), cases):
            got, inputs = C.classify(PF.codec_decode, ref, pk, length, W, B, stride)
            outside = length < 0 or length > stride
            assert got == (C.E_INVALID if outside else intent), (name, stride, got, intent)
            if stride == full:  # only the cases built to lie outside the row do
                assert outside == (intent == C.E_INVALID), name
            assert (length == length0) or intent == C.E_INVALID, name
            if got == C.OK:
                assert len(inputs) <= W and all(len(x) == B for x in inputs)


@pytest.mark.parametrize("W,B", C.SHAPES)
def test_pycodec_agrees_on_every_decode_case(oracle, W, B):
    stride = strides(W, B)[-1]
    for name, intent, ref, pk, length in decode_cases(W, B):
        if intent == C.E_INVALID:
            continue  # a length outside the row, the ABI's own verdict: no bytes to decode
        assert 0 <= length <= stride
        data = C.row_of(pk, stride)[:length].tobytes()
        rc, inputs = PF.codec_decode(ref, data)
        assert pycodec_verdict(ref, data, W, B) == intent, name
        if rc == 0:
            assert PC.decode(ref, data) == inputs, name


@pytest.mark.parametrize("W,B", C.SHAPES)
def test_census(oracle, W, B):
    """A condition on the cases, not a measurement: the oracle reaches every verdict class at least
    three times and accepts at least one tag-1 packet, with no case left out."""
    stride = strides(W, B)[-1]
    cases = decode_cases(W, B, stride)
    seen = {v: 0 for v in C.VERDICTS}
    tag1 = 0
    for name, intent, ref, pk, length in cases:
        got, _ = C.classify(PF.codec_decode, ref, pk, length, W, B, stride)
        seen[got] += 1
        tag1 += got == C.OK and pk[0] == 1
    assert all(n >= 3 for n in seen.values()), seen
    assert tag1 >= 1
    assert len(cases) <= 600  # (the device batches repeat them)


@pytest.mark.parametrize("W,B", C.SHAPES)
def test_encode_cases_round_trip_within_the_bound(oracle, W, B):
    packets = encode_packets(W, B)
    bound = C.max_packet_bytes(B, W)
    assert bound == PF.max_packet_bytes(B, W)
    longest = 0
    for name, ref, inputs, pk in packets:
        assert PF.codec_decode(ref, pk) == (0, inputs), name
        assert pk == PC.encode(ref, inputs), name
        longest = max(longest, len(pk))
    assert longest <= bound
    # the alternating one-byte runs are the longest packets the format has: 3 bytes per 2 of input
    assert longest == 9 + W * B + (W * B + 1) // 2
    by_name = {name: pk for name, _, _, pk in packets}
    assert len(by_name) == len(packets)
    runs = [C.parse_runs(by_name[f"all_{cls}_{W}"][9:]) for cls in "zfl"]
    assert [(r[0][0], len(r)) for r in runs] == [("z", 1), ("f", 1), ("l", 1)]  # one run each, W*B long
    if W * B >= 64:  # the two-byte literal header starts at 64
        assert len(C.varint(64 << 1)) == 2 and any(len(v) == 64 for pk in by_name.values()
                                                   for cls, v in C.parse_runs(pk[9:]) if cls == "l")


def test_assembler():
    assert C.varint(0) == b"\x00" and C.varint(300) == b"\xac\x02" and C.varint(5, 2) == b"\x85\x80\x00"
    assert C.fill(100) == bytes([0x91, 0x03]) and C.fill(1, True) == b"\x07" and C.lit(b"ab") == b"\x04ab"
    assert C.lit(b"a", claim=2) == b"\x04a" and len(C.fill(3, pad=9)) == 10
    assert C.packet([C.fill(2), C.lit(b"x")]) == b"\x00" + (3).to_bytes(8, "little") + b"\x09\x02x"
    assert C.packet(b"", sizes=[-1, 2]) == b"\x01" + (2).to_bytes(8, "little") + b"\xff\xff\xff\xff\x02\x00\x00\x00" + bytes(8)
    assert C.packet(b"\x05", m=7, tail=b"zz", tag=9)[:10] == b"\x09" + (7).to_bytes(8, "little") + b"\x05"
    assert PC.rle_decode(C.fill(3, True, 4) + C.lit(b"q", 2) + C.fill(0, pad=1)) == b"\xff\xff\xffq"


@pytest.mark.parametrize("B", [1, 2, 4])
def test_recode_kinds(oracle, B):
    from oracle import oracle as O
    rng = np.random.default_rng(B)
    differ = {k: 0 for k in C.ACCEPTING + C.REJECTING}
    for trial in range(60):
        ref = rng.integers(0, 256, B, dtype=np.uint8).tobytes()
        n = int(rng.integers(0 if trial % 10 == 0 else 1, 20))
        held = rng.choice(np.array([0, 0, 0, 0, 255, 255, 7, 93], np.uint8), (n, B))  # deltas with fills
        inputs = [held[k].tobytes() for k in range(n)]
        data = O.codec_encode(ref, inputs)
        for kind in C.ACCEPTING:
            out = C.recode(data, kind, rng, B)
            assert PF.codec_decode(ref, out) == (0, inputs) and PC.decode(ref, out) == inputs, kind
            differ[kind] += out != data
            if kind == "trailing_junk":
                assert out[:len(data)] == data and len(out) > len(data)
            if kind == "some_sizes":
                assert out[0] == 1
        for kind in C.REJECTING:
            out = C.recode(data, kind, rng, B)
            if n == 0:
                assert out is None
                continue
            got, _ = C.classify(PF.codec_decode, ref, out, len(out), 64, B, len(out))
            assert got == C.RECODE_STATUS[kind], kind
            differ[kind] += 1
    assert all(v >= 40 for v in differ.values()), differ  # (an empty or all-one-byte-run stream has no other form)
