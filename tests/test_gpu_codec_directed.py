"""GPU parity of the batched wire codec on directed packets (tests/codec_cases.py) against oracle/codec.c:
every run length, header width, size list and reject edge, at the shapes where the launch takes
another kernel, under every kernel form.  The rule is exact: status, count and the whole output row
equal the oracle's (UNSUPPORTED exactly when it decodes sizes other than B, E_CAP exactly when it
decodes more than W inputs); encoded bytes and lengths equal oracle.codec_encode's.

Which kernel a shape reaches (codec_cases.SHAPES, asserted from the launch arithmetic on the CPU in
tests/test_codec_cases.py::test_dispatch_table), decode at the default stride, form "default":
  (1,4) (8,1) (12,1) (3,4) (5,4) (16,2)   run-level, 32-bit masks; scratch K > W*B at (12,1) (3,4) (5,4)
  (32,2) (16,4) (64,1)                    run-level, 64-bit masks -- decode only: the 64-bit-mask encode
                                          is over the LDS budget at every stride, these encode staged
  (4,3) (8,8)                             staged (B outside {1,2,4}); (20,4) (21,4): staged, W*B > 64,
                                          (21,4) with 64512 of the 65536 bytes of LDS
  (22,4)                                  direct under every form (staged would need 66560 bytes)
  (1,7) (33,4)                            direct
Form "staged" gives the staged kernel wherever the default is run-level or staged; "direct" the direct
one everywhere.  The wide decode stride keeps that table except where noted at its use."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import codec_cases as C  # noqa: E402
from tests import packet_feed_model as PF  # noqa: E402

pytestmark = pytest.mark.gpu

MIN_PACKETS = 600


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cpu(*ts):
    return [t.cpu().numpy() for t in ts]


@pytest.fixture(params=["default", "staged", "direct"])
def kernels(request):
    """Every kernel form: default (thread-per-packet run-level where input_bytes is 1, 2 or 4 and
    W*B <= 64 whole dwords, else LDS-staged), LDS-staged, and direct."""
    from ggrs_amd import codec
    codec.set_kernels(request.param)
    yield request.param
    codec.set_kernels("default")


def order_of(n_cases, rejects, seed):
    """Case indices for a batch: whole permutations of the cases up to at least MIN_PACKETS and to a
    block boundary's neighbourhood, then one 256-packet block of rejected cases only, then a partial
    block: neighbouring lanes differ and the batch crosses more than two block boundaries."""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.permutation(n_cases) for _ in range(-(-MIN_PACKETS // n_cases))])
    pad = (-len(idx)) % 256
    idx = np.concatenate([idx, rng.integers(0, n_cases, pad)])
    block = rng.permutation(np.resize(np.asarray(rejects), 256))
    return np.concatenate([idx, block, rng.permutation(n_cases)[:37]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def full_stride(W, B):
    return (max(len(pk) for _, _, _, pk, _ in C.decode_cases(W, B)) + 3) // 4 * 4


def decode_strides(W, B):
    """The default stride; the wide one (every parsed case fits, or the widest row of the run-level
    decoder's LDS); and, where that clipped it -- (64,1), whose Some(..) cases are 280 bytes -- the
    full one, at which every form of that shape is the direct kernel."""
    full = full_stride(W, B)
    return sorted({C.max_packet_bytes(B, W), C.wide_stride(W, B, full), max(full, C.wide_stride(W, B, full))})


@functools.lru_cache(maxsize=None)
def decode_batch(W, B, stride):
    """The batch and the oracle's answers, once per (shape, stride) for every form."""
    from oracle import oracle as O
    O.build()
    cases = C.decode_cases(W, B, stride)
    verdicts, rows = [], np.zeros((len(cases), W * B), np.uint8)
    for i, (name, intent, ref, pk, length) in enumerate(cases):
        v, inputs = C.classify(PF.codec_decode, ref, pk, length, W, B, stride)
        verdicts.append((v, len(inputs) if v == C.OK else 0))
        if v == C.OK:
            flat = np.frombuffer(b"".join(inputs), np.uint8)
            rows[i, :len(flat)] = flat
    rejects = [i for i, (v, _) in enumerate(verdicts) if v != C.OK]
    idx = order_of(len(cases), rejects, 1000 * W + B)
    assert len(idx) >= MIN_PACKETS + 256 and all(verdicts[i][0] != C.OK for i in idx[-293:-37])
    return dict(names=[cases[i][0] for i in idx],
                ref=np.stack([np.frombuffer(cases[i][2], np.uint8) for i in idx]),
                packets=np.stack([C.row_of(cases[i][3], stride) for i in idx]),
                length=np.array([cases[i][4] for i in idx], np.int32),
                status=np.array([verdicts[i][0] for i in idx], np.int32),
                count=np.array([verdicts[i][1] for i in idx], np.int32),
                out=rows[idx].reshape(len(idx), W, B))


def assert_decoded(b, dec, cnt, st, what):
    dec, cnt, st = cpu(dec, cnt, st)
    bad = np.nonzero((st != b["status"]) | (cnt != b["count"]) | (dec != b["out"]).any(axis=(1, 2)))[0]
    assert len(bad) == 0, (what, [(int(p), b["names"][p], int(st[p]), int(b["status"][p]), int(cnt[p])) for p in bad[:6]])


@pytest.mark.parametrize("W,B", C.SHAPES)
def test_decode_matches_oracle(oracle, kernels, W, B):
    """status, count and the whole row, written into a 0xAB-dirty out: the inputs with zeros past
    count, all zeros for a rejected packet.  A case longer than the stride goes in with its true length
    and a cut row: E_INVALID."""
    from ggrs_amd import codec
    for stride in decode_strides(W, B):
        b = decode_batch(W, B, stride)
        N = len(b["length"])
        assert set(C.VERDICTS) <= set(b["status"].tolist())
        dirty = torch.full((N, W, B), 0xAB, dtype=torch.uint8, device="cuda")
        dec, cnt, st = codec.decode(gpu(b["ref"]), gpu(b["packets"]), gpu(b["length"]), max_inputs=W, out=dirty)
        assert dec.data_ptr() == dirty.data_ptr()
        assert_decoded(b, dec, cnt, st, (kernels, stride))


@pytest.mark.parametrize("W,B", [s for s in C.SHAPES if C.chunked_ok(*s, C.max_packet_bytes(s[1], s[0]))])
def test_chunked_decode_matches_oracle(oracle, W, B):
    """The same cases back to back at their chunk offsets (a length outside [1, stride] takes no
    bytes), against the oracle and not against the strided kernel."""
    from ggrs_amd import codec
    for stride in decode_strides(W, B):
        if not C.chunked_ok(W, B, stride):
            continue  # (64,1)'s full stride: over the run-level decoder's LDS, the ABI refuses it (below)
        b = decode_batch(W, B, stride)
        N = len(b["length"])
        off = codec.chunk_offsets(b["length"], stride)
        flat = np.full(N * stride, 0xEE, np.uint8)  # what lies between the blocks' packets is not read
        for p in range(N):
            n = int(b["length"][p])
            if 1 <= n <= stride:
                flat[off[p]:off[p] + n] = b["packets"][p, :n]
                flat[off[p] + n:off[p] + (n + 3) // 4 * 4] = 0
        dirty = torch.full((N, W, B), 0xAB, dtype=torch.uint8, device="cuda")
        dec, cnt, st = codec.decode(gpu(b["ref"]), gpu(flat.reshape(N, stride)), gpu(b["length"]), max_inputs=W,
                                    chunked=True, out=dirty)
        assert_decoded(b, dec, cnt, st, ("chunked", stride))


# ---- encode

@functools.lru_cache(maxsize=None)
def encode_batch(W, B):
    from oracle import oracle as O
    O.build()
    cases = C.encode_cases(W, B)
    want = [O.codec_encode(ref.tobytes(), [pend[k].tobytes() for k in range(count)]) for _, ref, pend, count in cases]
    rng = np.random.default_rng(W * 131 + B)
    idx = np.concatenate([rng.permutation(len(cases)) for _ in range(-(-(MIN_PACKETS + 1) // len(cases)))])
    wlen = np.array([len(want[i]) for i in idx], np.int32)
    wbytes = np.zeros((len(idx), int(wlen.max())), np.uint8)
    for p, i in enumerate(idx):
        wbytes[p, :wlen[p]] = np.frombuffer(want[i], np.uint8)
    return dict(names=[cases[i][0] for i in idx], ref=np.stack([cases[i][1] for i in idx]),
                pending=np.stack([cases[i][2] for i in idx]), count=np.array([cases[i][3] for i in idx], np.int32),
                wlen=wlen, wbytes=wbytes)


def encode_strides(W, B):
    d = C.max_packet_bytes(B, W)
    return sorted({d, d - 16, d - 5} | set(range(12, 49, 4)))


def assert_encoded(b, out, ln, stride, what, good=None):
    """Lengths (E_CAP exactly when the oracle's packet is longer than the stride) and every byte of
    every packet that fits."""
    from ggrs_amd import codec
    good = np.ones(len(ln), bool) if good is None else good
    fits = b["wlen"] <= stride
    want_len = np.where(fits, b["wlen"], codec.E_CAP)
    bad = np.nonzero((ln != want_len) & good)[0]
    assert len(bad) == 0, (what, "length", [(int(p), b["names"][p], int(ln[p]), int(want_len[p])) for p in bad[:6]])
    width = min(stride, b["wbytes"].shape[1])
    live = (np.arange(width)[None, :] < b["wlen"][:, None]) & (fits & good)[:, None]
    bad = np.nonzero(((out[:, :width] != b["wbytes"][:, :width]) & live).any(axis=1))[0]
    assert len(bad) == 0, (what, "bytes", [(int(p), b["names"][p]) for p in bad[:6]])


@pytest.mark.parametrize("W,B", C.SHAPES)
def test_encode_matches_oracle(oracle, kernels, W, B):
    """Every stride from far too short to the ABI's bound, whole dwords and not: at the default stride
    no case is E_CAP (ggrs_codec_max_packet_bytes holds for the longest packets the format has), and
    the ABI's value is the formula the CPU tests bound the cases with."""
    from ggrs_amd import codec
    b = encode_batch(W, B)
    default = codec.max_packet_bytes(B, W)
    assert default == C.max_packet_bytes(B, W) and b["wlen"].max() <= default
    assert len(b["count"]) > 2 * 256
    ref, pend, count = gpu(b["ref"]), gpu(b["pending"]), gpu(b["count"])
    for stride in encode_strides(W, B):
        out, ln = cpu(*codec.encode(ref, pend, count, stride=stride))
        assert_encoded(b, out, ln, stride, (kernels, stride))
        if stride == default:
            assert (ln > 0).all()
        if stride == 12:  # (a literal run of the whole stream alone is 10 + W*B bytes)
            assert (ln == codec.E_CAP).any() and (ln > 0).any()


def short_stride(W, B):
    """A stride that the fill-only packets fit and a literal run of the whole stream does not."""
    return max(12, (9 + W * B + 2) // 4 * 4)


@pytest.mark.parametrize("W,B", [s for s in C.SHAPES if C.chunked_ok(*s, short_stride(*s), encode=True)])
def test_chunked_encode_with_errors_in_every_block(oracle, W, B):
    """Counts outside 0..W and packets too long for the stride in every 256-packet block: the block
    scan sees zero-byte packets between the others.  Lengths and codes, every good packet's bytes at its
    chunk offset with zero padding, and the chunked decode of that buffer gives the inputs back."""
    from ggrs_amd import codec
    b = encode_batch(W, B)
    N, stride = len(b["count"]), short_stride(W, B)
    count = b["count"].copy()
    count[::7] = -1
    count[3::11] = W + 1
    good = (count >= 0) & (count <= W)
    out, ln = codec.encode(gpu(b["ref"]), gpu(b["pending"]), gpu(count), stride=stride, chunked=True)
    flat, lh = out.cpu().numpy().reshape(-1), ln.cpu().numpy()
    assert (lh[~good] == codec.E_INVALID).all()
    off = codec.chunk_offsets(lh, stride)
    rows = np.zeros((N, stride), np.uint8)
    for p in np.nonzero(lh > 0)[0]:
        n = int(lh[p])
        rows[p, :n] = flat[off[p]:off[p] + n]
        assert not flat[off[p] + n:off[p] + (n + 3) // 4 * 4].any(), (p, b["names"][p])
    assert_encoded(b, rows, lh, stride, ("chunked", stride), good)
    for blk in range(0, N, 256):
        codes = set(lh[blk:blk + 256][lh[blk:blk + 256] < 0].tolist())
        assert codes == {codec.E_INVALID, codec.E_CAP} and (lh[blk:blk + 256] > 0).any(), blk
    dec, cnt, st = cpu(*codec.decode(gpu(b["ref"]), out, ln, max_inputs=W, chunked=True))
    ok = lh > 0
    assert (st[ok] == 0).all() and (cnt[ok] == count[ok]).all() and (st[~ok] == codec.E_INVALID).all()
    live = (np.arange(W)[None, :] < np.where(ok, count, 0)[:, None])[:, :, None]
    assert (dec == np.where(live, b["pending"], 0)).all()


# ---- pointers off the dword

def shifted(t, k=1):
    """t's values in a contiguous view that starts k bytes into a larger tensor."""
    big = torch.empty(t.numel() * t.element_size() + k, dtype=torch.uint8, device=t.device)
    v = big[k:].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 4 == k % 4
    return v


def raw_encode(ref, pend, count, out, out_len, stride, chunked=False):
    from ggrs_amd import _lib, codec
    L = _lib.lib()
    codec._bind(L)
    N, W, B = pend.shape
    fn = L.ggrs_codec_encode_chunked if chunked else L.ggrs_codec_encode
    return fn(codec._p(ref), codec._p(pend), codec._p(count), N, B, W, codec._p(out), stride, codec._p(out_len),
              codec._stream(pend))


@pytest.mark.parametrize("W,B", [(16, 2), (64, 1), (3, 4), (8, 8), (21, 4), (1, 7)])
def test_unaligned_pointers_change_nothing(oracle, kernels, W, B):
    """ref at an odd address with everything else dword-aligned (the run-level forms read it through
    byte loads), then pending, packets and out one byte off the dword each on its own (the launch
    falls back to the direct kernel): the results of the aligned call, bit for bit."""
    from ggrs_amd import codec
    stride = C.max_packet_bytes(B, W)
    b = decode_batch(W, B, stride)
    N = len(b["length"])
    ref, pk, ln = gpu(b["ref"]), gpu(b["packets"]), gpu(b["length"])
    for what, args, out_k in (("ref", (shifted(ref), pk, ln), 0), ("ref+3", (shifted(ref, 3), pk, ln), 0),
                              ("packets", (ref, shifted(pk), ln), 0), ("out", (ref, pk, ln), 1)):
        dirty = shifted(torch.full((N, W, B), 0xAB, dtype=torch.uint8, device="cuda"), out_k) if out_k else None
        assert_decoded(b, *codec.decode(*args, max_inputs=W, out=dirty), (kernels, "decode", what))
    e = encode_batch(W, B)
    N = len(e["count"])
    ref, pend, count = gpu(e["ref"]), gpu(e["pending"]), gpu(e["count"])
    for what, r, p, out_k in (("ref", shifted(ref), pend, 0), ("pending", ref, shifted(pend), 0), ("out", ref, pend, 1)):
        out = torch.full((N, stride), 0xAB, dtype=torch.uint8, device="cuda")
        out = shifted(out, out_k) if out_k else out
        out_len = torch.empty(N, dtype=torch.int32, device="cuda")
        assert raw_encode(r, p, count, out, out_len, stride) == 0
        assert_encoded(e, *cpu(out, out_len), stride, (kernels, "encode", what))


# ---- what the ABI refuses

def test_abi_rejections(oracle):
    from ggrs_amd import InvalidRequest, _lib, codec
    L = _lib.lib()
    codec._bind(L)
    W, B, N = 8, 2, 4
    stride = C.max_packet_bytes(B, W)
    ref, pend = gpu(np.zeros((N, B), np.uint8)), gpu(np.zeros((N, W, B), np.uint8))
    count = gpu(np.full(N, W, np.int32))
    pk, ln = codec.encode(ref, pend, count)
    out = torch.empty((N, W, B), dtype=torch.uint8, device="cuda")
    cnt, st_ = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
    p, null, s = codec._p, ctypes.c_void_p(None), codec._stream(ref)

    def enc(fn, n=N, b=B, w=W, st=stride):
        return fn(p(ref), p(pend), p(count), n, b, w, p(pk), st, p(ln), s)

    def dec(fn, n=N, b=B, w=W, st=stride):
        return fn(p(ref), p(pk), p(ln), n, st, b, w, p(out), p(cnt), p(st_), s)

    for fn in (L.ggrs_codec_encode, L.ggrs_codec_encode_chunked):
        assert enc(fn) == 0
        for bad in (dict(st=8), dict(st=0), dict(n=-1), dict(b=0), dict(b=-1), dict(w=-1)):
            assert enc(fn, **bad) == _lib.GGRS_E_INVALID, (fn.__name__, bad)
        assert fn(null, null, null, 0, B, W, null, stride, null, s) == 0  # nothing to do, nothing read
        assert fn(null, p(pend), p(count), N, B, W, p(pk), stride, p(ln), s) == _lib.GGRS_E_INVALID
    for fn in (L.ggrs_codec_decode, L.ggrs_codec_decode_chunked):
        assert dec(fn) == 0
        for bad in (dict(n=-1), dict(b=0), dict(w=-1), dict(st=-4)):
            assert dec(fn, **bad) == _lib.GGRS_E_INVALID, (fn.__name__, bad)
        assert fn(null, null, null, 0, stride, B, W, null, null, null, s) == 0
        assert fn(p(ref), null, p(ln), N, stride, B, W, p(out), p(cnt), p(st_), s) == _lib.GGRS_E_INVALID
    torch.cuda.synchronize()
    # the chunked entry points on shapes they do not take: B outside {1, 2, 4}, rows not whole dwords,
    # W*B > 64, a stride off the dword, the 64-bit-mask encode (over its LDS), a decode row too wide
    # for the run-level kernel's LDS
    for w, b, st, both in ((4, 3, 48, True), (3, 2, 32, True), (33, 2, 128, True), (8, 2, 30, True),
                           (64, 1, 128, False), (16, 4, 128, False)):
        r, x = gpu(np.zeros((N, b), np.uint8)), gpu(np.zeros((N, w, b), np.uint8))
        with pytest.raises(InvalidRequest):
            codec.encode(r, x, gpu(np.zeros(N, np.int32)), stride=st, chunked=True)
        if both:
            with pytest.raises(InvalidRequest):
                codec.decode(r, gpu(np.zeros((N, st), np.uint8)), gpu(np.zeros(N, np.int32)), max_inputs=w, chunked=True)
    with pytest.raises(InvalidRequest):
        codec.decode(gpu(np.zeros((N, 1), np.uint8)), gpu(np.zeros((N, 284), np.uint8)), gpu(np.zeros(N, np.int32)),
                     max_inputs=64, chunked=True)
    # unaligned buffers: the strided entry points take them, the chunked ones refuse
    with pytest.raises(InvalidRequest):
        codec.decode(ref, shifted(pk), ln, max_inputs=W, chunked=True)
    assert raw_encode(ref, shifted(pend), count, pk, ln, stride, chunked=True) == _lib.GGRS_E_INVALID
    assert codec.encode(ref, pend, count)[1].min() > 0  # the library still works
