"""GPU parity of the wire envelope (ggrs_wire_unpack / ggrs_wire_pack, csrc/wire.hip; ggrs_amd/wire.py)
against tests/wire_model.py: every datagram and every output array byte for byte, hostile datagrams
beside valid neighbours with guarded outputs, pack -> unpack on the device, the shapes at which the
kernels take another path, misuse -- and two engines playing each other datagram to datagram through
the lossy link of tests/test_gpu_p2p_emit.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import wire_model as W  # noqa: E402

pytestmark = pytest.mark.gpu

S, N, M = 130, 3, 4  # two full waves and a block of two; three calls; pack's four slots
NOW0 = 1 << 41
PACK_GROUPS = (  # the inputs that fill slot 0, 1, 2, 3
    ("start_frame", "packet_len", "ack_frame", "packets", "disc_mask", "last_frame", "disconnect_requested", "send_ack",
     "keep_alive"),
    ("send_report", "local_advantage"),
    ("kinds", "ping"),
    ("report_frame", "report_checksum"),
)


def dev(a):
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def now_table(n):
    return (NOW0 + 16 * np.arange(n)).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def pack_inputs(n, S_, ns, pstride, seed=0):
    """Random arrays of every input of ggrs_wire_pack: body lengths 1 .. packet_stride in turn (so the
    body ends on each of the four byte positions of a dword), some sessions without a packet."""
    rng = np.random.default_rng(100 + seed + ns)
    k = np.arange(n * S_).reshape(n, S_)
    a = dict(
        start_frame=rng.integers(0, 1 << 20, (n, S_)).astype(np.int32),
        packet_len=(1 + k % pstride).astype(np.int32),
        ack_frame=rng.integers(-1, 1 << 20, (n, S_)).astype(np.int32),
        packets=rng.integers(0, 256, (n, S_, pstride)).astype(np.uint8),
        disc_mask=rng.integers(0, 1 << ns, (n, S_)).astype(np.uint8),
        last_frame=rng.integers(-1, 1 << 20, (n, ns, S_)).astype(np.int32),
        disconnect_requested=(rng.random((n, S_)) < 0.2).astype(np.uint8),
        send_ack=(rng.random((n, S_)) < 0.6).astype(np.uint8),
        keep_alive=(rng.random((n, S_)) < 0.6).astype(np.uint8),
        send_report=(rng.random((n, S_)) < 0.5).astype(np.uint8),
        local_advantage=rng.integers(-40000, 40000, (n, S_)).astype(np.int32),
        kinds=rng.integers(0, 64, (n, S_)).astype(np.uint8),
        ping=np.zeros((n, S_, 16), np.uint8),
        report_frame=rng.integers(-3, 1 << 20, (n, S_)).astype(np.int32),
        report_checksum=rng.integers(0, 1 << 16, (n, S_)).astype(np.uint16),
    )
    a["start_frame"][rng.random((n, S_)) < 0.25] = -1
    a["packet_len"][rng.random((n, S_)) < 0.1] = 0
    a["report_frame"][rng.random((n, S_)) < 0.5] = -1
    # pings a reply may carry back: at most 2^20 ms before the call's clock, so that unpack accepts the pong
    ping = now_table(n)[:, None] - rng.integers(0, 1 << 20, (n, S_)).astype(np.uint64)
    a["ping"][:, :, :8] = ping[:, :, None].view(np.uint8).reshape(n, S_, 8)
    magic = rng.integers(0, 1 << 16, S_).astype(np.uint16)
    return magic, a


def run_pack(magic, now, ns, pstride, arrays, dstride=None):
    from ggrs_amd import wire
    dg, ln = wire.pack(dev(magic), dev(now), ns, pstride, dgram_stride=dstride, **{k: dev(v) for k, v in arrays.items()})
    torch.cuda.synchronize()
    return host(dg), host(ln)


def assert_packed(got, want):
    (dg, ln), (mdg, mln) = got, want
    assert dg.shape == mdg.shape
    assert (ln == mln).all(), np.argwhere(ln != mln)[:5]
    body = np.arange(dg.shape[-1]) < ln[..., None]
    bad = np.argwhere(np.where(body, dg, 0) != mdg)
    assert not len(bad), bad[:5]


def run_unpack(dgrams, lens, now, ns, rmask, first_call, pstride, **kw):
    from ggrs_amd import wire
    out = wire.unpack(dev(dgrams), dev(lens), dev(now), ns, rmask, pstride, first_call=first_call, **kw)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in out.items()}


def assert_unpacked(got, want):
    for k, m in want.items():
        if k not in got:
            continue
        g = got[k]
        if k == "packets":
            g = np.where(np.arange(g.shape[-1]) < want["packet_len"][..., None], g, 0)
        assert g.shape == m.shape and g.dtype == m.dtype, (k, g.shape, g.dtype, m.shape, m.dtype)
        bad = np.argwhere(g != m)
        assert not len(bad), (k, bad[:5], g[tuple(bad[0])], m[tuple(bad[0])])


def random_polls(n, M_, S_, ns, pstride, seed, empty=0.2):
    """Messages of all six tags in random slot order with empty slots; some Inputs carry more statuses."""
    rng = np.random.default_rng(seed)
    now = now_table(n)
    polls = [[[b""] * S_ for _ in range(M_)] for _ in range(n)]
    for i in range(n):
        for s in range(S_):
            for m in range(M_):
                if rng.random() >= empty:
                    msg = W.random_message(rng, int(rng.integers(6)), ns, pstride, int(now[i]),
                                           extra_statuses=int(rng.integers(0, 3)) * (rng.random() < 0.3))
                    polls[i][m][s] = W.serialize(msg)
    return polls, now


# ---- 1. pack parity

@pytest.mark.parametrize("ns", (2, 4))
def test_pack_matches_the_model_for_every_combination_of_absent_inputs(ns):
    pstride = 64
    magic, a = pack_inputs(N, S, ns, pstride)
    now = now_table(N)
    dstride = W.max_datagram_bytes(ns, pstride)
    assert sorted(set(a["packet_len"].ravel())) == list(range(pstride + 1))
    for combo in range(16):
        present = {k: v for g, names in enumerate(PACK_GROUPS) if combo >> g & 1 for k, v in a.items() if k in names}
        assert_packed(run_pack(magic, now, ns, pstride, present), W.pack_batch(magic, now, ns, pstride, dstride, **present))
    # single inputs absent inside slot 0's group: the envelope's defaults, the ack alone, the keep-alive alone
    for drop in (("ack_frame",), ("disc_mask", "last_frame", "disconnect_requested"), ("packets",), ("send_ack",),
                 ("start_frame", "packet_len", "packets", "send_ack", "send_report", "kinds", "report_frame")):
        present = {k: v for k, v in a.items() if k not in drop}
        assert_packed(run_pack(magic, now, ns, pstride, present), W.pack_batch(magic, now, ns, pstride, dstride, **present))
    # a wider row than the minimum
    assert_packed(run_pack(magic, now, ns, pstride, a, dstride + 20), W.pack_batch(magic, now, ns, pstride, dstride + 20, **a))


# ---- 2. unpack parity

@pytest.mark.parametrize("ns", (2, 4))
def test_unpack_matches_the_model_on_mixed_polls(ns):
    pstride = 64
    dstride = W.max_datagram_bytes(ns + 2, pstride)
    polls, now = random_polls(N, M, S, ns, pstride, seed=20 + ns)
    dgrams, lens = W.slots_to_arrays(polls, M, S, dstride)
    rmask = 0b1010 & ((1 << ns) - 1)
    want = W.unpack_batch(dgrams, lens, now, ns, rmask, 5, pstride)
    for t in range(6):
        assert (want["slot_status"] == t + 1).any()
    assert (want["notes"] != 0).any() and (want["events"] != 0).any()
    assert_unpacked(run_unpack(dgrams, lens, now, ns, rmask, 5, pstride), want)
    # a subset of the outputs: the others are not computed, these do not change
    few = run_unpack(dgrams, lens, now, ns, rmask, 5, pstride, want=("ack_in", "last_frame", "report_checksum"))
    assert sorted(few) == ["ack_in", "last_frame", "report_checksum"]
    assert_unpacked(few, want)


# ---- 3. hostile input

def guarded_outputs(n, M_, S_, ns, pstride, pattern=0xA5):
    """Every output of unpack carved out of one buffer with 256 guard bytes after each (and before the
    first): (the dict for wire.unpack's out, the buffer, a mask of its guard bytes)."""
    from ggrs_amd import wire
    specs = [(name, dtype, shape(n, M_, S_, ns, pstride)) for name, dtype, shape in wire.UNPACK_OUTPUTS]
    sizes = [int(np.prod(shape)) * np.dtype(dtype).itemsize for _, dtype, shape in specs]
    at, offs = 256, []
    for sz in sizes:
        offs.append(at)
        at += (sz + 255) // 256 * 256 + 256
    buf = torch.full((at,), pattern, dtype=torch.uint8, device="cuda")
    guard = np.ones(at, bool)
    out = {}
    for (name, dtype, shape), off, sz in zip(specs, offs, sizes):
        out[name] = buf[off:off + sz].view(getattr(torch, dtype)).view(shape)
        guard[off:off + sz] = False
    return out, buf, guard


def test_hostile_datagrams_leave_their_neighbours_and_the_guards_alone():
    """Every refusal of the CPU list sits in some slot of some session of calls 0 and 1, the other slots
    holding valid messages; call 2's slots hold random bytes at random stated lengths up to 4 past the
    row.  Outputs equal the model's; the guard bytes after packets and after every other output keep
    their pattern."""
    from ggrs_amd import wire
    ns, pstride = 2, 16
    cases = W.hostile_cases(ns, pstride, int(now_table(N)[0]))
    dstride = 64
    assert len(cases) <= 2 * S and max(len(d) for _, d, _ in cases) <= dstride
    polls, now = random_polls(N, M, S, ns, pstride, seed=31, empty=0.1)
    # (the hostile list is built for call 0's clock; call 1's is 16 ms later, which moves no verdict
    # but "pong now" and "pong from the future": those go to call 0)
    order = sorted(range(len(cases)), key=lambda k: not cases[k][0].startswith("pong"))
    placed = {}
    for j, k in enumerate(order):
        i, s, m = j // S, j % S, j % M
        polls[i][m][s] = cases[k][1]
        placed[(i, m, s)] = cases[k]
    rng = np.random.default_rng(32)
    for s in range(S):
        for m in range(M):
            stated = int(rng.integers(0, dstride + 5))
            polls[2][m][s] = (rng.integers(0, 256, dstride, dtype=np.uint8).tobytes(), stated)
    polls[2][1][7] = (bytes(dstride), 1 << 30)
    polls[2][2][7] = (bytes(dstride), -5)
    dgrams, lens = W.slots_to_arrays(polls, M, S, dstride)
    want = W.unpack_batch(dgrams, lens, now, ns, 0b10, 0, pstride)
    for (i, m, s), (name, _, status) in placed.items():
        assert want["slot_status"][i, m, s] == status, name
    assert (want["slot_status"][2] == W.E_BINCODE).sum() > S
    out, buf, guard = guarded_outputs(N, M, S, ns, pstride)
    wire.unpack(dev(dgrams), dev(lens), dev(now), ns, 0b10, pstride, out=out)
    torch.cuda.synchronize()
    got = {k: host(v) for k, v in out.items()}
    assert_unpacked(got, want)
    assert (buf.cpu().numpy()[guard] == 0xA5).all()
    # rows past packet_len are not written at all (nothing is scattered inside packets either)
    untouched = np.arange(pstride) >= (want["packet_len"][..., None] + 3) // 4 * 4
    assert (got["packets"][untouched] == 0xA5).all()


# ---- 4. pack -> unpack on the device

def test_pack_then_unpack_on_the_device_returns_the_arrays_packed():
    from ggrs_amd import wire
    ns, pstride = 2, 64
    magic, a = pack_inputs(N, S, ns, pstride)
    now = dev(now_table(N))
    d = {k: dev(v) for k, v in a.items()}
    dg, ln = wire.pack(dev(magic), now, ns, pstride, **d)
    got = wire.unpack(dg, ln, now, ns, 0b10, pstride)  # (no host copy between)
    torch.cuda.synchronize()
    got = {k: host(v) for k, v in got.items()}
    st = got["slot_status"]
    has_input = (a["start_frame"] >= 0) & (a["packet_len"] > 0)
    ack_only = ~has_input & (a["send_ack"] != 0)
    report, reply, cksum = a["send_report"] != 0, (a["kinds"] >> 2 & 1) != 0, a["report_frame"] >= 0
    keep = ~has_input & ~ack_only & (a["keep_alive"] != 0) & ~report & ~reply & ~cksum
    assert (st[:, 0] == np.select([has_input, ack_only, keep], [1, 2, 6], 0)).all()
    assert (st[:, 1] == 3 * report).all() and (st[:, 2] == 4 * reply).all() and (st[:, 3] == 5 * cksum).all()
    for case in (has_input, ack_only, keep, report, reply, cksum):
        assert case.any() and not case.all()
    # slot 0
    assert (got["start_frame"] == np.where(has_input, a["start_frame"], -1)).all()
    assert (got["packet_len"] == np.where(has_input, a["packet_len"], 0)).all()
    body = np.arange(pstride) < got["packet_len"][..., None]
    assert (np.where(body, got["packets"], 0) == np.where(body, a["packets"], 0)).all()
    assert (got["ack_in"] == np.where(has_input | ack_only, a["ack_frame"], -1)).all()
    dreq = has_input & (a["disconnect_requested"] != 0)
    merged = has_input & ~dreq
    assert (got["events"] == np.where(dreq, 0b10, 0)).all()
    assert (got["disc_mask"] == np.where(merged, a["disc_mask"], 0)).all()
    assert (got["last_frame"] == np.where(merged[:, None, :], a["last_frame"], -1)).all()
    # slots 1-3
    assert (got["remote_advantage"] == np.where(report, np.clip(a["local_advantage"], -32768, 32767), W.TIME_SYNC_KEEP)).all()
    sent_ping = np.zeros((N, S, 16), np.uint8)
    sent_ping[:, :, :8] = np.broadcast_to(now_table(N)[:, None], (N, S)).copy()[..., None].view(np.uint8).reshape(N, S, 8)
    assert (got["ping"] == np.where(report[..., None], sent_ping, 0)).all()  # a report's ping is the call's clock
    pong = a["ping"][:, :, :8].copy().view(np.uint64)[..., 0]
    assert (got["rtt_ms"] == np.where(reply, (now_table(N)[:, None] - pong).astype(np.int64), -1)).all()
    assert (got["report_frame"] == np.where(cksum, a["report_frame"], -1)).all()
    assert (got["report_checksum"] == np.where(cksum, a["report_checksum"], 0)).all()
    assert (got["kinds"] == (has_input * 1 | ack_only * 2 | report * 4 | reply * 8 | cksum * 16 | keep * 32)).all()


# ---- 5. the shapes at which the kernels take another path

@pytest.mark.parametrize("n,M_,S_,ns,pstride", [
    (3, 1, 130, 2, 64),     # one slot per poll
    (3, 8, 130, 2, 64),     # eight
    (3, 4, 1, 3, 64),       # one session: a block with one live lane
    (3, 4, 64, 1, 64),      # exactly one full block
    (1, 4, 130, 2, 64),     # one call
    (2, 4, 37, 4, 1012),    # the longest packet row: fewer sessions per block, so several blocks, the last partial
    (2, 4, 70, 2, 252),     # a stride between: 32 sessions per block
])
def test_shapes(n, M_, S_, ns, pstride):
    dstride = W.max_datagram_bytes(ns, pstride)
    polls, now = random_polls(n, M_, S_, ns, pstride, seed=50 + M_ + S_)
    rng = np.random.default_rng(51)
    for i in range(n):  # the longest body there is, and the lengths around a dword's end beside it
        for s in range(min(S_, 8)):
            body = rng.integers(0, 256, pstride - (s % 5), dtype=np.uint8).tobytes()
            polls[i][M_ - 1][s] = W.serialize(W.Message(s, W.Input([(False, 3)] * ns, False, 1 << 21, 9, body)))
    dgrams, lens = W.slots_to_arrays(polls, M_, S_, dstride)
    want = W.unpack_batch(dgrams, lens, now, ns, 1, 2, pstride)
    assert want["packet_len"].max() == pstride
    assert_unpacked(run_unpack(dgrams, lens, now, ns, 1, 2, pstride), want)
    magic, a = pack_inputs(n, S_, ns, pstride, seed=S_)
    assert_packed(run_pack(magic, now, ns, pstride, a), W.pack_batch(magic, now, ns, pstride, dstride, **a))


# ---- 6. misuse

def test_misuse_returns_invalid():
    from ggrs_amd import InvalidRequest, wire
    ns, pstride = 2, 64
    dstride = wire.max_datagram_bytes(ns, pstride)
    assert dstride == W.max_datagram_bytes(ns, pstride) == 112
    assert wire.max_datagram_bytes(4, 1012) == 1072 and wire.max_datagram_bytes(1, 12) == 48
    now = dev(now_table(N))

    def unpack(M_=M, ns_=ns, dstride_=dstride, pstride_=pstride, **kw):
        dg = torch.zeros((N, M_, S, dstride_), dtype=torch.uint8, device="cuda")
        ln = torch.zeros((N, M_, S), dtype=torch.int32, device="cuda")
        return wire.unpack(dg, ln, now, ns_, 0b10, pstride_, **kw)

    unpack()
    for bad in (dict(dstride_=110), dict(pstride_=62), dict(M_=0), dict(M_=9), dict(ns_=0), dict(ns_=5), dict(dstride_=4),
                dict(dstride_=2052), dict(pstride_=1016), dict(first_call=-1)):
        with pytest.raises(InvalidRequest):
            unpack(**bad)
    magic, a = pack_inputs(N, S, ns, pstride)
    d = {k: dev(v) for k, v in a.items()}
    wire.pack(dev(magic), now, ns, pstride, **d)
    for bad in (dict(dgram_stride=dstride - 4), dict(dgram_stride=dstride + 2), dict(dgram_stride=2052)):
        with pytest.raises(InvalidRequest):
            wire.pack(dev(magic), now, ns, pstride, **bad, **d)
    for bad_ns in (0, 5):
        with pytest.raises(InvalidRequest):
            wire.pack(dev(magic), now, bad_ns, pstride, dgram_stride=dstride)
    with pytest.raises(InvalidRequest):
        wire.pack(dev(magic), now, ns, 62, dgram_stride=dstride)
    with pytest.raises(InvalidRequest):  # a tensor of another shape never reaches the library
        wire.pack(dev(magic), now, ns, pstride, send_ack=d["send_ack"][:1])
    with pytest.raises(InvalidRequest):
        wire.pack(dev(magic), now, ns, pstride, no_such_input=d["send_ack"])
    torch.cuda.synchronize()


# ---- 7. two engines, datagram to datagram

class Datagrams:
    """One engine's packed datagrams, call by call, in device memory."""

    def __init__(self, calls, S_, dstride, dev_):
        self.dgrams = torch.zeros((calls, 4, S_, dstride), dtype=torch.uint8, device=dev_)
        self.len = torch.zeros((calls, 4, S_), dtype=torch.int32, device=dev_)

    def row(self, c):
        return self.dgrams[c:c + 1], self.len[c:c + 1]


def poll_slots(c, ok, D):
    """What the poll of call c receives of the other engine's datagrams (Datagrams D): ok [calls][4][S]
    says whether the datagrams of call c - k (k = 1..4) arrive now; whole slots move, by index
    arithmetic on the device.  Eight slots, oldest first: slot 0 (Input or InputAck) of calls c - 4 ..
    c - 1, then of each its QualityReport or QualityReply (a call never sends both here: reports leave
    at every 12th call and arrive 1-4 calls later)."""
    S_, dstride = D.dgrams.shape[2], D.dgrams.shape[3]
    dg = torch.zeros((1, 8, S_, dstride), dtype=torch.uint8, device=D.dgrams.device)
    ln = torch.zeros((1, 8, S_), dtype=torch.int32, device=D.dgrams.device)
    for k in (4, 3, 2, 1):
        if c - k < 0:
            continue
        here = ok[c, k - 1]
        dg[0, 4 - k] = D.dgrams[c - k, 0]
        ln[0, 4 - k] = torch.where(here, D.len[c - k, 0], 0)
        report = D.len[c - k, 1] > 0
        dg[0, 8 - k] = torch.where(report[:, None], D.dgrams[c - k, 1], D.dgrams[c - k, 2])
        ln[0, 8 - k] = torch.where(here, torch.where(report, D.len[c - k, 1], D.len[c - k, 2]), 0)
    return dg, ln


def test_two_engines_play_each_other_datagram_to_datagram(oracle):
    """The closed loop of tests/test_gpu_p2p_emit.py's packet-to-packet test (the same pair case, 130
    sessions, the same link tables) with the envelope in between: each engine's emit output and its
    time sync's local_advantage go through pack, the link moves whole datagram slots, and the
    receiver's unpack produces what receive_packets, emit_packets(ack_in) and time_sync take; a
    QualityReport leaves at every 12th call.  No session has an error; every call's start_frame,
    packet_len, packet bytes and ack_frame equal the modelled peers' -- the loop run without the
    envelope; each side's remote_advantage row is its peer's clamped local_advantage at the calls a
    report survived the link and GGRS_TIME_SYNC_KEEP elsewhere, and a reply that survived both ways
    measures the clock difference between the report's call and the reply's arrival."""
    from ggrs_amd import wire
    from tests.test_gpu_p2p_emit import History, engine
    from tests.test_packet_emit_model import PAIR_CALLS, PAIR_S, pair_case
    rows_a, rows_b, delay, drop, resend, peers = pair_case()
    calls, S_, mp, cap = PAIR_CALLS, PAIR_S, 8, 128
    dv = torch.device("cuda")
    A = engine(2, (0,), 0, mp, cap=cap, feed=True)
    B = engine(2, (1,), 0, mp, cap=cap, feed=True)
    A.set_time_sync(60)
    B.set_time_sync(60)
    stride = A.out_stride
    assert stride == B.out_stride == A.packet_stride == B.packet_stride
    dstride = wire.max_datagram_bytes(2, stride)
    HA, HB = History(calls, S_, stride, dv), History(calls, S_, stride, dv)
    DA, DB = Datagrams(calls, S_, dstride, dv), Datagrams(calls, S_, dstride, dv)
    i32 = lambda fill: torch.full((calls, S_), fill, dtype=torch.int32, device=dv)  # noqa: E731
    adv = {0: i32(0), 1: i32(0)}       # each side's local_advantage per call
    radv = {0: i32(0), 1: i32(0)}      # the remote_advantage each side's unpack produced
    rtt = {0: i32(0), 1: i32(0)}
    scratch = [torch.zeros((1, S_), dtype=torch.int32, device=dv) for _ in range(2)]
    ok = np.zeros((2, calls, 4, S_), bool)
    for k in range(1, 5):
        ok[:, k:, k - 1] = (delay[:, :calls - k] == k) & ~drop[:, :calls - k]
    ok_d = torch.from_numpy(ok).to(dv)
    resend_d = torch.from_numpy(resend).to(dv)
    now = dev(now_table(calls))
    magic = {0: dev(np.arange(S_).astype(np.uint16) + 0x4100), 1: dev(np.arange(S_).astype(np.uint16) + 0x4200)}
    ones = torch.ones((1, S_), dtype=torch.uint8, device=dv)
    sides = ((0, A, rows_a, HA, DA, DB, ok_d[1], 0b10), (1, B, rows_b, HB, DB, DA, ok_d[0], 0b01))
    for c in range(calls):
        polled = []
        for side, eng, rows, H, D, Dpeer, okd, rmask in sides:
            dg, ln = poll_slots(c, okd, Dpeer)
            polled.append(wire.unpack(dg, ln, now[c:c + 1], 2, rmask, stride, first_call=c))
        torch.cuda.synchronize()
        for (side, eng, rows, H, D, Dpeer, okd, rmask), u in zip(sides, polled):
            eng.add_inputs(c, rows[c:c + 1])
            eng.receive_packets(c, u["start_frame"], u["packet_len"], u["packets"], u["events"])
            eng.advance_frames(1)
            eng.emit_packets(c, 1, u["ack_in"], resend_d[c:c + 1], out=H.row(c))
            eng.time_sync(c, 1, u["rtt_ms"], u["remote_advantage"], out=(adv[side][c:c + 1], *scratch))
            radv[side][c] = u["remote_advantage"][0]
            rtt[side][c] = u["rtt_ms"][0]
        A.synchronize()
        B.synchronize()
        for (side, eng, rows, H, D, Dpeer, okd, rmask), u in zip(sides, polled):
            start, length, ack, packets = H.row(c)
            wire.pack(magic[side], now[c:c + 1], 2, stride, out=D.row(c), start_frame=start, packet_len=length,
                      ack_frame=ack, packets=packets, send_ack=ones, send_report=ones * (c % 12 == 0),
                      local_advantage=adv[side][c:c + 1], kinds=u["kinds"], ping=u["ping"])
    torch.cuda.synchronize()
    clock = now_table(calls).astype(np.int64)
    for side, eng, rows, H, D, Dpeer, okd, rmask in sides:
        frames, skipped, errors = eng.sessions()
        assert (errors == 0).all()
        assert (skipped[::5] > 0).all()  # the blackout sessions hit the prediction threshold
        start, length, ack = H.start.cpu().numpy(), H.length.cpu().numpy(), H.ack.cpu().numpy()
        packets = H.packets.cpu().numpy()
        for s in range(S_):
            X = peers[s][side]
            assert (start[:, s] == X.start).all() and (ack[:, s] == X.ack).all(), s
            for c in range(calls):
                assert length[c, s] == len(X.data[c]) and packets[c, s, :length[c, s]].tobytes() == X.data[c], (s, c)
            assert skipped[s] == X.skipped and frames[s] == X.cur, s
        last_acked, pending, st, closed = eng.emit_state()
        assert (st == 0).all() and (pending <= 2).all()
        # the reports: the peer's direction is 1 - side (direction 0 is A -> B)
        peer_adv = np.clip(adv[1 - side].cpu().numpy(), -32768, 32767)
        want = np.full((calls, S_), W.TIME_SYNC_KEEP, np.int64)
        want_rtt = np.full((calls, S_), -1, np.int64)
        d_in, d_out = 1 - side, side
        for c2 in range(0, calls, 12):
            for s in range(S_):
                c = c2 + delay[d_in, c2, s]
                if not drop[d_in, c2, s] and c < calls:
                    want[c, s] = peer_adv[c2, s]
        for c2 in range(0, calls, 12):  # this side's own report, the peer's reply at its arrival, back here
            for s in range(S_):
                c1 = c2 + delay[d_out, c2, s]
                if drop[d_out, c2, s] or c1 >= calls:
                    continue
                c3 = c1 + delay[d_in, c1, s]
                if not drop[d_in, c1, s] and c3 < calls:
                    want_rtt[c3, s] = clock[c3] - clock[c2]
        assert (radv[side].cpu().numpy() == want).all()
        assert (want != W.TIME_SYNC_KEEP).sum() > 10 * S_
        assert (rtt[side].cpu().numpy() == want_rtt).all()
        assert (want_rtt >= 0).sum() > 5 * S_
        # the time sync took what the envelope carried
        ts = eng.time_sync_state()
        last = np.array([want[want[:, s] != W.TIME_SYNC_KEEP, s][-1] for s in range(S_)])
        assert (ts[1] == last).all()
