"""GPU parity of the P2P engine's packet emit (ggrs_p2p_set_packet_emit / emit_packets /
read_emit_state, csrc/p2p_emit.hip) against tests/packet_emit_model.py: every call's start_frame,
packet_len, ack_frame and packet bytes under arrival schedules, emit split over launches, overflow,
close, misuse -- and two engines playing each other packet to packet through a lossy link, the
packets staying in device memory."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import packet_emit_model as E  # noqa: E402
from tests import packet_feed_model as F  # noqa: E402
from tests.test_gpu_p2p_sched import check_sessions, schedules, set_form  # noqa: E402

pytestmark = pytest.mark.gpu

PIECES = (1, 3, 60, 17, 159)
S, CALLS, W = 130, 240, 64

CASES = [
    # form, P, local players, input delay, max_prediction
    ("flat", 2, (0,), 0, 8),
    ("flat", 2, (0,), 2, 8),
    ("flat", 4, (0, 2), 0, 7),
    ("flat", 4, (1, 2, 3), 1, 8),
    ("flat", 2, (1,), 0, 0),  # lockstep mode
    ("chains", 2, (0,), 0, 8),
    ("chains", 4, (0, 2), 0, 7),
]


def pushed_table(o, rows, arrive, events, P, mask, delay, mp):
    """(pushed [calls][S], stop_call [S]) from the oracle's P2PSession: the frame each call queued
    (packet_emit_model.pushes over its per-call `advanced`), the call at which it panics (-1)."""
    calls, S_ = arrive.shape
    pushed = np.full((calls, S_), -1, np.int32)
    stop = np.full(S_, -1, np.int32)
    for s in range(S_):
        out = o.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=mask,
                              input_delay=delay, max_prediction=mp)
        if out["rc"] != 0:
            stop[s] = out["result"].frames_done
        n = calls if stop[s] < 0 else stop[s]
        pushed[:n, s] = E.pushes(out["advanced"][:n], delay)
    return pushed, stop


def ack_tables(pushed, seed):
    """Random lagging acks (so some are stale), no ack at four calls in ten, a silence of 30 calls in
    every fourth session, an ack ahead of the newest pending frame in every seventh; sparse resend
    flags."""
    calls, S_ = pushed.shape
    rng = np.random.default_rng(seed)
    newest = np.maximum.accumulate(pushed, axis=0)
    lag = rng.integers(1, 7, (calls, S_))
    src = np.maximum(np.arange(calls)[:, None] - lag, 0)
    ack = newest[src, np.arange(S_)[None, :]].astype(np.int32)
    ack[np.arange(calls)[:, None] < lag] = -1
    ack[rng.random((calls, S_)) < 0.4] = -1
    ack[90:120, 1::4] = -1
    ack[150, 3::7] = newest[150, 3::7] + 5
    resend = (rng.random((calls, S_)) < 0.1).astype(np.uint8)
    return ack, resend


@functools.lru_cache(maxsize=None)
def parity_case(P, local, delay, mp):
    from oracle import oracle as o
    mask = sum(1 << k for k in local)
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0xE317), CALLS, P, 0) for s in range(S)], axis=1)
    arrive, events = schedules(S, CALLS, max(mp, 8), 19 + P + delay, mask, P)
    pushed, stop = pushed_table(o, rows, arrive, events, P, mask, delay, mp)
    ack, resend = ack_tables(pushed, 7 + P)
    stride = F.max_packet_bytes(len(local), W)
    m = E.run(rows, pushed, mask, W, stride, ack, resend, events, recv=np.maximum.accumulate(arrive, axis=0),
              stop_call=stop)
    return rows, arrive, events, ack, resend, m


def engine(P, local, delay, mp, cap=CALLS, max_pending=W, feed=False, S_=S):
    from ggrs_amd import P2PEngine
    e = P2PEngine(S_, num_players=P, local_players=local, input_delay=delay, max_prediction=mp, remote_latency=1,
                  input_capacity=cap)
    e.set_arrival_schedule(True)
    if feed:
        e.set_packet_feed(W)
    e.set_packet_emit(max_pending)
    return e


def assert_emitted(got, m, c0=0, n=None):
    """emit_packets' outputs of calls c0 .. c0 + n - 1 against the model's, every call and session."""
    start, length, ack, packets = got
    n = start.shape[0] if n is None else n
    sl = slice(c0, c0 + n)
    assert (start == m["start"][sl]).all(), np.argwhere(start != m["start"][sl])[:5]
    assert (length == m["length"][sl]).all(), np.argwhere(length != m["length"][sl])[:5]
    assert (ack == m["ack"][sl]).all(), np.argwhere(ack != m["ack"][sl])[:5]
    body = np.arange(packets.shape[2])[None, None, :] < length[:, :, None]
    assert (np.where(body, packets, 0) == m["packets"][sl]).all()


def assert_state(eng, m):
    last_acked, pending, status, closed = eng.emit_state()
    assert (last_acked == m["last_acked"]).all() and (pending == m["pending"]).all()
    assert (status == m["status"]).all() and (closed == m["closed_call"]).all()


@pytest.mark.parametrize("form,P,local,delay,mp", CASES)
def test_emitted_packets_match_the_model(oracle, monkeypatch, form, P, local, delay, mp):
    """Arrival schedules with stalls (calls at the prediction threshold send nothing) and disconnects
    (the stream closes); the pushes come from the oracle's `advanced`, never from the engine.  The
    whole run emitted in one piece, and -- on a second engine -- in the launches' pieces."""
    set_form(monkeypatch, form)
    rows, arrive, events, ack, resend, m = parity_case(P, local, delay, mp)
    assert (m["start"] >= 0).sum() > S * CALLS // 3 and (m["status"] == E.EMIT_CLOSED).sum() > 5
    assert (m["start"][:, 0][m["start"][:, 0] >= 0][0] == delay)  # the first packet starts at the delay
    one, many = engine(P, local, delay, mp), engine(P, local, delay, mp)
    pieces = []
    done = 0
    for e in (one, many):
        e.add_inputs(0, rows)
        e.add_arrivals(0, arrive, events)
    for n in PIECES:
        one.advance_frames(n)
        many.advance_frames(n)
        pieces.append(many.emit_packets(done, n, ack[done:done + n], resend[done:done + n]))
        done += n
    assert done == CALLS
    got = one.emit_packets(0, CALLS, ack, resend)
    assert_emitted(got, m)
    assert_state(one, m)
    assert_emitted(tuple(np.concatenate([p[i] for p in pieces]) for i in range(4)), m)
    assert_state(many, m)
    frames, skipped, errors = one.sessions()
    assert skipped.sum() > 0
    check_sessions(one, rows, arrive, events, range(0, S, 13), CALLS)


def test_overflow_disconnects_at_the_models_call(oracle):
    """max_pending_inputs 16, acks withheld from a few sessions from call 50 on while their arrivals
    stay prompt: GGRS_EMIT_DISCONNECTED at the model's call, nothing afterwards; the others run on."""
    from oracle import oracle as o
    P, local, mp, calls, maxpend = 2, (0,), 8, 120, 16
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0x0F10), calls, P, 1) for s in range(S)], axis=1)
    arrive = np.repeat(np.maximum(np.arange(calls) - 1, -1)[:, None], S, axis=1).astype(np.int32)
    events = np.zeros((calls, S), np.uint8)
    pushed, stop = pushed_table(o, rows, arrive, events, P, 0b01, 0, mp)
    assert (stop < 0).all()
    ack = np.maximum(np.maximum.accumulate(pushed, axis=0) - 2, -1).astype(np.int32)
    withheld = [3, 64, 65, 129]
    ack[50:, withheld] = -1
    stride = F.max_packet_bytes(1, maxpend)
    m = E.run(rows, pushed, 0b01, maxpend, stride, ack, None, events, recv=arrive)
    assert (m["status"][withheld] == E.EMIT_DISCONNECTED).all() and (m["status"] != 0).sum() == len(withheld)
    assert ((m["closed_call"][withheld] > 60) & (m["closed_call"][withheld] < 75)).all()
    eng = engine(P, local, 0, mp, cap=calls, max_pending=maxpend)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    eng.advance_frames(calls)
    got = eng.emit_packets(0, calls, ack)
    assert_emitted(got, m)
    assert_state(eng, m)
    for s in withheld:
        assert (got[0][m["closed_call"][s]:, s] == -1).all() and (got[1][m["closed_call"][s]:, s] == 0).all()
    frames, skipped, errors = eng.sessions()
    assert (errors == 0).all()


def test_event_closes_the_stream_from_its_call(oracle):
    from oracle import oracle as o
    from ggrs_amd._lib import GGRS_EMIT_CLOSED
    P, local, mp, calls = 3, (1,), 8, 80
    rows = np.stack([o.gen_inputs(o.session_seed(s, 0xC105), calls, P, 0) for s in range(S)], axis=1)
    arrive = np.repeat(np.maximum(np.arange(calls) - 2, -1)[:, None], S, axis=1).astype(np.int32)
    events = np.zeros((calls, S), np.uint8)
    events[40, 5], events[41, 64], events[79, 129] = 1 << 0, 1 << 2, 1 << 0
    pushed, stop = pushed_table(o, rows, arrive, events, P, 0b010, 0, mp)
    ack = np.maximum(np.maximum.accumulate(pushed, axis=0) - 3, -1).astype(np.int32)
    m = E.run(rows, pushed, 0b010, W, F.max_packet_bytes(1, W), ack, None, events, recv=arrive, stop_call=stop)
    eng = engine(P, local, 0, mp, cap=calls)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    eng.advance_frames(calls)
    got = eng.emit_packets(0, calls, ack)
    assert_emitted(got, m)
    last_acked, pending, status, closed = eng.emit_state()
    assert [(int(status[s]), int(closed[s])) for s in (5, 64, 129)] == [(GGRS_EMIT_CLOSED, 40), (GGRS_EMIT_CLOSED, 41),
                                                                       (GGRS_EMIT_CLOSED, 79)]
    assert (status != 0).sum() == 3 and (got[0][40:, 5] == -1).all() and (got[0][39, 5] >= 0)


def test_misuse_raises(oracle):
    from ggrs_amd import InvalidRequest, P2PEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    S_, P = 8, 2

    def fresh(schedule=True):
        e = P2PEngine(S_, num_players=P, local_players=(0,), max_prediction=8, remote_latency=1, input_capacity=32)
        if schedule:
            e.set_arrival_schedule(True)
        return e

    e = fresh(schedule=False)
    with pytest.raises(GgrsError) as err:  # without arrival schedules
        e.set_packet_emit(16)
    assert err.value.code == GGRS_E_STATE
    e = fresh()
    e.add_inputs(0, np.zeros((8, S_, P), np.uint8))
    e.add_arrivals(0, np.full((8, S_), -1, np.int32))
    with pytest.raises(GgrsError) as err:  # emit without set_packet_emit
        e.emit_packets(0, 1)
    assert err.value.code == GGRS_E_STATE
    for bad_n, bad_stride in ((16, 28), (16, 50), (0, 48), (129, 1012), (16, 2048)):
        with pytest.raises(InvalidRequest):
            e.set_packet_emit(bad_n, bad_stride)
    e.set_packet_emit(16)
    with pytest.raises(InvalidRequest):  # call 0 has not run
        e.emit_packets(0, 1)
    e.advance_frames(4)
    with pytest.raises(GgrsError) as err:  # configured after the first call
        e.set_packet_emit(16)
    assert err.value.code == GGRS_E_STATE
    with pytest.raises(InvalidRequest):  # out of order
        e.emit_packets(1, 1)
    with pytest.raises(InvalidRequest):  # not yet run
        e.emit_packets(0, 5)
    start, length, ack, packets = e.emit_packets(0, 2)
    assert (start == 0).all() and (length > 9).all() and (ack == -1).all()
    with pytest.raises(InvalidRequest):  # each call once
        e.emit_packets(1, 1)
    e.emit_packets(2, 2)
    e = P2PEngine(S_, num_players=2, local_players=(), max_prediction=8, remote_latency=1, input_capacity=32)
    e.set_arrival_schedule(True)
    with pytest.raises(InvalidRequest):  # no local player: nothing to send
        e.set_packet_emit(16)


class History:
    """One engine's emitted messages, call by call, in device memory."""

    def __init__(self, calls, S_, stride, dev):
        self.start = torch.full((calls, S_), -1, dtype=torch.int32, device=dev)
        self.length = torch.zeros((calls, S_), dtype=torch.int32, device=dev)
        self.ack = torch.full((calls, S_), -1, dtype=torch.int32, device=dev)
        self.packets = torch.zeros((calls, S_, stride), dtype=torch.uint8, device=dev)

    def row(self, c):
        return self.start[c:c + 1], self.length[c:c + 1], self.ack[c:c + 1], self.packets[c:c + 1]


def route(c, ok, H, lanes):
    """What the poll of call c receives of the other engine's messages (History H): ok [calls][4][S]
    says whether the message of call c - k (k = 1..4) arrives now -- the link tables alone; the
    newest surviving packet and the newest surviving ack_frame, by index arithmetic on the device."""
    sel = torch.full_like(lanes, -1)
    ack = torch.full_like(H.ack[0], -1)
    for k in (4, 3, 2, 1):
        if c - k < 0:
            continue
        here = ok[c, k - 1]
        ack = torch.where(here, torch.maximum(ack, H.ack[c - k]), ack)
        sel = torch.where(here & (H.start[c - k] >= 0), torch.full_like(sel, c - k), sel)
    has = sel >= 0
    idx = sel.clamp(min=0)
    start = torch.where(has, H.start[idx, lanes], torch.full_like(ack, -1))
    length = torch.where(has, H.length[idx, lanes], torch.zeros_like(ack))
    return start[None].contiguous(), length[None].contiguous(), H.packets[idx, lanes][None].contiguous(), ack[None].contiguous()


def test_two_engines_play_each_other_packet_to_packet(oracle):
    """Engines A (local player 0) and B (local player 1), 130 sessions each, stepped call by call:
    each receives what the other emitted, routed through the CPU model test's delay, drop and blackout
    tables; the packets never leave the device.  After 200 lossy calls and a loss-free tail: no
    session has an error; every call's emitted message of either engine equals the modelled peer's
    (whose closed loop tests/test_packet_emit_model.py shows to deliver every sent frame into the
    other side's rows -- the engine's input rows cannot be read back, so the remote columns are
    checked through the oracle's session over the model's rows and arrival tables, which the engines'
    own arrival rows equal); the ring cells of frames both engines confirmed have equal checksums."""
    from tests.test_packet_emit_model import PAIR_CALLS, PAIR_S, pair_case
    rows_a, rows_b, delay, drop, resend, peers = pair_case()
    calls, S_, mp, cap = PAIR_CALLS, PAIR_S, 8, 128
    dev = torch.device("cuda")
    A = engine(2, (0,), 0, mp, cap=cap, feed=True)
    B = engine(2, (1,), 0, mp, cap=cap, feed=True)
    stride = A.out_stride
    assert stride == B.out_stride == A.packet_stride == B.packet_stride
    HA, HB = History(calls, S_, stride, dev), History(calls, S_, stride, dev)
    lanes = torch.arange(S_, device=dev)
    # ok[d][c][k - 1][s]: direction d's message of call c - k arrives at call c
    ok = np.zeros((2, calls, 4, S_), bool)
    for k in range(1, 5):
        ok[:, k:, k - 1] = (delay[:, :calls - k] == k) & ~drop[:, :calls - k]
    ok = torch.from_numpy(ok).to(dev)
    resend_d = torch.from_numpy(resend).to(dev)
    for c in range(calls):
        into_a = route(c, ok[1], HB, lanes)  # B -> A
        into_b = route(c, ok[0], HA, lanes)
        torch.cuda.synchronize()
        for eng, rows, (start, length, packets, ack), H in ((A, rows_a, into_a, HA), (B, rows_b, into_b, HB)):
            eng.add_inputs(c, rows[c:c + 1])
            eng.receive_packets(c, start, length, packets)
            eng.advance_frames(1)
            eng.emit_packets(c, 1, ack, resend_d[c:c + 1], out=H.row(c))
        A.synchronize()
        B.synchronize()
    for eng, H, side, rows in ((A, HA, 0, rows_a), (B, HB, 1, rows_b)):
        frames, skipped, errors = eng.sessions()
        assert (errors == 0).all()
        assert (skipped[::5] > 0).all()  # the blackout sessions hit the prediction threshold
        start, length, ack = H.start.cpu().numpy(), H.length.cpu().numpy(), H.ack.cpu().numpy()
        packets = H.packets.cpu().numpy()
        held = rows.copy()
        arrive = np.zeros((calls, S_), np.int32)
        for s in range(S_):
            X = peers[s][side]
            assert (start[:, s] == X.start).all() and (ack[:, s] == X.ack).all(), s
            for c in range(calls):
                assert length[c, s] == len(X.data[c]) and packets[c, s, :length[c, s]].tobytes() == X.data[c], (s, c)
            held[:, s] = X.rows
            arrive[:, s] = X.arrive
            assert skipped[s] == X.skipped and frames[s] == X.cur, s
        status, eng_arrive = eng.packet_results(calls - cap, cap)
        assert (eng_arrive == arrive[-cap:]).all()
        check_sessions(eng, held, arrive, np.zeros((calls, S_), np.uint8), range(side, S_, 3), calls)
        last_acked, pending, st, closed = eng.emit_state()
        assert (st == 0).all() and (pending <= 2).all()
    confirmed = np.minimum(HA.ack[-1].cpu().numpy(), HB.ack[-1].cpu().numpy())
    compared = 0
    for s in range(S_):
        fa, ca, _ = A.ring(s)
        fb, cb, _ = B.ring(s)
        for f, ck in zip(fa, ca):
            if 0 <= f <= confirmed[s] and f in fb:
                assert ck == cb[list(fb).index(f)], (s, f)
                compared += 1
    assert compared > 3 * S_
