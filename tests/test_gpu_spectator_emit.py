"""GPU parity of the P2P engine's spectator emit (ggrs_p2p_set_spectator_emit /
emit_spectator_packets / read_spectator_emit_state, csrc/p2p_spec_emit.hip) against
tests/spectator_emit_model.py: every call's start_frame, packet_len, packet bytes and note for every
session and endpoint, and the final state -- under arrival schedules whose bursts confirm more than 8
frames in one call, emit split over invocations, overflow, disconnects, stopped sessions, lost rows,
sparse saving, lockstep, both kernel forms, beside the packet feed and packet emit, misuse -- and a
P2P engine streaming to two spectator engines through a lossy link, the packets staying in device
memory."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import packet_feed_model as F  # noqa: E402
from tests import spectator_emit_model as M  # noqa: E402
from tests.test_gpu_p2p_sched import check_sessions, set_form  # noqa: E402

pytestmark = pytest.mark.gpu

S, CALLS, W = 130, 300, 64  # two full waves and a two-session tail; the 128-frame ring wraps
PIECES = (1, 7, 8, 9, CALLS - 25)
STOPPED = (7, 64)  # sessions whose network is silent for 270 calls: the burst is past the device queue

CASES = [
    # form, P, local players, input delay, max_prediction, K, sparse saving
    ("flat", 2, (0,), 0, 12, 1, False),
    ("flat", 4, (0, 2), 1, 12, 3, False),
    ("chains", 2, (1,), 0, 12, 3, False),
    ("chains", 4, (0, 2), 1, 12, 1, False),
    ("flat", 2, (0,), 2, 12, 3, True),
    ("flat", 4, (1, 3), 0, 0, 3, False),  # lockstep mode
]


def engine(P, local, delay, mp, K, cap=CALLS, max_pending=W, sparse=False, feed=False, emit=False, S_=S):
    from ggrs_amd import P2PEngine
    e = P2PEngine(S_, num_players=P, local_players=local, input_delay=delay, max_prediction=mp, remote_latency=1,
                  input_capacity=cap)
    if sparse:
        e.set_sparse_saving(True)
    e.set_arrival_schedule(True)
    if feed:
        e.set_packet_feed(W)
    if emit:
        e.set_packet_emit(W)
    if K:
        e.set_spectator_emit(K, max_pending)
    return e


@functools.lru_cache(maxsize=None)
def parity_case(P, local, delay, mp, K, sparse):
    """Jittered arrivals with stalls of 16 calls (a burst confirms max_prediction + 1 frames: 13), a
    disconnect in every fifth session and a second one in every tenth (P = 4), two stopped sessions,
    random rows (long literal stretches at P = 4)."""
    from oracle import oracle as o
    mask = sum(1 << k for k in local)
    rows = np.random.default_rng(0x5EC + P + delay).integers(0, 256, (CALLS, S, P)).astype(np.uint8)
    arrive, events = M.schedules(S, CALLS, 16, 31 + P + delay, mask, P, disconnect_every=5, second_every=10)
    # (lockstep, mp 0: a session advances on every other call at best while its remote players send at
    # the call rate, so most sessions reach the InputQueue's 128 entries within the run and stop
    # there, in the engine at the oracle's call: tests/test_gpu_p2p_queue_bound.py)
    for s in STOPPED:
        arrive[:, s] = np.maximum(np.arange(CALLS) - 1, -1)
        arrive[:270, s] = -1
        events[:, s] = 0
    pushed, stop = M.pushed_table(rows, arrive, events, P, mask, delay, mp, sparse)
    confirmed = M.confirmed_table(arrive, events, pushed, mask, P)
    ack, resend = M.acks(confirmed, K, 7 + P)
    stride = F.max_packet_bytes(P, W)
    m = M.run(rows, arrive, events, pushed, mask, K, W, stride, ack, resend, stop)
    return rows, arrive, events, ack, resend, stop, m


def assert_emitted(got, m, c0=0):
    """emit_spectator_packets' outputs of calls c0 .. against the model's: every call, endpoint, session."""
    start, length, notes, packets = got
    sl = slice(c0, c0 + start.shape[0])
    assert (start == m["start"][sl]).all(), np.argwhere(start != m["start"][sl])[:5]
    assert (length == m["length"][sl]).all(), np.argwhere(length != m["length"][sl])[:5]
    assert (notes == m["notes"][sl]).all(), np.argwhere(notes != m["notes"][sl])[:5]
    body = np.arange(packets.shape[3])[None, None, None, :] < length[..., None]
    assert (np.where(body, packets, 0) == m["packets"][sl]).all()


def assert_state(eng, m):
    nxt, last_acked, pending, status, closed = eng.read_spectator_emit_state()
    assert (nxt == m["next"]).all(), np.argwhere(nxt != m["next"])[:5]
    assert (last_acked == m["last_acked"]).all() and (pending == m["pending"]).all()
    assert (status == m["status"]).all() and (closed == m["closed_call"]).all()


def longest_literal(packet):
    """The longest literal stretch among a packet's bitfield-rle runs."""
    n = int.from_bytes(packet[1:9], "little")
    rle, q, best = packet[9:9 + n], 0, 0
    while q < len(rle):
        h, shift = 0, 0
        while True:
            b = int(rle[q])
            q += 1
            h |= (b & 0x7f) << shift
            shift += 7
            if not b & 0x80:
                break
        if not h & 1:
            best = max(best, h >> 1)
            q += h >> 1
    return best


@pytest.mark.parametrize("form,P,local,delay,mp,K,sparse", CASES)
def test_spectator_packets_match_the_model(oracle, monkeypatch, form, P, local, delay, mp, K, sparse):
    """The pushes come from the oracle's `advanced`, never from the engine.  The whole run emitted in
    one invocation, and -- on a second engine -- in pieces of 1, 7, 8, 9 and the rest."""
    set_form(monkeypatch, form)
    rows, arrive, events, ack, resend, stop, m = parity_case(P, local, delay, mp, K, sparse)
    assert (stop[list(STOPPED)] == 270).all() and (m["start"][270:, :, list(STOPPED)] == -1).all()
    assert (m["start"] >= 0).sum() > S * K * CALLS // 3 and (m["status"] == 0).all()
    if mp:
        assert m["npush"].max() > 8  # one call confirms more than 8 frames
    gone = (events != 0).any(axis=0) & (stop < 0)
    assert gone.sum() >= 10 and (m["notes"][-1, gone] != 0).all() and (m["notes"][:, ~gone & (stop < 0)] == 0).all()
    if P == 4:
        both = ((events != 0).sum(axis=0) == 2) & (stop < 0)
        assert both.sum() >= 8 and all(len(set(m["notes"][-2:, s])) == 2 for s in np.nonzero(both)[0])  # the rotation
        # acks withheld for 30 calls: a literal stretch with the two-byte header
        assert max(longest_literal(m["packets"][c, 0, s]) for c in range(110, 120) for s in range(1, S, 4)) >= 64
    one, many = (engine(P, local, delay, mp, K, sparse=sparse) for _ in range(2))
    for e in (one, many):
        e.add_inputs(0, rows)
        e.add_arrivals(0, arrive, events)
    pieces, done = [], 0
    for n in PIECES:
        one.advance_frames(n)
        many.advance_frames(n)
        pieces.append(many.emit_spectator_packets(done, n, ack[done:done + n], resend[done:done + n]))
        done += n
    assert done == CALLS
    assert_emitted(one.emit_spectator_packets(0, CALLS, ack, resend), m)
    assert_state(one, m)
    assert_emitted(tuple(np.concatenate([p[i] for p in pieces]) for i in range(4)), m)
    assert_state(many, m)
    frames, skipped, errors = one.sessions()
    assert (errors[list(STOPPED)] != 0).all() and (errors != 0).sum() == (stop >= 0).sum()
    check_sessions(one, rows, arrive, events, range(0, S, 13), CALLS, sparse_saving=sparse)


def steady(P, calls, lag=1, seed=0x0F1):
    rows = np.random.default_rng(seed).integers(0, 256, (calls, S, P)).astype(np.uint8)
    arrive = np.repeat(np.maximum(np.arange(calls) - lag, -1)[:, None], S, axis=1).astype(np.int32)
    return rows, arrive, np.zeros((calls, S), np.uint8)


def test_overflow_closes_one_endpoint_and_its_siblings_run_on(oracle):
    """max_pending_inputs 4, endpoint 1 never acks: GGRS_EMIT_DISCONNECTED on it at the model's call,
    byte-exact packets on endpoints 0 and 2 to the end."""
    P, local, mp, calls, K = 2, (0,), 8, 60, 3
    rows, arrive, events = steady(P, calls)
    pushed, stop = M.pushed_table(rows, arrive, events, P, 0b01, 0, mp)
    confirmed = M.confirmed_table(arrive, events, pushed, 0b01, P)
    ack = np.repeat(np.maximum(confirmed - 1, -1)[:, None, :], K, axis=1).astype(np.int32)
    ack[:, 1] = -1
    stride = F.max_packet_bytes(P, 4)
    m = M.run(rows, arrive, events, pushed, 0b01, K, 4, stride, ack, None, stop)
    assert (m["status"][1] == M.EMIT_DISCONNECTED).all() and (m["status"][[0, 2]] == 0).all()
    assert (m["closed_call"][1] == 5).all() and (m["pending"][1] == 5).all() and (m["start"][-1, [0, 2]] >= 0).all()
    eng = engine(P, local, 0, mp, K, cap=calls, max_pending=4)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    eng.advance_frames(calls)
    got = eng.emit_spectator_packets(0, calls, ack)
    assert_emitted(got, m)
    assert_state(eng, m)
    assert (got[0][5:, 1] == -1).all() and (got[1][5:, 1] == 0).all()
    assert (eng.sessions()[2] == 0).all()


def test_disconnect_blanks_later_frames_and_confirmed_jumps(oracle):
    """Local player 1; player 0 is silent from frame 20 on and disconnects at call 40 in session 5:
    confirmed jumps from 20 to the local player's last frame, the frames after 20 carry a blank byte
    for player 0 (decoded from the last emitted packet, nothing acked), and the note stands on every
    later call."""
    from tests import spectator_model as SM
    P, local, mp, calls, K = 2, (1,), 8, 60, 1
    rows, arrive, events = steady(P, calls, lag=2)
    arrive[23:, 5] = 20
    events[40, 5] = 1 << 0
    pushed, stop = M.pushed_table(rows, arrive, events, P, 0b10, 0, mp)
    m = M.run(rows, arrive, events, pushed, 0b10, K, W, F.max_packet_bytes(P, W), None, None, stop)
    assert stop[5] < 0 and (m["confirmed"][39, 5], m["npush"][39, 5]) == (20, 0) and m["npush"][40, 5] >= mp
    assert (m["notes"][40:, 5] == SM.note(0, 20)).all() and (m["notes"][:40, 5] == 0).all()
    eng = engine(P, local, 0, mp, K, cap=calls)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    eng.advance_frames(calls)
    got = eng.emit_spectator_packets(0, calls)
    assert_emitted(got, m)
    assert_state(eng, m)
    rc, inputs = F.codec_decode(bytes(P), got[3][-1, 0, 5, :got[1][-1, 0, 5]].tobytes())  # nothing acked: from frame 0
    assert rc == 0 and got[0][-1, 0, 5] == 0 and len(inputs) == m["next"][5] > 40
    for f, b in enumerate(inputs):
        assert b[0] == (rows[f, 5, 0] if f <= 20 else 0), f
    assert any(b[1] for b in inputs[21:])


def test_lost_rows_close_the_endpoints(oracle):
    """input_capacity 64, arrivals two calls late: calls 0..39 are emitted in time; 60 more calls are
    run (and their rows added) before the emit of call 40, which must push frame 38 -- its row slot
    holds frame 102 by then: GGRS_EMIT_ROW_LOST on every endpoint at call 40, nothing afterwards."""
    from ggrs_amd._lib import GGRS_EMIT_ROW_LOST
    P, local, mp, calls, K, cap = 2, (0,), 8, 104, 2, 64
    rows, arrive, events = steady(P, calls, lag=2)
    pushed, stop = M.pushed_table(rows, arrive, events, P, 0b01, 0, mp)
    held = np.where(np.arange(calls) < 40, 0, calls - cap)
    m = M.run(rows, arrive, events, pushed, 0b01, K, W, F.max_packet_bytes(P, W), None, None, stop, held_from=held)
    assert GGRS_EMIT_ROW_LOST == M.EMIT_ROW_LOST and (m["status"] == M.EMIT_ROW_LOST).all()
    assert (m["closed_call"] == 40).all() and (m["next"] == 38).all() and (m["start"][39] == 0).all()
    eng = engine(P, local, 0, mp, K, cap=cap)
    eng.add_inputs(0, rows[:cap])
    eng.add_arrivals(0, arrive[:cap], events[:cap])
    eng.advance_frames(44)
    first = eng.emit_spectator_packets(0, 40)
    eng.add_inputs(cap, rows[cap:])
    eng.add_arrivals(cap, arrive[cap:], events[cap:])
    eng.advance_frames(calls - 44)
    rest = eng.emit_spectator_packets(40, calls - 40)
    assert_emitted(first, m)
    assert_emitted(rest, m, 40)
    assert_state(eng, m)
    assert (rest[0] == -1).all() and (eng.sessions()[2] == 0).all()


def test_beside_packet_feed_and_packet_emit_the_peer_facing_outputs_are_unchanged(oracle):
    """Two engines with the packet feed and packet emit, one of them with spectator emit too, fed the
    same packets: equal peer-facing outputs and states; the spectator packets are the model's over the
    feed's arrival rows."""
    from tests import packet_emit_model as E
    P, local, mp, calls, K = 2, (0,), 8, 120, 2
    rows = np.random.default_rng(0xFEED).integers(0, 256, (calls, S, P)).astype(np.uint8)
    want, _ = M.schedules(S, calls, 12, 77, 0b01, P, disconnect_every=0)
    stride = F.max_packet_bytes(1, W)
    start = np.full((calls, S), -1, np.int32)
    length = np.zeros((calls, S), np.int32)
    packets = np.zeros((calls, S, stride), np.uint8)
    for s in range(S):  # the remote peer's packets: the frames since the last delivery, against the one before
        last = -1
        for c in range(calls):
            upto = int(want[c, s])
            if upto > last:
                first = max(last + 1, upto - W + 1)
                ref = bytes([rows[first - 1, s, 1]]) if first else bytes(1)
                data = oracle.codec_encode(ref, [bytes([rows[f, s, 1]]) for f in range(first, upto + 1)])
                start[c, s], length[c, s] = first, len(data)
                packets[c, s, :len(data)] = np.frombuffer(data, np.uint8)
                last = upto
    with_spec, without = engine(P, local, 0, mp, K, cap=calls, feed=True, emit=True), engine(P, local, 0, mp, 0, cap=calls,
                                                                                             feed=True, emit=True)
    outs = []
    for e in (with_spec, without):
        e.add_inputs(0, rows)
        e.receive_packets(0, start, length, packets)
        e.advance_frames(calls)
        outs.append(e.emit_packets(0, calls))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert (a == b).all()
    body = np.arange(outs[0][3].shape[2])[None, None, :] < outs[0][1][:, :, None]  # (bytes past packet_len: unspecified)
    assert (outs[0][0] >= 0).sum() > S * calls // 2 and (np.where(body, outs[0][3], 0) == np.where(body, outs[1][3], 0)).all()
    assert all((a == b).all() for a, b in zip(with_spec.emit_state(), without.emit_state()))
    assert (with_spec.states() == without.states()).all() and (with_spec.sessions()[2] == 0).all()
    arrive = np.maximum.accumulate(want, axis=0).astype(np.int32)
    status, fed = with_spec.packet_results(0, calls)
    assert (fed == arrive).all()
    events = np.zeros((calls, S), np.uint8)
    pushed, stop = M.pushed_table(rows, arrive, events, P, 0b01, 0, mp)
    m = M.run(rows, arrive, events, pushed, 0b01, K, W, F.max_packet_bytes(P, W), None, None, stop)
    assert_emitted(with_spec.emit_spectator_packets(0, calls), m)
    assert_state(with_spec, m)


def test_misuse_raises(oracle):
    from ggrs_amd import InvalidRequest, P2PEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    from ggrs_amd.p2p import peer_report
    S_, P = 8, 3

    def fresh(schedule=True, local=(0,)):
        e = P2PEngine(S_, num_players=P, local_players=local, max_prediction=8, remote_latency=1, input_capacity=32)
        if schedule:
            e.set_arrival_schedule(True)
        return e

    def state_error(f, *a):
        with pytest.raises(GgrsError) as err:
            f(*a)
        assert err.value.code == GGRS_E_STATE

    state_error(fresh(schedule=False).set_spectator_emit, 1, 16)  # a fixed-latency engine
    e = fresh()
    e.add_inputs(0, np.zeros((8, S_, P), np.uint8))
    e.add_arrivals(0, np.repeat(np.arange(-1, 7, dtype=np.int32)[:, None], S_, axis=1))  # a lag of one call
    state_error(e.emit_spectator_packets, 0, 1)  # emit without set_spectator_emit
    need = F.max_packet_bytes(P, 16)
    for k, n, stride in ((0, 16, None), (5, 16, None), (1, 0, 64), (1, 129, 1012), (1, 16, need - 4), (1, 16, need + 2),
                         (1, 16, 2048)):
        with pytest.raises(InvalidRequest):
            e.set_spectator_emit(k, n, stride)
    e.set_spectator_emit(2, 16)
    rep = np.zeros((1, S_), np.int32)
    rep[0, 0] = peer_report(1, 2, -1)
    state_error(e.add_peer_reports, 0, rep)  # peer reports with spectator emit
    with pytest.raises(InvalidRequest):  # call 0 has not run
        e.emit_spectator_packets(0, 1)
    e.advance_frames(4)
    state_error(e.set_spectator_emit, 2, 16)  # configured after the first call
    with pytest.raises(InvalidRequest):  # out of order
        e.emit_spectator_packets(1, 1)
    with pytest.raises(InvalidRequest):  # not yet run
        e.emit_spectator_packets(0, 5)
    start, length, notes, packets = e.emit_spectator_packets(0, 3)
    assert start.shape == (3, 2, S_) and (start[0] == -1).all() and (start[1:] == 0).all() and (notes == 0).all()
    with pytest.raises(InvalidRequest):  # each call once
        e.emit_spectator_packets(2, 1)
    e.emit_spectator_packets(3, 1)
    e = fresh()
    e.add_inputs(0, np.zeros((8, S_, P), np.uint8))
    e.add_arrivals(0, np.full((8, S_), -1, np.int32))
    e.add_peer_reports(0, rep)
    state_error(e.set_spectator_emit, 1, 16)  # spectator emit after peer reports
    with pytest.raises(InvalidRequest):  # no local player: no session hosts spectators
        fresh(local=()).set_spectator_emit(1, 16)


def test_p2p_engine_streams_to_two_spectator_engines_in_device_memory(oracle):
    """A P2P engine (130 sessions, two spectator endpoints each) emits with on_device = 1; a torch
    link drops and delays its packets per (call, endpoint, session) and hands back the InputAcks the
    spectator engines report; the two spectator engines receive with on_device = 1.  Every
    spectator's per-call trace, final state, current_frame and last_recv equal those of a spectator
    engine fed the model's confirmed rows and arrival table through add_inputs / add_arrivals."""
    from ggrs_amd import SpectatorEngine
    from tests.test_spectator_emit_model import E2E, e2e_case, notes_taken, spectate
    k = E2E
    S_, K, P, calls = k["S"], k["K"], k["P"], k["calls"]
    rows, arrive, events, delay, drop, ack_drop, resend, runs = e2e_case()
    # the condition, on the model alone: every spectator advances, none is lost, no endpoint closes
    recv = np.stack([r["recv"] for r in runs], axis=2)  # [calls][K][S]
    notes_in = np.stack([np.stack([notes_taken(r, j) for j in range(K)]) for r in runs], axis=2).transpose(1, 0, 2)
    for s, r in enumerate(runs):
        for j in range(K):
            sp, adv, _, _ = spectate(recv[:, j, s], notes_in[:, j, s], r["receivers"][j].rows, P)
            assert sp.error == 0 and adv.sum() > 0 and r["session"].eps[j].status == 0, (s, j)
    nxt = np.array([r["session"].host.next for r in runs])
    conf_rows = np.zeros((calls, S_, P), np.uint8)
    for s, r in enumerate(runs):
        for f, b in r["pushes"].items():
            conf_rows[f, s] = np.frombuffer(b, np.uint8)

    dev = torch.device("cuda")
    host = engine(P, k["local"], 0, k["mp"], K, cap=256, S_=S_)
    stride = host.spectator_stride
    spectators = []
    for j in range(K):
        sp = SpectatorEngine(S_, num_players=P, input_capacity=256, trace_capacity=calls)
        sp.set_packet_feed(k["mp"], k["W"])
        assert sp.packet_stride == stride
        spectators.append(sp)
    H_start = torch.full((calls, K, S_), -1, dtype=torch.int32, device=dev)
    H_len = torch.zeros((calls, K, S_), dtype=torch.int32, device=dev)
    H_notes = torch.zeros((calls, S_), dtype=torch.int32, device=dev)
    H_pk = torch.zeros((calls, K, S_, stride), dtype=torch.uint8, device=dev)
    # ok[c][d - 1][k][s]: the host's packet of call c - d arrives at spectator k's call c
    ok = np.zeros((calls, 3, K, S_), bool)
    for d in range(1, 4):
        ok[d:, d - 1] = (delay[:calls - d] == d) & ~drop[:calls - d]
    ok = torch.from_numpy(ok).to(dev)
    resend_d = torch.from_numpy(resend).to(dev)
    ack_drop_d = torch.from_numpy(ack_drop).to(dev)
    lanes = torch.arange(S_, device=dev)
    acks = torch.full((1, K, S_), -1, dtype=torch.int32, device=dev)
    for c in range(calls):
        host.add_inputs(c, rows[c:c + 1])
        host.add_arrivals(c, arrive[c:c + 1], events[c:c + 1])
        host.advance_frames(1)
        ack_in = torch.where(ack_drop_d[c:c + 1], torch.full_like(acks, -1), acks).contiguous()
        host.emit_spectator_packets(c, 1, ack_in, resend_d[c:c + 1].contiguous(),
                                    out=(H_start[c:c + 1], H_len[c:c + 1], H_notes[c:c + 1], H_pk[c:c + 1]))
        host.synchronize()
        new_acks = []
        for j, sp in enumerate(spectators):
            sel = torch.full_like(lanes, -1)
            for d in (3, 2, 1):  # the newest surviving packet that arrives now
                if c - d >= 0:
                    sel = torch.where(ok[c, d - 1, j] & (H_start[c - d, j] >= 0), torch.full_like(sel, c - d), sel)
            has, idx = sel >= 0, sel.clamp(min=0)
            start = torch.where(has, H_start[idx, j, lanes], torch.full_like(H_start[0, j], -1))[None].contiguous()
            length = torch.where(has, H_len[idx, j, lanes], torch.zeros_like(H_len[0, j]))[None].contiguous()
            notes = torch.where(has, H_notes[idx, lanes], torch.zeros_like(H_notes[0]))[None].contiguous()
            packets = H_pk[idx, j, lanes][None].contiguous()
            torch.cuda.synchronize()
            sp.receive_packets(c, start, length, packets, notes)
            sp.advance_frames(1)
            new_acks.append(sp.read_packet_results(c, 1)[1][0])  # the InputAck: last_recv after the call
        acks = torch.from_numpy(np.stack(new_acks)[None]).to(dev)
    m_start = np.stack([r["start"] for r in runs], axis=2)
    assert (H_start.cpu().numpy() == m_start).all() and (host.sessions()[2] == 0).all()
    state = host.read_spectator_emit_state()
    assert (state[0] == nxt).all() and (state[3] == 0).all()
    for j, sp in enumerate(spectators):
        ref = SpectatorEngine(S_, num_players=P, input_capacity=256, trace_capacity=calls)
        ref.add_inputs(0, conf_rows)
        ref.add_arrivals(0, recv[:, j], notes_in[:, j])
        ref.advance_frames(calls)
        for a, b in zip(sp.trace(0, calls), ref.trace(0, calls)):
            assert (a == b).all(), j
        got, want = sp.sessions(), ref.sessions()
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[3] == 0).all() and (want[3] == 0).all()
        assert (got[0] >= 0).all() and (sp.states() == ref.states()).all()
