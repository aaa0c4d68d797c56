"""GPU parity of the endpoint poll (ggrs_p2p_set_endpoint_poll / poll_endpoints / read_endpoint_state,
csrc/p2p_poll.hip) against tests/endpoint_poll_model.py: every output of every call and session and the
endpoints' state under three clocks and six kinds of link, split over launches in several ways, from
host arrays and device tensors; the packet feed's dropped packets; the timeout reaching the session
(against an engine given the same events bytes by the host, and the oracle); misuse; and an engine
without the unit.  The events rows have no read-back of their own: they are compared through the units
that read them (time sync's and packet emit's closing call, the sessions' states)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import endpoint_poll_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

S, CALLS, CAP, MP = M.CASE_S, M.CASE_CALLS, 64, 8
NAMES = ("resend", "send_ack", "send_report", "net_events")


def engine(cap=CAP, S_=S, poll=True, time_sync=False, emit=False, feed=False, start=M.CASE_START,
           timeout=M.CASE_TIMEOUT, notify=M.CASE_NOTIFY):
    from ggrs_amd import P2PEngine
    e = P2PEngine(S_, num_players=2, local_players=(0,), input_delay=0, max_prediction=MP, remote_latency=1,
                  input_capacity=cap)
    e.set_arrival_schedule(True)
    if feed:
        e.set_packet_feed(64)
    if emit:
        e.set_packet_emit(64)
    if time_sync:
        e.set_time_sync(60)
    if poll:
        e.set_endpoint_poll(timeout, notify, start)
    return e


def plain_rows(calls=CALLS, S_=S, seed=3):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 16, (calls, S_, 2), dtype=np.uint8)
    # frame c arrives at call c: a call reaches back one row only (the prediction's base)
    arrive = np.repeat(np.arange(calls)[:, None], S_, axis=1).astype(np.int32)
    return rows, arrive


def pieces_of(pieces, calls):
    done, i = 0, 0
    while done < calls:
        n = min(pieces[i % len(pieces)], calls - done)
        yield done, n
        done, i = done + n, i + 1


def drive(eng, rows, arrive, events, now, kinds, pieces, device, after=None):
    """The run in pieces: a piece's arrivals, its polls in one launch, then its inputs and calls -- at
    most 32 at a time, so that a piece as long as the row ring leaves the rows its first calls reach
    back for (a device piece and a host piece alternate with device="both").  -> the unit's four
    outputs, [calls][S] each."""
    calls = len(now)
    out = [np.zeros((calls, S), np.uint8) for _ in range(4)]
    for i, (c0, n) in enumerate(pieces_of(pieces, calls)):
        sl = slice(c0, c0 + n)
        eng.add_arrivals(c0, arrive[sl], events[sl])
        if device is True or (device == "both" and i % 2 == 0):
            d_now = torch.from_numpy(now[sl].view(np.int64).copy()).cuda()
            d_kinds = torch.from_numpy(kinds[sl].copy()).cuda()
            d_out = tuple(torch.zeros((n, S), dtype=torch.uint8, device="cuda") for _ in range(4))
            eng.poll_endpoints(c0, n, d_now, d_kinds, out=d_out)
            eng.synchronize()
            got = [t.cpu().numpy() for t in d_out]
        else:
            got = eng.poll_endpoints(c0, n, now[sl], kinds[sl])
        for o, g in zip(out, got):
            o[sl] = g
        for h0, hn in pieces_of((32,), n):
            eng.add_inputs(c0 + h0, rows[c0 + h0:c0 + h0 + hn])
            eng.advance_frames(hn)
        if after:
            after(c0, n)
    return out


def assert_outputs(got, m):
    for name, g in zip(NAMES, got):
        assert (g == m[name]).all(), (name, np.argwhere(g != m[name])[:5])


def assert_state(eng, model):
    for name, g, w in zip(("state", "last_recv", "last_input_recv", "last_report", "shutdown", "flags", "closed_call"),
                          eng.endpoint_state(), model.fields()):
        assert g.dtype == w.dtype and (g == w).all(), (name, np.argwhere(g != w)[:5])


def first_event_call(events_after, rmask=M.CASE_RMASK):
    """The first call whose events row holds a remote bit (-1): where the other units close."""
    hit = (events_after & rmask) != 0
    return np.where(hit.any(axis=0), hit.argmax(axis=0), -1).astype(np.int32)


# ---- 1. parity per call and session

@pytest.mark.parametrize("pieces,device", [((64,), False), ((1,), True), ((1, 3, 8, 13, 64), "both")])
@pytest.mark.parametrize("kind", M.CLOCKS)
def test_every_output_and_the_state_match_the_model(kind, pieces, device):
    now, kinds, events = M.gpu_case(kind)
    m = M.case_run(kind)
    M.assert_case_is_not_vacuous(kind, m)  # (checked on the CPU as well: parity cannot pass vacuously)
    rows, arrive = plain_rows()
    eng = engine(time_sync=True)
    got = drive(eng, rows, arrive, events, now, kinds, pieces, device,
                after=lambda c0, n: eng.time_sync(c0, n))
    assert_outputs(got, m)
    assert_state(eng, m["model"])
    # the events rows, the timeouts' bits included, as time sync read them
    assert (eng.time_sync_state()[4] == first_event_call(m["events"])).all()
    assert (eng.sessions()[2] == 0).all()
    # one call more, from the device, with a clock from the past: it is taken as the engine's last clock
    d_now = torch.tensor([int(now[0])], dtype=torch.int64).cuda()
    eng.add_inputs(CALLS, rows[:1])
    eng.add_arrivals(CALLS, arrive[-1:] + 1, events[:1] * 0)
    out = tuple(torch.zeros((1, S), dtype=torch.uint8, device="cuda") for _ in range(4))
    eng.poll_endpoints(CALLS, 1, d_now, torch.zeros((1, S), dtype=torch.uint8, device="cuda"), out=out)
    eng.synchronize()
    want = M.run(S, 0, 0, 0, M.CASE_RMASK, now[:1], np.zeros((1, S), np.uint8), np.zeros((1, S), np.uint8),
                 first_call=CALLS, model=m["model"])
    assert want["model"].clock == now[-1]
    assert_outputs([t.cpu().numpy() for t in out], want)
    assert_state(eng, want["model"])


# ---- 2. the packet feed: a dropped packet is no decoded Input

def test_dropped_packets_give_no_ack_and_do_not_reset_the_retry_timer(oracle):
    from tests import packet_feed_model as F
    calls, mask = CALLS, 0b01
    rows, arrive, _ = F.damage_case(S=S, calls=calls, P=2, local_mask=mask, max_prediction=MP)
    rng = np.random.default_rng(21)
    damage = {}
    for s in range(0, S, 2):  # a dozen damaged packets in every second session, where the sender sends
        rises = np.nonzero(arrive[1:, s] > arrive[:-1, s])[0] + 1
        for c in rng.choice(rises, 12, replace=False):
            damage[(int(c), s)] = ("truncate", "random")[int(c) % 2]
    pk = F.run(rows, arrive, mask, MP, seed=9, damage=damage)
    assert (pk["stop_call"] < 0).all()
    # 250 ms a call: one call without a decoded Input is enough for the retry timer
    now = np.uint64(M.CASE_START) + np.arange(calls).astype(np.uint64) * np.uint64(250)
    kinds = np.where(pk["start"] >= 0, M.K_INPUT, 0).astype(np.uint8)
    events = np.zeros((calls, S), np.uint8)
    eng = engine(cap=calls, feed=True, timeout=1 << 20, notify=1 << 20)
    eng.add_inputs(0, rows)
    got = [np.zeros((calls, S), np.uint8) for _ in range(4)]
    for c0, n in pieces_of((1, 3, 8, 13, 64), calls):
        sl = slice(c0, c0 + n)
        eng.receive_packets(c0, pk["start"][sl], pk["length"][sl], pk["packets"][sl])
        for g, o in zip(got, eng.poll_endpoints(c0, n, now[sl], kinds[sl])):
            g[sl] = o
        eng.advance_frames(n)
    status, _ = eng.packet_results(0, calls)
    assert (status == pk["status"]).all()
    dropped = (status < 0) & (kinds != 0)
    assert dropped.sum() > S
    m = M.run(S, 1 << 20, 1 << 20, M.CASE_START, M.CASE_RMASK, now, kinds, events, status=status)
    assert_outputs(got, m)
    assert_state(eng, m["model"])
    assert not got[1][dropped].any() and got[1][(status >= 0) & (kinds != 0)].all()
    blind = M.run(S, 1 << 20, 1 << 20, M.CASE_START, M.CASE_RMASK, now, kinds, events)  # every packet taken as decoded
    assert (blind["resend"] != m["resend"]).sum() > S // 4  # the drops moved retries
    assert (eng.sessions()[2] == 0).all()


# ---- 3. the timeout reaches the session

@pytest.mark.parametrize("form", ["chains", "flat"])
def test_a_timed_out_player_is_disconnected_by_the_call_itself(oracle, monkeypatch, form):
    """Engine A's events come from the unit (the class-3 timeouts on top of the class-4 requests);
    engine B gets the model's events bytes from the host and no unit; the oracle's P2PSession runs on
    those bytes.  With emit and time sync on A, both close at the unit's closing call."""
    from ggrs_amd._lib import GGRS_EMIT_CLOSED
    from tests.test_gpu_p2p_packets import assert_same
    from tests.test_gpu_p2p_sched import check_sessions, schedules, set_form
    set_form(monkeypatch, form)
    now, kinds, events = M.gpu_case("jitter")
    m = M.case_run("jitter")
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 0xE9D), CALLS, 2, 0) for s in range(S)], axis=1)
    arrive, _ = schedules(S, CALLS, MP, 31, 0b01, 2, disconnect_every=0)
    A, B = engine(time_sync=True, emit=True), engine(poll=False)
    acks = np.repeat(np.arange(CALLS, dtype=np.int32)[:, None], S, axis=1)

    def after(c0, n):
        A.emit_packets(c0, n, acks[c0:c0 + n])
        A.time_sync(c0, n)

    got = drive(A, rows, arrive, events, now, kinds, (1, 3, 8, 13), False, after=after)
    assert_outputs(got, m)
    for c0, n in pieces_of((1, 3, 8, 13), CALLS):
        B.add_inputs(c0, rows[c0:c0 + n])
        B.add_arrivals(c0, arrive[c0:c0 + n], m["events"][c0:c0 + n])
        B.advance_frames(n)
    timed_out = (m["net_events"] & M.NET_DISCONNECTED).any(axis=0)
    assert timed_out.sum() >= S // 6 and (m["events"] != events).sum() == timed_out.sum()
    assert_same(A, B)
    assert A.stats()[0][timed_out].sum() > 0  # the disconnects rolled sessions back
    check_sessions(A, rows, arrive, m["events"], range(0, S, 2), CALLS)
    closed = A.endpoint_state()[6]
    assert (closed == first_event_call(m["events"])).all() and (closed >= 0).sum() > S // 4
    assert (A.time_sync_state()[4] == closed).all()
    _, _, emit_status, emit_closed = A.emit_state()
    assert (emit_closed == closed).all() and (emit_status[closed >= 0] == GGRS_EMIT_CLOSED).all()
    assert (emit_status[closed < 0] == 0).all()


# ---- 5. misuse

def test_misuse(oracle):
    from ggrs_amd import P2PEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError, InvalidRequest
    rows, arrive = plain_rows(8)
    events = np.zeros((8, S), np.uint8)
    now = M.case_clock("const8", 8)

    def state_error(fn):
        with pytest.raises(GgrsError) as e:
            fn()
        assert e.value.code == GGRS_E_STATE, e.value

    plain = engine(poll=False)
    plain.add_inputs(0, rows)
    plain.add_arrivals(0, arrive, events)
    state_error(lambda: plain.poll_endpoints(0, 1, now[:1]))          # unconfigured
    state_error(plain.endpoint_state)
    plain.advance_frames(1)
    state_error(lambda: plain.set_endpoint_poll(640, 160, 0))         # after the first call
    fixed = P2PEngine(S, num_players=2, local_players=(0,), max_prediction=MP, remote_latency=2, input_capacity=CAP)
    state_error(lambda: fixed.set_endpoint_poll(640, 160, 0))         # a fixed-latency engine
    with pytest.raises(InvalidRequest):
        engine(timeout=100, notify=101)                               # the reference's subtraction panics
    engine(timeout=100, notify=100)
    eng = engine()
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive[:6], events[:6])
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(1, 1, now[1:2])                            # out of order
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(0, 7, now[:7])                             # call 6 has no arrivals yet
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(0, 2, now[:2][::-1].copy())                # a host clock that decreases
    state_error(lambda: eng.advance_frames(1))                        # call 0 was not polled
    assert eng.calls() == 0
    eng.poll_endpoints(0, 2, now[:2])
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(1, 1, now[1:2])                            # repeated
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(2, 1, now[:1])                             # below the last host clock
    eng.advance_frames(2)
    state_error(lambda: eng.advance_frames(1))                        # call 2 was not polled
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(1, 1, now[2:3])                            # already run
    assert eng.calls() == 2
    eng.poll_endpoints(2, 4, now[2:6])
    eng.advance_frames(4)
    # nothing above changed the endpoints: the six polls that ran are the model's
    m = M.run(S, M.CASE_TIMEOUT, M.CASE_NOTIFY, M.CASE_START, M.CASE_RMASK, now[:6], np.zeros((6, S), np.uint8), events[:6])
    assert_state(eng, m["model"])


# ---- 6. an engine without the unit is unchanged

def test_links_that_never_go_silent_leave_the_engine_as_it_was(oracle):
    from tests.test_gpu_p2p_packets import assert_same
    from tests.test_gpu_p2p_sched import schedules
    now = M.case_clock("jitter")
    kinds = np.full((CALLS, S), M.K_INPUT, np.uint8)
    rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 0xE9E), CALLS, 2, 0) for s in range(S)], axis=1)
    arrive, events = schedules(S, CALLS, MP, 33, 0b01, 2)  # (its own disconnect requests in every fifth session)
    A, B = engine(time_sync=True), engine(poll=False, time_sync=True)
    got = drive(A, rows, arrive, events, now, kinds, (13, 8), "both", after=lambda c0, n: A.time_sync(c0, n))
    for c0, n in pieces_of((13, 8), CALLS):
        B.add_inputs(c0, rows[c0:c0 + n])
        B.add_arrivals(c0, arrive[c0:c0 + n], events[c0:c0 + n])
        B.advance_frames(n)
        B.time_sync(c0, n)
    assert not (got[3] & (M.NET_INTERRUPTED | M.NET_RESUMED | M.NET_DISCONNECTED)).any() and not got[0].any()
    assert_same(A, B)
    for a, b in zip(A.time_sync_state(), B.time_sync_state()):  # (the events rows as time sync read them)
        assert (a == b).all()
    assert (A.endpoint_state()[6] == first_event_call(events)).all()


# ---- 4. closed loop: two engines, datagram to datagram, no host-made flag

def test_two_engines_play_each_other_with_the_units_flags(oracle):
    """The datagram-to-datagram loop of tests/test_gpu_wire.py with resend, send_ack and send_report
    taken from each side's unit.  16 ms a call: notify is 10 calls, the timeout 40.  Every fifth
    session's link blacks out both ways, alternately for 20 calls (17 to 33 calls of silence at the
    receiver) and for good; the other links lose 15 % of their datagrams.  Each side's recorded unit
    inputs, replayed through the model, give its recorded outputs; a short blackout raises
    INTERRUPTED then RESUMED on both sides and nothing else, a long one INTERRUPTED then DISCONNECTED
    (at the model's calls, by the replay), the other sessions nothing; emit and time sync close at
    the unit's call; no session has an error, and the timed-out sessions play on alone.  Final
    states, rings, rollback counts and frames equal the oracle's P2PSession run on the events rows
    the units produced, for every blacked-out session and every third of the others: the arrival
    rows are the feed's ack rows, the rows a side holds are its own local inputs and, at frame f, the
    peer's input of the call that queued f -- which calls queue which frame follows from the peer's
    arrival and events rows alone (the oracle's `advanced`), not from any input byte.
    input_capacity is 256 for 240 calls, on purpose: a link that stays silent keeps the row of the
    last frame it delivered in use, and the scheduled launch stops such a session
    (GGRS_E_PRECONDITION) once the row ring has wrapped over that row, input_capacity calls after the
    blackout began -- so "play on alone" is shown here for fewer calls than that (include/ggrs_amd.h,
    "Endpoint poll")."""
    from ggrs_amd import wire
    from tests.test_gpu_p2p_emit import History
    from tests import packet_emit_model as E
    from tests.test_gpu_p2p_sched import check_sessions
    from tests.test_gpu_wire import Datagrams, dev, now_table, poll_slots
    calls, cap = 240, 256
    rng = np.random.default_rng(77)
    rows = {side: rng.integers(0, 16, (calls, S, 2), dtype=np.uint8) for side in (0, 1)}
    delay = rng.integers(1, 5, (2, calls, S)).astype(np.int32)
    drop = rng.random((2, calls, S)) < 0.15
    black = np.arange(0, S, 5)
    short, long_ = black[0::2], black[1::2]
    drop[:, :, black] = False
    for s in black:
        b0 = 60 + s % 7
        drop[:, b0:(b0 + 20 if s in short else calls), s] = True
    ok = np.zeros((2, calls, 4, S), bool)
    for k in range(1, 5):
        ok[:, k:, k - 1] = (delay[:, :calls - k] == k) & ~drop[:, :calls - k]
    dv = torch.device("cuda")
    ok_d = torch.from_numpy(ok).to(dv)
    clock = now_table(calls)
    now = dev(clock)
    engines = {0: engine(cap=cap, feed=True, emit=True, time_sync=True, start=int(clock[0])),
               1: None}
    from ggrs_amd import P2PEngine
    B = P2PEngine(S, num_players=2, local_players=(1,), input_delay=0, max_prediction=MP, remote_latency=1,
                  input_capacity=cap)
    B.set_arrival_schedule(True)
    B.set_packet_feed(64)
    B.set_packet_emit(64)
    B.set_time_sync(60)
    B.set_endpoint_poll(M.CASE_TIMEOUT, M.CASE_NOTIFY, int(clock[0]))
    engines[1] = B
    stride = B.out_stride
    dstride = wire.max_datagram_bytes(2, stride)
    H = {side: History(calls, S, stride, dv) for side in (0, 1)}
    D = {side: Datagrams(calls, S, dstride, dv) for side in (0, 1)}
    u8 = lambda: torch.zeros((calls, S), dtype=torch.uint8, device=dv)  # noqa: E731
    rec = {side: {name: u8() for name in NAMES + ("kinds", "events")} for side in (0, 1)}
    adv = {side: torch.zeros((calls, S), dtype=torch.int32, device=dv) for side in (0, 1)}
    scratch = [torch.zeros((1, S), dtype=torch.int32, device=dv) for _ in range(2)]
    magic = {side: dev(np.arange(S).astype(np.uint16) + 0x4100 + 0x100 * side) for side in (0, 1)}
    rmask = {0: 0b10, 1: 0b01}
    for c in range(calls):
        polled = {}
        for side in (0, 1):
            dg, ln = poll_slots(c, ok_d[1 - side], D[1 - side])
            polled[side] = wire.unpack(dg, ln, now[c:c + 1], 2, rmask[side], stride, first_call=c)
        torch.cuda.synchronize()
        for side, eng in engines.items():
            u, r = polled[side], rec[side]
            eng.add_inputs(c, rows[side][c:c + 1])
            eng.receive_packets(c, u["start_frame"], u["packet_len"], u["packets"], u["events"])
            eng.poll_endpoints(c, 1, now[c:c + 1], u["kinds"], out=tuple(r[name][c:c + 1] for name in NAMES))
            eng.advance_frames(1)
            eng.emit_packets(c, 1, u["ack_in"], r["resend"][c:c + 1], out=H[side].row(c))
            eng.time_sync(c, 1, u["rtt_ms"], u["remote_advantage"], out=(adv[side][c:c + 1], *scratch))
            r["kinds"][c] = u["kinds"][0]
            r["events"][c] = u["events"][0]
        for eng in engines.values():
            eng.synchronize()
        for side in (0, 1):
            u, r = polled[side], rec[side]
            start, length, ack, packets = H[side].row(c)
            wire.pack(magic[side], now[c:c + 1], 2, stride, out=D[side].row(c), start_frame=start, packet_len=length,
                      ack_frame=ack, packets=packets, send_ack=r["send_ack"][c:c + 1],
                      send_report=r["send_report"][c:c + 1], local_advantage=adv[side][c:c + 1], kinds=u["kinds"],
                      ping=u["ping"])
    torch.cuda.synchronize()
    others = np.setdiff1d(np.arange(S), black)
    checked = sorted(set(black.tolist()) | set(others[::3].tolist()))
    seq = lambda col: [int(v) for v in col if v]  # noqa: E731
    arrive, events_after, pushed = {}, {}, {}
    for side, eng in engines.items():
        r = {name: t.cpu().numpy() for name, t in rec[side].items()}
        frames, skipped, errors = eng.sessions()
        assert (errors == 0).all(), (side, np.nonzero(errors)[0])
        status, arrive[side] = eng.packet_results(0, calls)
        assert (status >= 0).all() and not r["events"].any()
        m = M.run(S, M.CASE_TIMEOUT, M.CASE_NOTIFY, int(clock[0]), rmask[side], clock, r["kinds"], r["events"],
                  status=status)
        events_after[side] = m["events"]
        assert_outputs([r[name] for name in NAMES], m)
        assert_state(eng, m["model"])
        net = r["net_events"]
        assert not net[:, others].any()
        for s in short:
            assert seq(net[:, s]) == [M.NET_INTERRUPTED, M.NET_RESUMED], (side, s, seq(net[:, s]))
        for s in long_:
            assert seq(net[:, s]) == [M.NET_INTERRUPTED, M.NET_DISCONNECTED], (side, s, seq(net[:, s]))
        closed = eng.endpoint_state()[6]
        assert (closed[long_] > 100).all() and (np.delete(closed, long_) == -1).all()
        assert (closed == first_event_call(m["events"], rmask[side])).all()
        assert (eng.time_sync_state()[4] == closed).all() and (eng.emit_state()[3] == closed).all()
        assert r["resend"][:, black].any(axis=0).all() and r["send_report"].sum(axis=0).min() >= 5
        assert r["send_ack"][:, others].mean() > 0.5
        assert (skipped[black] > 0).all()           # the blackouts hit the prediction threshold,
        assert (frames[long_] > calls - 70).all()   # and the timed-out sessions went on alone
        # which call queued which frame: the session's control flow, which no input byte enters
        pushed[side] = np.full((calls, S), -1, np.int64)
        for s in checked:
            out = oracle.p2p_sched_run(rows[side][:, s], arrive[side][:, s], events_after[side][:, s], num_players=2,
                                       local_mask=eng.local_mask, input_delay=0, max_prediction=MP)
            assert out["rc"] == 0, (side, s)
            pushed[side][:, s] = E.pushes(out["advanced"], 0)
    # the final states against the oracle's run on the events rows the units produced
    for side, eng in engines.items():
        peer = 1 - side
        held = rows[side].copy()
        for s in checked:
            g = np.nonzero(pushed[peer][:, s] >= 0)[0]
            held[pushed[peer][g, s], s, peer] = rows[peer][g, s, peer]
            assert arrive[side][:, s].max() <= pushed[peer][:, s].max()  # nothing arrived that was not sent
        check_sessions(eng, held, arrive[side], events_after[side], checked, calls)
    assert (events_after[0][:, long_] != 0).any(axis=0).all() and (events_after[1][:, long_] != 0).any(axis=0).all()
