"""GPU parity of the two spectator poll units against tests/spectator_poll_model.py: the spectator
engine's own endpoint (ggrs_spectator_set_endpoint_poll / poll_endpoints / read_endpoint_state,
csrc/spectator_poll.hip) and the P2P engine's spectator endpoints (ggrs_p2p_set_spectator_poll /
poll_spectator_endpoints / read_spectator_endpoint_state, csrc/p2p_spec_poll.hip, and what spectator emit
reads of it) -- every output of every call and endpoint and the endpoints' state under three clocks and
six kinds of link, split over launches in several ways, from host arrays and device tensors; the packet
feed's dropped packets; the emit overflow in the live order; a P2P engine and two spectator engines
datagram to datagram with only the units' flags; misuse; and engines without the units.
S = 130 (two full waves and a two-lane block), 200 calls, timeout 640 ms, notify 160 ms, the clock
starting just below a multiple of 2^32, K in {1, 3} (a [n][K][S] stride mix-up shows at K = 3)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import spectator_poll_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

S, CALLS = M.CASE_S, M.CASE_CALLS
SPLITS = [((200,), False), ((1,), True), ((1, 3, 8, 13, 64), "both")]
HOST_FIELDS = ("last_recv", "last_input_recv", "last_report", "flags", "disconnected_call")
LINK_FIELDS = ("state", "last_recv", "last_input_recv", "last_report", "shutdown", "flags", "closed_call")


def pieces_of(pieces, calls):
    done, i = 0, 0
    while done < calls:
        n = min(pieces[i % len(pieces)], calls - done)
        yield done, n
        done, i = done + n, i + 1


def on_device(device, i):
    return device is True or (device == "both" and i % 2 == 0)


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_now(now):
    return torch.from_numpy(np.ascontiguousarray(now).view(np.int64).copy()).cuda()


def assert_outputs(got, m, names):
    for name, g in zip(names, got):
        w = m[name].reshape(g.shape)
        assert (g == w).all(), (name, np.argwhere(g != w)[:5])


def assert_fields(got, want, names):
    for name, g, w in zip(names, got, want):
        w = w.reshape(g.shape)
        assert g.dtype == w.dtype and (g == w).all(), (name, np.argwhere(g != w)[:5])


# ---- 1. the spectator engine's endpoint: parity per call and session

def spectator_engine(poll=True, feed=None, cap=256, timeout=M.CASE_TIMEOUT, notify=M.CASE_NOTIFY, start=M.CASE_START, S_=S):
    from ggrs_amd import SpectatorEngine
    e = SpectatorEngine(S_, num_players=2, input_capacity=cap)
    if feed:
        e.set_packet_feed(*feed)
    if poll:
        e.set_endpoint_poll(timeout, notify, start)
    return e


def poll_host(eng, c0, now, kinds, events, device):
    n = len(now)
    if device:
        out = tuple(torch.zeros((n, S), dtype=torch.uint8, device="cuda") for _ in range(3))
        eng.poll_endpoints(c0, n, dev_now(now), dev_u8(kinds), dev_u8(events), out=out)
        eng.synchronize()
        return [t.cpu().numpy() for t in out]
    return eng.poll_endpoints(c0, n, now, kinds, events)


@pytest.mark.parametrize("pieces,device", SPLITS)
@pytest.mark.parametrize("kind", M.CLOCKS)
def test_spectator_engine_outputs_and_state_match_the_model(kind, pieces, device):
    now, kinds, events = M.host_case(kind)
    m = M.host_run(kind)
    M.assert_host_case_is_not_vacuous(kind, m)
    eng = spectator_engine()
    got = [np.zeros((CALLS, S), np.uint8) for _ in range(3)]
    for i, (c0, n) in enumerate(pieces_of(pieces, CALLS)):
        sl = slice(c0, c0 + n)
        for g, o in zip(got, poll_host(eng, c0, now[sl], kinds[sl], events[sl], on_device(device, i))):
            g[sl] = o
    assert_outputs(got, m, M.HOST_NAMES)
    assert_fields(eng.endpoint_state(), m["model"].fields(), HOST_FIELDS)
    assert not (got[2] & M.NET_SHUTDOWN).any()
    # one call more, from the device, with a clock from the past: it is taken as the engine's last clock
    zeros = np.zeros((1, S), np.uint8)
    out = poll_host(eng, CALLS, now[:1], zeros, zeros, True)
    want = M.run_host(S, 0, 0, 0, now[:1], zeros, zeros, first_call=CALLS, model=m["model"])
    assert want["model"].clock == now[-1]
    assert_outputs(out, want, M.HOST_NAMES)
    assert_fields(eng.endpoint_state(), want["model"].fields(), HOST_FIELDS)


# ---- 2. the spectator engine with the packet feed: a damaged packet is no decoded Input

@functools.lru_cache(maxsize=None)
def damaged_feed():
    from tests import spectator_feed_model as F
    k = F.DAMAGED
    rows, host_upto, _, _ = F.damage_case()
    rng = np.random.default_rng(21)
    damage = {}
    for s in range(0, S, 2):  # a dozen damaged packets in every second session, where the sender sends
        rises = np.nonzero(host_upto[1:, s] > host_upto[:-1, s])[0] + 1
        for c in rng.choice(rises, 12, replace=False):
            damage[(int(c), s)] = ("truncate", "random")[int(c) % 2]
    return k, F.run_feed(rows, host_upto, k["mp"], k["W"], seed=9, damage=damage)


def test_damaged_packets_give_no_ack_and_do_not_reset_running_last_input_recv(oracle):
    k, feed = damaged_feed()
    assert (feed["stop_call"] < 0).all()
    # 250 ms a call: one call without a decoded Input is enough for the retry timer
    now = np.uint64(M.CASE_START) + np.arange(CALLS).astype(np.uint64) * np.uint64(250)
    kinds = np.where(feed["start"] >= 0, M.K_INPUT, 0).astype(np.uint8)
    events = np.zeros((CALLS, S), np.uint8)
    big = 1 << 20
    eng = spectator_engine(feed=(k["mp"], k["W"], feed["stride"]), cap=k["cap"], timeout=big, notify=big)
    got = [np.zeros((CALLS, S), np.uint8) for _ in range(3)]
    for c0, n in pieces_of((1, 3, 8, 13, 64), CALLS):
        sl = slice(c0, c0 + n)
        eng.receive_packets(c0, feed["start"][sl], feed["length"][sl], feed["packets"][sl])
        for g, o in zip(got, eng.poll_endpoints(c0, n, now[sl], kinds[sl])):
            g[sl] = o
        eng.advance_frames(n)
    status, _ = eng.read_packet_results(0, CALLS)
    assert (status == feed["status"]).all()
    dropped = (status < 0) & (kinds != 0)
    assert dropped.sum() > S
    m = M.run_host(S, big, big, M.CASE_START, now, kinds, events, status=status)
    assert_outputs(got, m, M.HOST_NAMES)
    assert_fields(eng.endpoint_state(), m["model"].fields(), HOST_FIELDS)
    assert not got[0][dropped].any() and got[0][(status >= 0) & (kinds != 0)].all()
    # a model blind to the status differs in the acks (and in running_last_input_recv: the next test)
    blind = M.run_host(S, big, big, M.CASE_START, now, kinds, events)
    assert (blind["send_ack"] != m["send_ack"]).sum() == dropped.sum()


def test_running_last_input_recv_tells_a_dropped_packet_from_a_decoded_one(oracle):
    """100 ms a call, so the retry timer does not hide it: at the call of a damaged packet the field keeps
    its old value on the device, where a model blind to the feed's status would have reset it."""
    k, feed = damaged_feed()
    n = 60
    last_drop = None
    for c in range(n - 1, 0, -1):
        hit = (feed["status"][c] < 0) & (feed["start"][c] >= 0)
        if hit.any():
            last_drop, n = hit, c + 1
            break
    assert last_drop is not None
    now = np.uint64(M.CASE_START) + np.arange(n).astype(np.uint64) * np.uint64(100)
    kinds = np.where(feed["start"][:n] >= 0, M.K_INPUT, 0).astype(np.uint8)
    events = np.zeros((n, S), np.uint8)
    big = 1 << 20
    eng = spectator_engine(feed=(k["mp"], k["W"], feed["stride"]), cap=k["cap"], timeout=big, notify=big)
    eng.receive_packets(0, feed["start"][:n], feed["length"][:n], feed["packets"][:n])
    got = eng.poll_endpoints(0, n, now, kinds)
    m = M.run_host(S, big, big, M.CASE_START, now, kinds, events, status=feed["status"][:n])
    blind = M.run_host(S, big, big, M.CASE_START, now, kinds, events)
    assert_outputs(got, m, M.HOST_NAMES)
    assert_fields(eng.endpoint_state(), m["model"].fields(), HOST_FIELDS)
    assert (m["model"].last_input_recv[last_drop] != blind["model"].last_input_recv[last_drop]).any()


# ---- 3. the P2P engine's spectator endpoints: parity, and what spectator emit reads

MP, W = 8, 64


def p2p_engine(K, poll=True, cap=CALLS, max_pending=W, start=M.CASE_START, timeout=M.CASE_TIMEOUT, notify=M.CASE_NOTIFY):
    from tests.test_gpu_spectator_emit import engine
    e = engine(2, (0,), 0, MP, K, cap=cap, max_pending=max_pending)
    if poll:
        e.set_spectator_poll(timeout, notify, start)
    return e


@functools.lru_cache(maxsize=None)
def steady_run(calls, K, silent=()):
    """Rows, a lag-one arrival table and acks that follow the confirmed frame (endpoints in `silent`
    never ack); the sessions' control flow is the same in every session, so the oracle runs one."""
    from tests import spectator_emit_model as E
    from tests.test_gpu_spectator_emit import steady
    rows, arrive, events = steady(2, calls)
    pushed, stop = E.pushed_table(rows[:, :1], arrive[:, :1], events[:, :1], 2, 0b01, 0, MP)
    assert stop[0] < 0
    pushed = np.repeat(pushed, S, axis=1)
    confirmed = E.confirmed_table(arrive[:, :1], events[:, :1], pushed[:, :1], 0b01, 2)
    ack = np.repeat(np.repeat(np.maximum(confirmed - 1, -1), S, axis=1)[:, None, :], K, axis=1).astype(np.int32)
    for k, every in silent:
        ack[:, k, ::every] = -1
    return rows, arrive, events, pushed, ack


def poll_links(eng, K, c0, now, kinds, close_in, device):
    n = len(now)
    kinds, close_in = kinds.reshape(n, K, S), close_in.reshape(n, K, S)
    if device:
        out = tuple(torch.zeros((n, K, S), dtype=torch.uint8, device="cuda") for _ in range(3))
        eng.poll_spectator_endpoints(c0, n, dev_now(now), dev_u8(kinds), dev_u8(close_in), out=out)
        eng.synchronize()
        return [t.cpu().numpy() for t in out]
    return eng.poll_spectator_endpoints(c0, n, now, kinds, close_in)


def assert_emit_follows_the_poll(A, B, a_out, b_out, closed):
    """A's endpoints closed by the poll at closed[k][s] (-1: never): GGRS_EMIT_CLOSED there at the poll's
    call, nothing emitted from that call on; everything else byte-identical to B, an engine without
    the unit given the same acks and resend flags."""
    from ggrs_amd._lib import GGRS_EMIT_CLOSED
    from tests.test_gpu_p2p_packets import assert_same
    nxt_a, la_a, pend_a, status_a, closed_a = A.read_spectator_emit_state()
    nxt_b, la_b, pend_b, status_b, closed_b = B.read_spectator_emit_state()
    assert (status_a == np.where(closed >= 0, GGRS_EMIT_CLOSED, 0)).all() and (closed_a == closed).all()
    assert (status_b == 0).all() and (nxt_a == nxt_b).all()
    opened = closed < 0
    assert (la_a[opened] == la_b[opened]).all() and (pend_a[opened] == pend_b[opened]).all()
    assert_same(A, B)
    calls = a_out[0].shape[0]
    live = opened[None] | (np.arange(calls)[:, None, None] < closed[None])  # [calls][K][S]
    assert (a_out[0][live] == b_out[0][live]).all() and (a_out[1][live] == b_out[1][live]).all()
    assert (a_out[0][~live] == -1).all() and (a_out[1][~live] == 0).all()
    assert (a_out[2] == b_out[2]).all()  # the notes are the session's
    body = np.arange(a_out[3].shape[3])[None, None, None, :] < a_out[1][..., None]
    assert (np.where(body, a_out[3], 0)[live] == np.where(body, b_out[3], 0)[live]).all()
    assert (b_out[0][live] >= 0).sum() > live.sum() // 2


@pytest.mark.parametrize("pieces,device", SPLITS)
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("kind", M.CLOCKS)
def test_spectator_endpoints_match_the_model_and_emit_stops_where_the_poll_closed(oracle, kind, K, pieces, device):
    now, kinds, close_in, _ = M.link_case(kind, K)
    m = M.link_run(kind, K)
    M.assert_link_case_is_not_vacuous(kind, m)
    rows, arrive, events, _, ack = steady_run(CALLS, K)
    A, B = p2p_engine(K), p2p_engine(K, poll=False)
    for e in (A, B):
        e.add_inputs(0, rows)
        e.add_arrivals(0, arrive, events)
    got = [np.zeros((CALLS, K, S), np.uint8) for _ in range(3)]
    a_out, b_out = [], []
    for i, (c0, n) in enumerate(pieces_of(pieces, CALLS)):
        sl = slice(c0, c0 + n)
        for g, o in zip(got, poll_links(A, K, c0, now[sl], kinds[sl], close_in[sl], on_device(device, i))):
            g[sl] = o
        A.advance_frames(n)
        B.advance_frames(n)
        a_out.append(A.emit_spectator_packets(c0, n, ack[sl], got[0][sl]))
        b_out.append(B.emit_spectator_packets(c0, n, ack[sl], got[0][sl]))
    assert_outputs(got, m, M.LINK_NAMES)
    assert_fields(A.spectator_endpoint_state(), m["model"].fields(), LINK_FIELDS)
    closed = m["model"].closed_call.reshape(K, S)
    assert (closed >= 0).sum() >= K * S // 4
    cat = lambda outs: tuple(np.concatenate([o[j] for o in outs]) for j in range(4))  # noqa: E731
    assert_emit_follows_the_poll(A, B, cat(a_out), cat(b_out), closed)
    # one call more, from the device, with a clock from the past: it is taken as the engine's last clock
    zeros = np.zeros((1, K * S), np.uint8)
    out = poll_links(A, K, CALLS, now[:1], zeros, zeros, True)
    want = M.run_links(K * S, 0, 0, 0, now[:1], zeros, zeros, first_call=CALLS, model=m["model"])
    assert want["model"].clock == now[-1]
    assert_outputs(out, want, M.LINK_NAMES)
    assert_fields(A.spectator_endpoint_state(), want["model"].fields(), LINK_FIELDS)


# ---- 4. the emit overflow, in the live order

def test_an_overflowed_endpoint_is_closed_by_the_next_poll_and_shuts_down_5000_ms_later(oracle):
    """max_pending_inputs 4; endpoint 1 of every fifth session never acks: the emit closes it at the
    model's call c (GGRS_EMIT_DISCONNECTED), the poll of c + 1 raises GGRS_NET_DISCONNECTED and closes
    with closed_call = c + 1, Shutdown comes at the first clock more than 5,000 ms later.  Every call:
    poll, run, emit.  100 ms a call, an InputAck on every link at every call: nothing times out."""
    from ggrs_amd._lib import GGRS_EMIT_DISCONNECTED
    from tests import packet_feed_model as F
    from tests import spectator_emit_model as E
    K, calls, maxpend = 2, 64, 4
    rows, arrive, events, pushed, ack = steady_run(calls, K, silent=((1, 5),))
    em = E.run(rows, arrive, events, pushed, 0b01, K, maxpend, F.max_packet_bytes(2, maxpend), ack, None,
               np.full(S, -1, np.int32))
    over_call = np.where(em["status"] == E.EMIT_DISCONNECTED, em["closed_call"], -1)  # [K][S]
    hit = np.zeros((K, S), bool)
    hit[1, ::5] = True
    assert (over_call[hit] >= 0).all() and (over_call[~hit] == -1).all()
    c_e = int(over_call[1, 0])
    assert (over_call[hit] == c_e).all() and 0 < c_e < 10
    now = np.uint64(M.CASE_START) + np.arange(calls).astype(np.uint64) * np.uint64(100)
    kinds = np.full((calls, K * S), M.P.K_INPUT_ACK, np.uint8)
    close_in = np.zeros((calls, K * S), np.uint8)
    over = (np.arange(calls)[:, None] > over_call.reshape(-1)[None]) & (over_call.reshape(-1)[None] >= 0)
    m = M.run_links(K * S, M.CASE_TIMEOUT, M.CASE_NOTIFY, M.CASE_START, now, kinds, close_in, over)
    net = m["net_events"].reshape(calls, K, S)
    assert (net[c_e + 1][hit] == M.NET_DISCONNECTED).all() and (m["model"].closed_call.reshape(K, S)[hit] == c_e + 1).all()
    down = c_e + 1 + 51  # 100 ms a call: 5,100 ms is the first clock above shutdown_timeout
    assert (net[down][hit] == M.NET_SHUTDOWN).all() and net[:, hit].astype(bool).sum() == 2 * hit.sum()
    assert not net[:, ~hit].any()
    eng = p2p_engine(K, cap=calls, max_pending=maxpend)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    got = [np.zeros((calls, K, S), np.uint8) for _ in range(3)]
    for c in range(calls):
        sl = slice(c, c + 1)
        for g, o in zip(got, poll_links(eng, K, c, now[sl], kinds[sl], close_in[sl], c % 2 == 0)):
            g[sl] = o
        eng.advance_frames(1)
        eng.emit_spectator_packets(c, 1, ack[sl], got[0][sl])
    assert_outputs(got, m, M.LINK_NAMES)
    assert_fields(eng.spectator_endpoint_state(), m["model"].fields(), LINK_FIELDS)
    _, _, _, status, closed = eng.read_spectator_emit_state()
    assert (status[hit] == GGRS_EMIT_DISCONNECTED).all() and (closed[hit] == c_e).all()
    assert (status[~hit] == 0).all() and (closed[~hit] == -1).all()
    assert (eng.sessions()[2] == 0).all()


# ---- 6. misuse

def state_error(fn, *a):
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    with pytest.raises(GgrsError) as e:
        fn(*a)
    assert e.value.code == GGRS_E_STATE, e.value


def test_spectator_engine_misuse(oracle):
    from ggrs_amd._lib import InvalidRequest
    from tests import spectator_feed_model as F
    now = M.P.case_clock("const8", 8)
    zeros = np.zeros((8, S), np.uint8)
    plain = spectator_engine(poll=False)
    state_error(plain.poll_endpoints, 0, 1, now[:1])                      # unconfigured
    state_error(plain.endpoint_state)
    plain.add_inputs(0, np.zeros((4, S, 2), np.uint8))
    plain.add_arrivals(0, np.zeros((2, S), np.int32))
    state_error(plain.set_endpoint_poll, 640, 160, 0)                     # after the first arrival
    with pytest.raises(InvalidRequest):
        spectator_engine(timeout=100, notify=101)                         # the reference's subtraction panics
    spectator_engine(timeout=100, notify=100)
    eng = spectator_engine()
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(1, 1, now[1:2])                                # out of order
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(0, 2, now[:2][::-1].copy())                    # a host clock that decreases
    eng.poll_endpoints(0, 2, now[:2], zeros[:2])
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(1, 1, now[1:2])                                # repeated
    with pytest.raises(InvalidRequest):
        eng.poll_endpoints(2, 1, now[:1])                                 # below the last host clock
    eng.poll_endpoints(2, 4, now[2:6], zeros[:4])
    m = M.run_host(S, M.CASE_TIMEOUT, M.CASE_NOTIFY, M.CASE_START, now[:6], zeros[:6], zeros[:6])
    assert_fields(eng.endpoint_state(), m["model"].fields(), HOST_FIELDS)
    # with the packet feed: a call is polled after its packets, and while its status row is held
    k = F.DAMAGED
    _, feed = damaged_feed()
    cap = 72
    fed = spectator_engine(feed=(k["mp"], k["W"], feed["stride"]), cap=cap)
    clock = M.P.case_clock("const8", CALLS)
    with pytest.raises(InvalidRequest):
        fed.poll_endpoints(0, 1, clock[:1])                               # call 0's packets were not received
    fed.receive_packets(0, feed["start"][:40], feed["length"][:40], feed["packets"][:40])
    with pytest.raises(InvalidRequest):
        fed.poll_endpoints(0, 41, clock[:41])                             # call 40's were not
    fed.poll_endpoints(0, 2, clock[:2])
    fed.advance_frames(40)
    fed.receive_packets(40, feed["start"][40:100], feed["length"][40:100], feed["packets"][40:100])
    with pytest.raises(InvalidRequest):
        fed.poll_endpoints(2, 1, clock[2:3])                              # call 2's status row is gone (100 - 72 = 28)
    m = M.run_host(S, M.CASE_TIMEOUT, M.CASE_NOTIFY, M.CASE_START, clock[:2], np.zeros((2, S), np.uint8),
                   np.zeros((2, S), np.uint8), status=feed["status"][:2])
    assert_fields(fed.endpoint_state(), m["model"].fields(), HOST_FIELDS)


def test_p2p_side_misuse(oracle):
    from ggrs_amd import P2PEngine
    from ggrs_amd._lib import InvalidRequest
    K = 2
    rows, arrive, events, _, ack = steady_run(8, K)
    now = M.P.case_clock("const8", 8)
    zeros = np.zeros((8, K, S), np.uint8)
    plain = p2p_engine(K, poll=False, cap=64)
    plain.add_inputs(0, rows)
    plain.add_arrivals(0, arrive, events)
    state_error(plain.poll_spectator_endpoints, 0, 1, now[:1])            # unconfigured
    state_error(plain.spectator_endpoint_state)
    plain.advance_frames(1)
    state_error(plain.set_spectator_poll, 640, 160, 0)                    # after the first call
    plain.emit_spectator_packets(0, 1)                                    # (no unit: nothing to poll first)
    no_emit = P2PEngine(S, num_players=2, local_players=(0,), max_prediction=MP, remote_latency=1, input_capacity=64)
    no_emit.set_arrival_schedule(True)
    state_error(no_emit.set_spectator_poll, 640, 160, 0)                  # without spectator emit
    fixed = P2PEngine(S, num_players=2, local_players=(0,), max_prediction=MP, remote_latency=2, input_capacity=64)
    state_error(fixed.set_spectator_poll, 640, 160, 0)                    # a fixed-latency engine
    with pytest.raises(InvalidRequest):
        p2p_engine(K, cap=64, timeout=100, notify=101)
    p2p_engine(K, cap=64, timeout=100, notify=100)
    eng = p2p_engine(K, cap=64)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive, events)
    with pytest.raises(InvalidRequest):
        eng.poll_spectator_endpoints(1, 1, now[1:2])                      # out of order
    with pytest.raises(InvalidRequest):
        eng.poll_spectator_endpoints(0, 2, now[:2][::-1].copy())          # a host clock that decreases
    eng.advance_frames(4)                                                 # (no ordering against the calls)
    state_error(eng.emit_spectator_packets, 0, 1)                         # call 0 was not polled
    eng.poll_spectator_endpoints(0, 2, now[:2], zeros[:2])
    with pytest.raises(InvalidRequest):
        eng.poll_spectator_endpoints(1, 1, now[1:2])                      # repeated
    with pytest.raises(InvalidRequest):
        eng.poll_spectator_endpoints(2, 1, now[:1])                       # below the last host clock
    state_error(eng.emit_spectator_packets, 0, 3)                         # call 2 was not polled
    eng.emit_spectator_packets(0, 2)
    eng.poll_spectator_endpoints(2, 4, now[2:6], zeros[:4])
    eng.emit_spectator_packets(2, 2)
    m = M.run_links(K * S, M.CASE_TIMEOUT, M.CASE_NOTIFY, M.CASE_START, now[:6], zeros[:6].reshape(6, -1),
                    zeros[:6].reshape(6, -1))
    assert_fields(eng.spectator_endpoint_state(), m["model"].fields(), LINK_FIELDS)
    assert (eng.read_spectator_emit_state()[3] == 0).all()


# ---- 7. engines without the units are unchanged; links that never go silent change nothing

def test_links_that_never_go_silent_raise_nothing_and_change_no_packet(oracle):
    K = 3
    now = M.P.case_clock("jitter")
    kinds = np.full((CALLS, K * S), M.P.K_INPUT_ACK, np.uint8)
    close_in = np.zeros((CALLS, K * S), np.uint8)
    rows, arrive, events, _, ack = steady_run(CALLS, K)
    A, B = p2p_engine(K), p2p_engine(K, poll=False)
    for e in (A, B):
        e.add_inputs(0, rows)
        e.add_arrivals(0, arrive, events)
    a_out, b_out, resend = [], [], np.zeros((CALLS, K, S), np.uint8)
    for i, (c0, n) in enumerate(pieces_of((13, 8), CALLS)):
        sl = slice(c0, c0 + n)
        r, report, net = poll_links(A, K, c0, now[sl], kinds[sl], close_in[sl], i % 2 == 0)
        assert not net.any()
        resend[sl] = r
        A.advance_frames(n)
        B.advance_frames(n)
        a_out.append(A.emit_spectator_packets(c0, n, ack[sl], r))
        b_out.append(B.emit_spectator_packets(c0, n, ack[sl], r))
    assert resend.sum() > K * S  # (the 260, 700 and 5,200 ms steps of the clock: the retry, and nothing else)
    cat = lambda o: tuple(np.concatenate([x[j] for x in o]) for j in range(4))  # noqa: E731
    assert_emit_follows_the_poll(A, B, cat(a_out), cat(b_out), np.full((K, S), -1, np.int32))
    assert (A.spectator_endpoint_state()[6] == -1).all()


def test_a_spectator_engine_with_the_unit_advances_as_one_without(oracle):
    from tests.test_gpu_spectator_packets import assert_equal, reads
    k, feed = damaged_feed()
    now, kinds, events = M.host_case("jitter")
    engines = []
    for poll in (True, False):
        from ggrs_amd import SpectatorEngine
        e = SpectatorEngine(S, num_players=2, max_frames_behind=k["mfb"], catchup_speed=k["speed"], input_capacity=k["cap"],
                            trace_capacity=CALLS)
        e.set_packet_feed(k["mp"], k["W"], feed["stride"])
        if poll:
            e.set_endpoint_poll(M.CASE_TIMEOUT, M.CASE_NOTIFY, M.CASE_START)
        for c0, n in pieces_of((13, 8), CALLS):
            sl = slice(c0, c0 + n)
            e.receive_packets(c0, feed["start"][sl], feed["length"][sl], feed["packets"][sl])
            if poll:
                e.poll_endpoints(c0, n, now[sl], kinds[sl], events[sl])
            e.advance_frames(n)
        engines.append(reads(e, CALLS))
    assert_equal(engines[0], engines[1], "with the unit against without")
    assert (engines[0]["advanced"] > 0).sum() > S * CALLS // 4


# ---- 5. closed loop: a P2P engine and two spectator engines, datagram to datagram, no host-made flag

def assert_lossy_links_only_pause(lossy, interrupted, resumed):
    """The links that only lose 15 % of their datagrams: an ack leaves only at a call that decoded an
    Input, so a poll sees no message with a probability of up to about 0.35, and the 11 silent polls in a
    row that notify (160 ms at 16 ms a call) needs have a chance of about 1e-5 per poll -- 0.4 such pauses
    expected over the 255 lossy links' 160 polls, three or more with a chance below 1 %.  So a lossy link
    may pause (INTERRUPTED, then RESUMED when the next datagram arrives) but never more, and at most two
    of them do.  That each event sits at the right call is the replay's check, not this one's."""
    assert all(events in ([interrupted, resumed], [interrupted, resumed] * 2) for _, _, events in lossy), lossy
    assert len(lossy) <= 2, lossy


def test_a_p2p_engine_and_two_spectator_engines_play_with_the_units_flags(oracle):
    """One scheduled P2P engine with two spectators per session, followed by two SpectatorEngines; both
    directions travel as datagrams through ggrs_amd.wire in device memory.  resend, send_ack and
    send_report are taken only from the units.  16 ms a call (notify is 10 calls, the timeout 40), 160
    calls.  Every fifth session's link to spectator 0 blacks out both ways, alternately for 20 calls and
    for good from about call 50; the other links lose 15 % of their datagrams.  Each side's recorded
    unit inputs replayed through the model give its recorded outputs.  A short blackout raises
    INTERRUPTED then RESUMED on both ends and nothing else (a merely lossy link at most pauses:
    assert_lossy_links_only_pause); a long one INTERRUPTED then DISCONNECTED on
    both ends, the host's endpoint is GGRS_EMIT_CLOSED at the poll's call, that spectator stops
    advancing, the session plays on, and its other spectator follows it: every spectator that still
    has its link equals, bit for bit, a table-fed spectator engine given the session's confirmed inputs
    and the frames the link delivered.  No session has an error."""
    from ggrs_amd import SpectatorEngine, wire
    from ggrs_amd._lib import GGRS_EMIT_CLOSED, GGRS_PACKET_NO_REFERENCE
    from tests.test_gpu_spectator_emit import steady
    from tests.test_gpu_wire import Datagrams, dev, now_table, poll_slots
    K, calls, cap = 2, 160, 256
    dv = torch.device("cuda")
    rows, arrive, events = steady(2, calls)
    rng = np.random.default_rng(91)
    delay = rng.integers(1, 5, (2, K, calls, S)).astype(np.int32)   # [direction][link]: down (to the spectator), up
    drop = rng.random((2, K, calls, S)) < 0.15
    black = np.arange(0, S, 5)
    short, long_ = black[0::2], black[1::2]
    drop[:, 0][:, :, black] = False
    for s in black:
        b0 = 50 + s % 7
        drop[:, 0, b0:(b0 + 20 if s in short else calls), s] = True
    ok = np.zeros((2, K, calls, 4, S), bool)
    for k in range(1, 5):
        ok[:, :, k:, k - 1] = (delay[:, :, :calls - k] == k) & ~drop[:, :, :calls - k]
    ok_d = torch.from_numpy(ok).to(dv)
    clock = now_table(calls)
    now = dev(clock)
    host = p2p_engine(K, cap=cap, start=int(clock[0]))
    stride = host.spectator_stride
    spectators = []
    for j in range(K):
        sp = SpectatorEngine(S, num_players=2, input_capacity=cap, trace_capacity=calls)
        sp.set_packet_feed(MP, W)
        sp.set_endpoint_poll(M.CASE_TIMEOUT, M.CASE_NOTIFY, int(clock[0]))
        assert sp.packet_stride == stride
        spectators.append(sp)
    dstride = wire.max_datagram_bytes(2, stride)
    down = [Datagrams(calls, S, dstride, dv) for _ in range(K)]  # host -> spectator j
    up = [Datagrams(calls, S, dstride, dv) for _ in range(K)]    # spectator j -> host
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dv)  # noqa: E731
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dv)  # noqa: E731
    h_rec = {name: u8(calls, K, S) for name in M.LINK_NAMES + ("kinds",)}
    s_rec = [{name: u8(calls, S) for name in M.HOST_NAMES + ("kinds", "events")} for _ in range(K)]
    H = (torch.full((calls, K, S), -1, dtype=torch.int32, device=dv), i32(calls, K, S), i32(calls, S),
         u8(calls, K, S, stride))
    magic = [dev(np.arange(S).astype(np.uint16) + 0x5100 + 0x100 * j) for j in range(K + 1)]
    zero_adv = i32(1, S)
    for c in range(calls):
        t = now[c:c + 1]
        from_spec = [wire.unpack(*poll_slots(c, ok_d[1, j], up[j]), t, 2, 0b10, stride, first_call=c,
                                 want=("ack_in", "kinds", "ping")) for j in range(K)]
        from_host = [wire.unpack(*poll_slots(c, ok_d[0, j], down[j]), t, 2, 0b01, stride, first_call=c,
                                 want=("start_frame", "packet_len", "packets", "notes", "events", "kinds", "ping"))
                     for j in range(K)]
        torch.cuda.synchronize()
        # the host: poll its spectator endpoints, run the call, emit to the spectators
        h_rec["kinds"][c] = torch.stack([u["kinds"][0] for u in from_spec])
        ack_in = torch.stack([u["ack_in"][0] for u in from_spec])[None].contiguous()
        host.add_inputs(c, rows[c:c + 1])
        host.add_arrivals(c, arrive[c:c + 1], events[c:c + 1])
        host.poll_spectator_endpoints(c, 1, t, h_rec["kinds"][c:c + 1], None,
                                      out=tuple(h_rec[name][c:c + 1] for name in M.LINK_NAMES))
        host.advance_frames(1)
        host.emit_spectator_packets(c, 1, ack_in, h_rec["resend"][c:c + 1], out=tuple(x[c:c + 1] for x in H))
        host.synchronize()
        for j in range(K):
            wire.pack(magic[K], t, 2, stride, out=down[j].row(c), start_frame=H[0][c:c + 1, j].contiguous(),
                      packet_len=H[1][c:c + 1, j].contiguous(), packets=H[3][c:c + 1, j].contiguous(),
                      send_report=h_rec["send_report"][c:c + 1, j].contiguous(), local_advantage=zero_adv,
                      kinds=from_spec[j]["kinds"], ping=from_spec[j]["ping"])
        # the spectators: receive, poll the host endpoint, run the call, acknowledge
        for j, sp in enumerate(spectators):
            u, r = from_host[j], s_rec[j]
            r["kinds"][c], r["events"][c] = u["kinds"][0], u["events"][0]
            sp.receive_packets(c, u["start_frame"], u["packet_len"], u["packets"], u["notes"])
            sp.poll_endpoints(c, 1, t, u["kinds"], u["events"], out=tuple(r[name][c:c + 1] for name in M.HOST_NAMES))
            sp.advance_frames(1)
            ack = torch.from_numpy(sp.read_packet_results(c, 1)[1]).to(dv)
            wire.pack(magic[j], t, 2, stride, out=up[j].row(c), ack_frame=ack, send_ack=r["send_ack"][c:c + 1],
                      send_report=r["send_report"][c:c + 1], local_advantage=zero_adv, kinds=u["kinds"], ping=u["ping"])
        torch.cuda.synchronize()
    seq = lambda col: [int(v) for v in col if v]  # noqa: E731
    I_, R_, D_ = M.NET_INTERRUPTED, M.NET_RESUMED, M.NET_DISCONNECTED
    others = np.setdiff1d(np.arange(S), black)
    # the host's side: the recorded inputs through the model give the recorded outputs
    hr = {name: x.cpu().numpy() for name, x in h_rec.items()}
    assert not hr["kinds"].astype(np.uint8).__and__(M.K_INPUT).any()  # a spectator sends no Input
    m = M.run_links(K * S, M.CASE_TIMEOUT, M.CASE_NOTIFY, int(clock[0]), clock, hr["kinds"].reshape(calls, -1),
                    np.zeros((calls, K * S), np.uint8))
    assert_outputs([hr[name] for name in M.LINK_NAMES], m, M.LINK_NAMES)
    assert_fields(host.spectator_endpoint_state(), m["model"].fields(), LINK_FIELDS)
    closed = host.spectator_endpoint_state()[6]
    assert (closed[0][long_] > 60).all() and (np.delete(closed[0], long_) == -1).all() and (closed[1] == -1).all()
    _, _, _, emit_status, emit_closed = host.read_spectator_emit_state()
    assert (emit_closed == closed).all() and (emit_status == np.where(closed >= 0, GGRS_EMIT_CLOSED, 0)).all()
    net = hr["net_events"]
    lossy = [(j, int(s), seq(net[:, j, s])) for j in range(K) for s in (others if j == 0 else range(S)) if net[:, j, s].any()]
    assert_lossy_links_only_pause(lossy, I_, R_)
    for s in short:
        assert seq(net[:, 0, s]) == [I_, R_], ("host", s, seq(net[:, 0, s]))
    for s in long_:
        assert seq(net[:, 0, s]) == [I_, D_], ("host", s, seq(net[:, 0, s]))
    assert hr["resend"].any(axis=0).all() and hr["send_report"].sum(axis=0).min() >= 5
    frames, _, errors = host.sessions()
    assert (errors == 0).all() and (frames == frames[0]).all() and frames[0] >= calls - 2  # the sessions play on
    # the spectators' side
    for j, sp in enumerate(spectators):
        r = {name: x.cpu().numpy() for name, x in s_rec[j].items()}
        status, recv = sp.read_packet_results(0, calls)
        # (a packet that arrives after a newer one carried the spectator more than 2 max_prediction frames
        # past its reference is refused -- after a blackout's burst, mostly -- and no other way)
        assert (status[status < 0] == GGRS_PACKET_NO_REFERENCE).all() and (status < 0).mean() < 0.01, np.unique(status)
        assert not r["events"].any()
        m = M.run_host(S, M.CASE_TIMEOUT, M.CASE_NOTIFY, int(clock[0]), clock, r["kinds"], r["events"], status=status)
        assert_outputs([r[name] for name in M.HOST_NAMES], m, M.HOST_NAMES)
        assert_fields(sp.endpoint_state(), m["model"].fields(), HOST_FIELDS)
        net = r["net_events"]
        quiet = others if j == 0 else np.arange(S)
        assert_lossy_links_only_pause([(j, int(s), seq(net[:, s])) for s in quiet if net[:, s].any()], I_, R_)
        assert r["send_ack"][:, quiet].mean() > 0.5 and r["send_report"].sum(axis=0).min() >= 5
        cur, last, waited, err = sp.sessions()
        assert (err == 0).all()
        if j == 0:
            for s in short:
                assert seq(net[:, s]) == [I_, R_], ("spectator", s, seq(net[:, s]))
            for s in long_:
                assert seq(net[:, s]) == [I_, D_], ("spectator", s, seq(net[:, s]))
            assert (sp.endpoint_state()[4][long_] > 60).all()
            assert (cur[long_] < 60).all() and (cur[np.delete(np.arange(S), long_)] > calls - 30).all()  # it waits
        else:
            assert (cur > calls - 30).all()
        # the confirmed inputs of frame f are rows[f] (no input delay, no prediction threshold, nobody
        # disconnects): a table-fed engine given them and the frames this link delivered
        ref = SpectatorEngine(S, num_players=2, input_capacity=cap, trace_capacity=calls)
        ref.add_inputs(0, rows)
        ref.add_arrivals(0, recv)
        ref.advance_frames(calls)
        for a, b in zip(sp.trace(0, calls), ref.trace(0, calls)):
            assert (a == b).all(), j
        want = ref.sessions()
        assert (cur == want[0]).all() and (last == want[1]).all() and (want[3] == 0).all()
        assert (sp.states() == ref.states()).all()
