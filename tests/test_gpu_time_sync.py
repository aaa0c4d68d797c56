"""GPU parity of the P2P engine's time sync (ggrs_p2p_set_time_sync / time_sync / time_sync_state,
csrc/p2p_time_sync.hip) against tests/time_sync_model.py: every call's local_advantage, frames_ahead
and skip_frames and the final state under arrival schedules with stalls and disconnects, in one piece
and split over launches, with host arrays and in device memory, both window forms, the packet feed,
two engines handing each other their advantage rows on the device, misuse -- and an engine that does
not configure time sync against one that does.

The model's current_frame comes from the oracle's per-call `advanced`, the kernel's from the word the
scheduled kernels store (the local players' last queued frame - input_delay): local_advantage =
last_recv + ping frames - current_frame, so every call's parity checks that claim on the device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import packet_feed_model as F  # noqa: E402
from tests import time_sync_model as T  # noqa: E402
from tests.test_gpu_p2p_emit import CASES, PIECES  # noqa: E402
from tests.test_gpu_p2p_sched import check_sessions, schedules, set_form  # noqa: E402
from tests.test_time_sync_model import (CALLS, FPS, S, exactly_61_apart, oracle_tables, parity_case,  # noqa: E402
                                        proves_something)

pytestmark = pytest.mark.gpu

NAMES = ("local_advantage", "frames_ahead", "skip_frames")


def engine(P, local, delay, mp, cap=CALLS, S_=S, feed=False, time_sync=True):
    from ggrs_amd import P2PEngine
    e = P2PEngine(S_, num_players=P, local_players=local, input_delay=delay, max_prediction=mp, remote_latency=1,
                  input_capacity=cap)
    e.set_arrival_schedule(True)
    if feed:
        e.set_packet_feed(64)
    if time_sync:
        e.set_time_sync(FPS)
    return e


def assert_outputs(got, m, c0=0):
    """time_sync's outputs of calls c0 .. against the model's, every call and session."""
    for name, g in zip(NAMES, got):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        want = m[name][c0:c0 + g.shape[0]]
        assert (g == want).all(), (name, np.argwhere(g != want)[:5])


def assert_state(eng, m):
    for i, (g, want) in enumerate(zip(eng.time_sync_state(), m["state"])):
        assert (g == want).all(), (i, np.argwhere(g != want)[:5])


@pytest.mark.parametrize("form,P,local,delay,mp", CASES)
def test_time_sync_matches_the_model(oracle, monkeypatch, form, P, local, delay, mp):
    """The whole run in one piece with host arrays; on a second engine in the launches' pieces; on a
    third in pieces with every array in device memory."""
    set_form(monkeypatch, form)
    rows, arrive, events, rtt, radv, m = parity_case(P, local, delay, mp)
    if mp > 0:
        proves_something(m)
        assert exactly_61_apart(m, m["cur"])
    else:  # lockstep mode: the session trails its peer, nothing to recommend
        assert (m["frames_ahead"] < 0).sum() > S * CALLS // 2 and (m["state"][4] >= 0).sum() > 5
    one, many, dev = (engine(P, local, delay, mp) for _ in range(3))
    for e in (one, many, dev):
        e.add_inputs(0, rows)
        e.add_arrivals(0, arrive, events)
    d = torch.device("cuda")
    rtt_d, radv_d = torch.from_numpy(rtt).to(d), torch.from_numpy(radv).to(d)
    outs_d = tuple(torch.full((CALLS, S), 77, dtype=torch.int32, device=d) for _ in range(3))
    pieces, done = [], 0
    for n in PIECES:
        for e in (one, many, dev):
            e.advance_frames(n)
        pieces.append(many.time_sync(done, n, rtt[done:done + n], radv[done:done + n]))
        dev.time_sync(done, n, rtt_d[done:done + n], radv_d[done:done + n], out=tuple(o[done:done + n] for o in outs_d))
        done += n
    assert done == CALLS
    assert_outputs(one.time_sync(0, CALLS, rtt, radv), m)
    assert_state(one, m)
    assert_outputs(tuple(np.concatenate([p[i] for p in pieces]) for i in range(3)), m)
    assert_state(many, m)
    dev.synchronize()
    assert_outputs(outs_d, m)
    assert_state(dev, m)
    check_sessions(one, rows, arrive, events, range(0, S, 13), CALLS)


@pytest.mark.parametrize("lds", ["0", "1"])
def test_both_window_forms(oracle, monkeypatch, lds):
    """GGRS_TIME_SYNC_LDS: a block's windows in LDS for the launch, or a push's slot touched in HBM;
    launches of 1, 7 and 8 calls and a partial group cross the kernel's groups of eight."""
    monkeypatch.setenv("GGRS_TIME_SYNC_LDS", lds)
    P, local, delay, mp = CASES[1][1:]
    rows, arrive, events, rtt, radv, m = parity_case(P, local, delay, mp)
    e = engine(P, local, delay, mp)
    e.add_inputs(0, rows)
    e.add_arrivals(0, arrive, events)
    e.advance_frames(CALLS)
    done = 0
    for n in (1, 7, 8, 9, 16, 100, 99):
        assert_outputs(e.time_sync(done, n, rtt[done:done + n], radv[done:done + n]), m, done)
        done += n
    assert done == CALLS
    assert_state(e, m)


def test_no_inputs_means_nothing_arrived(oracle):
    """rtt_ms and remote_advantage NULL: round_trip_time and remote_frame_advantage stay 0."""
    P, local, delay, mp = CASES[0][1:]
    rows, arrive, events, _, _, _ = parity_case(P, local, delay, mp)
    advanced, stop = oracle_tables(rows, arrive, events, P, 0b01, delay, mp)
    cur, pushed = T.tables(advanced, delay, stop)
    m = T.run(cur, pushed, np.maximum.accumulate(arrive, axis=0), events, 0b10, FPS, stop_call=stop)
    assert (m["frames_ahead"] > 0).any() and (m["state"][1] == 0).all() and (m["state"][2] == 0).all()
    e = engine(P, local, delay, mp)
    e.add_inputs(0, rows)
    e.add_arrivals(0, arrive, events)
    e.advance_frames(CALLS)
    assert_outputs(e.time_sync(0, CALLS), m)
    assert_state(e, m)


def test_packet_feed_last_recv_is_the_feeds_ack_row(oracle):
    """The packet-fed engine (random bytes in the remote columns of its rows): last_recv_frame comes
    from the feed's ack row."""
    P, local, delay, mp = CASES[0][1:]
    rows, arrive, events, rtt, radv, m = parity_case(P, local, delay, mp)
    mask = 0b01
    pk = F.run(rows, arrive, mask, mp, seed=P + mp)
    assert (pk["arrive"] == arrive).all()
    junk = rows.copy()
    cols = F.remote_columns(P, mask)
    junk[:, :, cols] = np.random.default_rng(99).integers(0, 256, junk[:, :, cols].shape, dtype=np.uint8)
    e = engine(P, local, delay, mp, feed=True)
    e.add_inputs(0, junk)
    done = 0
    for n in PIECES:
        e.receive_packets(done, pk["start"][done:done + n], pk["length"][done:done + n], pk["packets"][done:done + n],
                          events[done:done + n])
        e.advance_frames(n)
        assert_outputs(e.time_sync(done, n, rtt[done:done + n], radv[done:done + n]), m, done)
        done += n
    assert_state(e, m)
    status, ack = e.packet_results(0, CALLS)
    assert (ack == arrive).all()


def test_two_engines_hand_each_other_their_advantage_rows(oracle):
    """Engines A (local player 0) and B (local player 1), each under its own schedule, stepped call by
    call: the remote_advantage of call c is the other engine's local_advantage row of call c - 1, in
    device memory (call 0: nothing arrived).  Both equal two coupled models."""
    from oracle import oracle as o
    calls, mp, P = 150, 8, 2
    d = torch.device("cuda")
    side = []
    for k, (local, seed) in enumerate((((0,), 61), ((1,), 62))):
        mask = 1 << local[0]
        rows = np.stack([o.gen_inputs(o.session_seed(s, 0x7154 + k), calls, P, 0) for s in range(S)], axis=1)
        arrive, events = schedules(S, calls, mp, seed, mask, P, disconnect_every=9)
        advanced, stop = oracle_tables(rows, arrive, events, P, mask, 0, mp)
        cur, pushed = T.tables(advanced, 0, stop)
        rtt, _ = T.input_tables(S, calls, seed)
        side.append(dict(local=local, rows=rows, arrive=arrive, events=events, cur=cur, pushed=pushed, stop=stop,
                         rtt=rtt, recv=np.maximum.accumulate(arrive, axis=0), rmask=~mask & 3,
                         model=[T.Session(FPS) for _ in range(S)], out=T.new_outputs(calls, S)))
    for c in range(calls):  # the coupled models
        for x, other in ((side[0], side[1]), (side[1], side[0])):
            for s in range(S):
                radv = T.KEEP if c == 0 else int(other["out"]["local_advantage"][c - 1, s])
                r = x["model"][s].step(c, int(x["cur"][c, s]), int(x["recv"][c, s]), int(x["pushed"][c, s]),
                                       int(x["rtt"][c, s]), radv, bool(x["events"][c, s] & x["rmask"]),
                                       0 <= x["stop"][s] <= c)
                for name, v in zip(NAMES, r):
                    x["out"][name][c, s] = v
    for x in side:
        x["out"]["state"] = T.final_state(x["model"])
        assert ((x["out"]["skip_frames"] > 0).sum(axis=0) > 0).sum() > S // 8
        x["eng"] = engine(P, x["local"], 0, mp, cap=calls)
        x["eng"].add_inputs(0, x["rows"])
        x["eng"].add_arrivals(0, x["arrive"], x["events"])
        x["dev"] = tuple(torch.zeros((calls, S), dtype=torch.int32, device=d) for _ in range(3))
        x["rtt_d"] = torch.from_numpy(x["rtt"]).to(d)
    for c in range(calls):
        for x, other in ((side[0], side[1]), (side[1], side[0])):
            x["eng"].advance_frames(1)
            x["eng"].time_sync(c, 1, x["rtt_d"][c:c + 1], other["dev"][0][c - 1:c] if c else None,
                               out=tuple(o[c:c + 1] for o in x["dev"]))
        side[0]["eng"].synchronize()  # (each engine runs on its own stream)
        side[1]["eng"].synchronize()
    for x in side:
        assert_outputs(x["dev"], x["out"])
        assert_state(x["eng"], x["out"])


def test_misuse_raises(oracle):
    from ggrs_amd import InvalidRequest, P2PEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    from ggrs_amd.p2p import peer_report
    S_, P = 8, 3

    def fresh(schedule=True, local=(0,), cap=32):
        e = P2PEngine(S_, num_players=P, local_players=local, max_prediction=8, remote_latency=1, input_capacity=cap)
        if schedule:
            e.set_arrival_schedule(True)
        return e

    def state_error(f, *a):
        with pytest.raises(GgrsError) as err:
            f(*a)
        assert err.value.code == GGRS_E_STATE

    def feed(e, c0, n):
        e.add_inputs(c0, np.zeros((n, S_, P), np.uint8))
        e.add_arrivals(c0, np.repeat(np.arange(c0, c0 + n, dtype=np.int32)[:, None] - 1, S_, axis=1))

    state_error(fresh(schedule=False).set_time_sync, 60)  # a fixed-latency engine
    e = fresh()
    feed(e, 0, 8)
    state_error(e.time_sync, 0, 1)  # before set_time_sync
    state_error(e.time_sync_state)
    for fps in (0, 1001, -60):
        with pytest.raises(InvalidRequest):
            e.set_time_sync(fps)
    e.set_time_sync(1)
    e.set_time_sync(1000)
    e.set_time_sync(60)
    with pytest.raises(InvalidRequest):  # call 0 has not run
        e.time_sync(0, 1)
    e.advance_frames(4)
    state_error(e.set_time_sync, 60)  # configured after the first call
    with pytest.raises(InvalidRequest):  # out of order
        e.time_sync(1, 1)
    with pytest.raises(InvalidRequest):  # not yet run
        e.time_sync(0, 5)
    local, ahead, skip = e.time_sync(0, 2)
    assert (local == [[0], [-1]]).all() and (ahead == 0).all() and (skip == 0).all()
    with pytest.raises(InvalidRequest):  # each call once
        e.time_sync(1, 1)
    assert e.time_sync(2, 0)[0].shape == (0, S_)
    e.time_sync(2, 2)
    # calls no longer held: 40 more calls over an input_capacity of 32
    feed(e, 8, 24)
    e.advance_frames(24)
    feed(e, 32, 16)
    e.advance_frames(16)
    with pytest.raises(InvalidRequest, match="no longer held"):
        e.time_sync(4, 4)
    e = fresh(local=())  # no local player: no frame advantage to speak of
    with pytest.raises(InvalidRequest):
        e.set_time_sync(60)
    # peers' disconnect reports: whichever comes second
    rep = np.zeros((1, S_), np.int32)
    rep[0, 0] = peer_report(1, 2, -1)
    e = fresh()
    feed(e, 0, 4)
    e.set_time_sync(60)
    state_error(e.add_peer_reports, 0, rep)
    e = fresh()
    feed(e, 0, 4)
    e.add_peer_reports(0, rep)
    state_error(e.set_time_sync, 60)


def test_an_engine_without_time_sync_is_unchanged(oracle):
    """Configuring time sync changes nothing a session computes: sessions() and states() of an engine
    that configures it equal those of one that does not, which stores no per-call word and so cannot
    take a time_sync call at all."""
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    P, local, delay, mp = CASES[2][1:]
    rows, arrive, events, rtt, radv, m = parity_case(P, local, delay, mp)
    plain, ts = engine(P, local, delay, mp, time_sync=False), engine(P, local, delay, mp)
    for e in (plain, ts):
        e.add_inputs(0, rows)
        e.add_arrivals(0, arrive, events)
        for n in PIECES:
            e.advance_frames(n)
    assert (plain.states() == ts.states()).all()
    for a, b in zip(plain.sessions(), ts.sessions()):
        assert (a == b).all()
    for a, b in zip(plain.stats(), ts.stats()):
        assert (a == b).all()
    with pytest.raises(GgrsError) as err:
        plain.time_sync(0, 1)
    assert err.value.code == GGRS_E_STATE
    assert_outputs(ts.time_sync(0, CALLS, rtt, radv), m)
