"""GPU parity of the spectator engine's packet feed (ggrs_spectator_set_packet_feed / receive_packets /
read_packet_results, csrc/spectator_ingest.hip, and the kFeed form of spectator_kernel) against
tests/spectator_feed_model.py -- its sender's wire packets go to the device, its receiver and
spectators are what the device must equal -- and, where the hosts stay within one window, against the
table-fed engine given the same rows and recv_upto.  Every session is compared: states,
read_sessions' four arrays, the (advanced, checksum) trace, packet status and ack."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import spectator_feed_model as M  # noqa: E402
from tests import spectator_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

MP = 8


def feed_engine(S, P, cap, mfb, speed, W, stride, calls, mp=MP):
    from ggrs_amd import SpectatorEngine
    e = SpectatorEngine(S, num_players=P, max_frames_behind=mfb, catchup_speed=speed, input_capacity=cap,
                        trace_capacity=calls)
    e.set_packet_feed(mp, W, stride)
    return e


def run_ops(e, feed, notes, ops):
    """receive_packets / advance_frames in the order of ops; -> (status, ack) of every call, read
    after each receive."""
    status, ack, got = [], [], 0
    for op, n in ops:
        if op == "recv":
            sl = slice(got, got + n)
            e.receive_packets(got, feed["start"][sl], feed["length"][sl], feed["packets"][sl],
                              None if notes is None else notes[sl])
            st, ak = e.read_packet_results(got, n)
            status.append(st)
            ack.append(ak)
            got += n
        else:
            e.advance_frames(n)
    return np.concatenate(status), np.concatenate(ack)


def reads(e, calls):
    cur, last, waited, err = e.sessions()
    adv, cks = e.trace(0, calls)
    return dict(current_frame=cur, last_recv=last, waited=waited, error=err, states=e.states(), advanced=adv,
                checksums=cks)


def assert_equal(got, ref, what):
    for k in ("error", "current_frame", "last_recv", "waited", "advanced", "checksums", "states"):
        bad = np.argwhere(np.asarray(got[k]) != np.asarray(ref[k]))
        assert len(bad) == 0, (what, k, bad[:4].tolist())


def assert_feed(e, feed, notes, ops, cap, mfb, speed, what):
    """The engine over ops equals the model over ops: packet results and every session."""
    calls = feed["recv"].shape[0]
    status, ack = run_ops(e, feed, notes, ops)
    bad = np.argwhere(status != feed["status"])
    assert len(bad) == 0, (what, "status", bad[:4].tolist())
    assert (ack == feed["ack"]).all(), (what, "ack")
    model = M.run_spectators(feed, notes, cap, mfb, speed, ops=ops)
    got = reads(e, calls)
    assert_equal(got, model, what)
    return got, model


# ---- 1. parity with the table-fed engine and the model

@pytest.mark.parametrize("P,speed", [(1, 1), (1, 3), (2, 1), (2, 3), (4, 1), (4, 3)])
def test_packet_fed_engine_equals_the_table_fed_engine_and_the_model(oracle, P, speed):
    from ggrs_amd import SpectatorEngine
    rows, recv, notes, feed = M.parity_case(P)
    calls, S = recv.shape
    cap, mfb = 512, 10
    assert (feed["ack"] == recv).all() and (notes != 0).sum() > 10
    ops = M.receive_then_advance(calls, 24)
    A = feed_engine(S, P, cap, mfb, speed, 64, feed["stride"], calls)
    got, model = assert_feed(A, feed, notes, ops, cap, mfb, speed, "model")
    assert model["waited"].sum() > 0 and not (model["error"] == M.E_PRECONDITION).any()
    if speed > 1:  # every burst is caught up on
        assert (model["advanced"] > 1).sum() > S and (model["error"] == 0).all()
    else:  # the hosts that run 3 frames per call are lost
        assert 1 <= (model["error"] == M.E_TOO_FAR_BEHIND).sum() <= S // 4
    B = SpectatorEngine(S, num_players=P, max_frames_behind=mfb, catchup_speed=speed, input_capacity=cap,
                        trace_capacity=calls)
    B.add_inputs(0, feed["rows"])
    B.add_arrivals(0, feed["recv"], notes)
    for op, n in ops:
        if op == "adv":
            B.advance_frames(n)
    assert_equal(got, reads(B, calls), "table-fed engine")
    A.close()
    B.close()


def test_one_session(oracle):
    P, mfb, speed, cap, calls = 2, 10, 3, 512, 120
    rows, recv, notes, _ = M.parity_case(P)
    s = 35  # s % 5 == 0: a note; s % 8 == 3: the host jumps 40 frames ahead at call 60
    rows, recv, notes = rows[:, s:s + 1], recv[:calls, s:s + 1], notes[:calls, s:s + 1]
    feed = M.run_feed(rows, recv, MP, 64, seed=3)
    assert (notes != 0).sum() == 1 and (feed["ack"] == recv).all()
    A = feed_engine(1, P, cap, mfb, speed, 64, feed["stride"], calls)
    got, model = assert_feed(A, feed, notes, M.receive_then_advance(calls, 7), cap, mfb, speed, "S = 1")
    ref = SM.run(rows[:, 0], recv[:, 0], notes[:, 0], num_players=P, max_frames_behind=mfb, catchup_speed=speed)
    assert bytes(got["states"][0]) == bytes(ref["state"]) and got["current_frame"][0] == ref["current_frame"]
    assert (got["advanced"][:, 0] > 1).any()


# ---- 2. hosts on different clocks

def test_hosts_on_different_clocks(oracle):
    """Hosts at 0.5, 1 and 1.5 frames per call with stalls and bursts over input_capacity 64: by the
    end the hosts are several windows apart, which no table-fed engine can hold."""
    rows, host_upto, feed = M.clock_case()
    calls, S = host_upto.shape
    k = M.CLOCK
    ops = M.receive_then_advance(calls, 1)
    model = M.run_spectators(feed, None, k["cap"], k["mfb"], k["speed"], ops=ops)
    # conditions on the inputs, on the model alone
    assert feed["ack"][-1].max() - feed["ack"][-1].min() > k["cap"]
    assert (model["waited"] > 0).any() and (model["advanced"] > 1).any()
    assert (model["error"] == M.E_TOO_FAR_BEHIND).any() and not (model["error"] == M.E_PRECONDITION).any()
    assert (feed["stop_call"] == -1).all() and feed["ack"][-1].max() > 4 * k["cap"]
    A = feed_engine(S, k["P"], k["cap"], k["mfb"], k["speed"], k["W"], feed["stride"], calls, k["mp"])
    assert_feed(A, feed, None, ops, k["cap"], k["mfb"], k["speed"], "clocks")


# ---- 3. the live loop in pieces

def test_live_loop_in_pieces(oracle):
    P, mfb, speed, cap = 2, 10, 3, 512
    rows, recv, notes, feed = M.parity_case(P)
    calls, S = recv.shape
    first = None
    for piece in (1, 3, 8, 64):
        A = feed_engine(S, P, cap, mfb, speed, 64, feed["stride"], calls)
        got, _ = assert_feed(A, feed, notes, M.receive_then_advance(calls, piece), cap, mfb, speed, f"pieces of {piece}")
        if first is None:
            first = got
        assert_equal(got, first, f"pieces of {piece} against pieces of 1")
        A.close()


def test_receives_queued_too_far_ahead_stop_sessions(oracle):
    """64 calls of receives before each launch over input_capacity 64: the fast hosts' frames leave
    the window before their sessions advance them."""
    rows, host_upto, feed = M.clock_case()
    calls, S = host_upto.shape
    k = M.CLOCK
    ops = M.receive_then_advance(calls, 64)
    model = M.run_spectators(feed, None, k["cap"], k["mfb"], k["speed"], ops=ops)
    stopped = model["error"] == M.E_PRECONDITION
    assert stopped.sum() >= S // 4 and (~stopped).sum() >= S // 4
    A = feed_engine(S, k["P"], k["cap"], k["mfb"], k["speed"], k["W"], feed["stride"], calls, k["mp"])
    got, _ = assert_feed(A, feed, None, ops, k["cap"], k["mfb"], k["speed"], "queued ahead")
    assert ((got["error"] == M.E_PRECONDITION) == stopped).all()


# ---- 4. damage

def test_damaged_packets(oracle):
    rows, host_upto, damage, feed = M.damage_case()
    calls, S = host_upto.shape
    k = M.DAMAGED
    ops = M.receive_then_advance(calls, 17)
    model = M.run_spectators(feed, None, k["cap"], k["mfb"], k["speed"], ops=ops)
    assert set(feed["applied"].values()) == set(M.DAMAGE)
    stopped = feed["stop_call"] >= 0
    assert stopped.sum() >= 2 and (model["error"][stopped] == M.E_PRECONDITION).all()
    assert (model["error"][~stopped] == 0).all() and (~stopped).sum() >= S // 2
    assert (feed["status"] == M.STOPPED).sum() == stopped.sum() and (feed["status"] == M.NO_REFERENCE).sum() >= 2
    assert (feed["status"] == M.CODEC_E_CAP).sum() >= 2
    A = feed_engine(S, k["P"], k["cap"], k["mfb"], k["speed"], k["W"], feed["stride"], calls, k["mp"])
    got, _ = assert_feed(A, feed, None, ops, k["cap"], k["mfb"], k["speed"], "damage")
    for s in np.nonzero(stopped)[0]:  # stopped at the model's call: nothing advances from there on
        assert (got["advanced"][feed["stop_call"][s]:, s] == 0).all()


def test_recoded_packets(oracle):
    """tests/codec_cases.py's recode on every third session, at several calls each: the accepting kinds
    deliver (status 1 wherever the sender's own bytes would have), the rejecting ones are dropped with
    UNSUPPORTED / E_DELTA; status, ack and every session equal the model's, and the table-fed engine
    given the receivers' rows and words."""
    import collections
    from ggrs_amd import SpectatorEngine
    from tests import codec_cases as C
    rows, host_upto, damage, feed, plain = M.recode_case()
    calls, S = host_upto.shape
    k = M.RECODED
    times = collections.Counter(feed["applied"].values())
    assert set(times) == set(M.PF.RECODE) and min(times.values()) >= 5, times
    assert (feed["stop_call"] == -1).all() and rows.shape[0] <= k["cap"]
    ops = M.receive_then_advance(calls, 17)
    A = feed_engine(S, k["P"], k["cap"], k["mfb"], k["speed"], k["W"], feed["stride"], calls, k["mp"])
    got, model = assert_feed(A, feed, None, ops, k["cap"], k["mfb"], k["speed"], "recode")
    status, _ = A.read_packet_results(0, calls)
    for (c, s), kind in feed["applied"].items():
        want = 1 if kind in C.ACCEPTING else C.RECODE_STATUS[kind]
        assert status[c, s] == want, (c, s, kind, status[c, s])
    accepting = sorted({s for (_, s), kind in feed["applied"].items() if kind in C.ACCEPTING})
    assert (status[:, accepting] == plain["status"][:, accepting]).all()
    assert (model["error"] == 0).all()
    B = SpectatorEngine(S, num_players=k["P"], max_frames_behind=k["mfb"], catchup_speed=k["speed"],
                        input_capacity=k["cap"], trace_capacity=calls)
    B.add_inputs(0, feed["rows"])
    B.add_arrivals(0, feed["recv"], None)
    for op, n in ops:
        if op == "adv":
            B.advance_frames(n)
    assert_equal(got, reads(B, calls), "table-fed engine")
    A.close()
    B.close()


def test_both_feeds_agree_on_the_same_packets(oracle):
    """The damage case's packets go to a packet-fed SpectatorEngine and to a packet-fed P2PEngine whose
    two remote players are the spectator's two players: the receive side both kernels share
    (csrc/ingest_device.h) must give every (call, session) the same status and ack, the models'."""
    from ggrs_amd import P2PEngine
    from tests import packet_feed_model as PF
    rows, host_upto, damage, feed = M.damage_case()
    calls, S = host_upto.shape
    k = M.DAMAGED
    # on the models alone: no rule only the P2P feed has fires.  Every input row is added first and
    # calls <= input_capacity, so every row slot holds its frame; no packet names a frame after its call;
    # and packet_feed_model's receiver over the same packets gives the spectator model's results.
    assert calls <= k["cap"] and (feed["ack"] <= np.arange(calls)[:, None]).all()
    assert set(feed["applied"].values()) == set(M.DAMAGE) and (feed["stop_call"] >= 0).sum() >= 2
    for s in range(S):
        r = PF.Receiver(np.zeros((calls, k["P"]), np.uint8), k["mp"], k["W"], feed["stride"], cap=k["cap"],
                        row_hi=lambda c: calls - 1)
        for c in range(calls):
            status, _ = r.receive(c, int(feed["start"][c, s]), feed["packets"][c, s, :feed["length"][c, s]].tobytes())
            assert (status, r.last) == (feed["status"][c, s], feed["ack"][c, s]), (c, s)
    spec = feed_engine(S, k["P"], k["cap"], k["mfb"], k["speed"], k["W"], feed["stride"], calls, k["mp"])
    p2p = P2PEngine(S, num_players=k["P"] + 1, local_players=(0,), max_prediction=k["mp"], remote_latency=1,
                    input_capacity=k["cap"])
    p2p.set_arrival_schedule(True)
    p2p.set_packet_feed(k["W"], feed["stride"])
    p2p.add_inputs(0, np.zeros((calls, S, k["P"] + 1), np.uint8))
    done = 0
    for n in (1, 3, 60, 17, calls - 81):  # (groups of 8 calls, whole and partial)
        sl = slice(done, done + n)
        for e in (spec, p2p):
            e.receive_packets(done, feed["start"][sl], feed["length"][sl], feed["packets"][sl])
        done += n
    got_spec, got_p2p = spec.read_packet_results(0, calls), p2p.packet_results(0, calls)
    for what, x, y in (("status", got_spec[0], got_p2p[0]), ("ack", got_spec[1], got_p2p[1])):
        bad = np.argwhere(x != y)
        assert len(bad) == 0, (what, "spectator feed against P2P feed", bad[:4].tolist())
        bad = np.argwhere(x != feed[what])
        assert len(bad) == 0, (what, "against the model", bad[:4].tolist())
    spec.close()
    p2p.close()


# ---- 5. the ingest kernel's staging forms

@pytest.mark.parametrize("P,W,cap,stride", [(2, 16, 64, None), (2, 32, 64, 256), (4, 128, 256, None), (4, 128, 256, 1012)])
def test_kernel_staging_forms(oracle, P, W, cap, stride):
    """Packet rows of which 8, 3 and 1 calls fit the block's LDS at a time; a network silent for more
    than max_packet_inputs calls, so that full packets follow (P = 4, 128 inputs: a 512-byte stream of
    random bytes, literal stretches with two-byte headers); the 64-row ring wraps several times; one
    stale duplicate per third session (every frame already held: status 0)."""
    S, calls, mfb, speed = 70, 160, 10, 3
    rows = np.random.default_rng(P * W).integers(0, 256, (2 * calls + W, S, P), dtype=np.uint8)
    c = np.arange(calls)
    host_upto = np.zeros((calls, S), np.int32)
    for s in range(S):
        r = np.floor((1.0, 1.5)[s % 2] * (c + 1)).astype(np.int64) - 1
        if s % 5 != 4:
            r[10:10 + W + 4] = r[9]
        host_upto[:, s] = np.maximum.accumulate(r)
    damage = {(calls - 10, s): "duplicate" for s in range(0, S, 3)}
    feed = M.run_feed(rows, host_upto, MP, W, stride=stride, seed=W, damage=damage)
    counts = np.where(feed["start"] >= 0, feed["ack"] - np.vstack([np.full((1, S), -1), feed["ack"][:-1]]), 0)
    assert feed["applied"] == damage and all(feed["status"][cs] == 0 and feed["start"][cs] >= 0 for cs in damage)
    assert counts.max() >= W - 3 and feed["ack"][-1].min() > 2 * 64
    if P * W == 512:
        assert feed["length"].max() > 512 + 8  # a literal stream: longer than the inputs it carries
    ops = M.receive_then_advance(calls, 20)
    A = feed_engine(S, P, cap, mfb, speed, W, feed["stride"], calls)
    got, model = assert_feed(A, feed, None, ops, cap, mfb, speed, "staging")
    assert (model["error"][4::5] == 0).all()  # the networks without the silence
    assert (model["error"] == M.E_TOO_FAR_BEHIND).any() == (W > 60)  # a burst of a whole buffer: lost, still receiving


# ---- 6. device pointers

def test_packets_in_device_memory(oracle):
    """The packets are encoded on the device (ggrs_codec_encode) from dense arrays and received in
    place; a second engine receives the same bytes from host memory."""
    from ggrs_amd import InvalidRequest, codec
    S, calls, P, W, cap, mfb, speed = 130, 64, 2, 8, 128, 10, 3  # (64 calls queued ahead of one launch: 96 frames)
    dev = torch.device("cuda:0")
    rows = M.host_inputs(S, 2 * calls, P, 0x0DE7)
    c, s = np.arange(calls)[:, None], np.arange(S)[None, :]
    upto = (np.floor(np.array([0.5, 1.0, 1.5])[s % 3] * (c + 1)) - 1).astype(np.int32)
    before = np.vstack([np.full((1, S), -1, np.int32), upto[:-1]])
    start = np.where(before < 0, 0, np.maximum(before + 1 - (c + s) % 3, 0)).astype(np.int32)
    count = np.where(upto > before, upto - start + 1, 0).astype(np.int32)
    assert count.max() <= W and (count > 0).sum() > calls * S // 3
    rows_d = torch.from_numpy(rows).to(dev)
    start_d, count_d = torch.from_numpy(start).to(dev), torch.from_numpy(count).to(dev)
    sess = torch.arange(S, device=dev)[None, :].expand(calls, S)
    frames = (start_d[:, :, None] + torch.arange(W, device=dev, dtype=torch.int32)).long()
    pending = rows_d[frames, sess[:, :, None].expand(calls, S, W)].reshape(calls * S, W, P)
    ref = torch.where((start_d > 0)[:, :, None], rows_d[torch.clamp(start_d - 1, min=0).long(), sess],
                      torch.zeros((calls, S, P), dtype=torch.uint8, device=dev)).reshape(calls * S, P)
    stride = codec.max_packet_bytes(P, W)
    packets, length = codec.encode(ref.contiguous(), pending.contiguous(), count_d.reshape(-1).contiguous(), stride=stride)
    has = count_d > 0
    length = torch.where(has, length.reshape(calls, S), torch.zeros_like(count_d)).contiguous()
    start_d = torch.where(has, start_d, torch.full_like(start_d, -1)).contiguous()
    packets = packets.reshape(calls, S, stride).contiguous()
    notes = np.zeros((calls, S), np.int32)
    notes[20, 3], notes[30, 4] = SM.note(1, 15), SM.note(0, 22)
    bad = notes.copy()
    bad[5, 6], bad[6, 7], bad[7, 8] = 2, SM.note(3, 1), -7  # no note bit, a player the session lacks, negative
    torch.cuda.synchronize()
    A = feed_engine(S, P, cap, mfb, speed, W, stride, calls)
    B = feed_engine(S, P, cap, mfb, speed, W, stride, calls)
    host = [start_d.cpu().numpy(), length.cpu().numpy(), packets.cpu().numpy()]
    with pytest.raises(InvalidRequest):  # a malformed note in host memory
        B.receive_packets(0, *host, bad)
    A.receive_packets(0, start_d, length, packets, torch.from_numpy(bad).to(dev), on_device=True)
    B.receive_packets(0, *host, notes)
    A.advance_frames(calls)
    B.advance_frames(calls)
    a, b = reads(A, calls), reads(B, calls)
    assert_equal(a, b, "device against host memory")
    for x, y in zip(A.read_packet_results(0, calls), B.read_packet_results(0, calls)):
        assert (x == y).all()
    assert (a["last_recv"] == upto[-1]).all() and (a["error"] == 0).all() and a["current_frame"].min() > 20
    assert (A.read_packet_results(0, calls)[1] == upto).all()
    with pytest.raises(InvalidRequest):  # host arrays where device tensors are announced
        A.receive_packets(calls, *host, None, on_device=True)


# ---- 7. misuse

def test_misuse_raises(oracle):
    from ggrs_amd import InvalidRequest, SpectatorEngine
    from ggrs_amd._lib import GGRS_E_STATE, GgrsError
    S, P, W, cap = 8, 2, 16, 64
    stride = M.max_packet_bytes(P, W)
    none = (np.full((1, S), -1, np.int32), np.zeros((1, S), np.int32), np.zeros((1, S, stride), np.uint8))

    def fresh():
        return SpectatorEngine(S, num_players=P, input_capacity=cap, trace_capacity=8)

    def state_error(call, *args):
        with pytest.raises(GgrsError) as err:
            call(*args)
        assert err.value.code == GGRS_E_STATE, err.value

    e = fresh()
    state_error(e.receive_packets, 0, *none)  # without the feed
    state_error(e.read_packet_results, 0, 0)
    for mp, w, st in ((MP, 0, stride), (MP, 129, 1012), (MP, W, stride - 4), (MP, W, stride + 2), (MP, W, 1016),
                      (-1, W, stride), (24, W, stride), (MP, 48, M.max_packet_bytes(P, 48))):
        with pytest.raises(InvalidRequest):  # (the last two: input_capacity 64 <= 2 max_prediction + max_packet_inputs)
            e.set_packet_feed(mp, w, st)
    e.add_inputs(0, np.zeros((1, S, P), np.uint8))
    state_error(e.set_packet_feed, MP, W, stride)  # after the first input
    e = fresh()
    e.add_arrivals(0, np.full((1, S), -1, np.int32))
    state_error(e.set_packet_feed, MP, W, stride)  # after the first arrival
    e = fresh()
    e.set_packet_feed(MP, W, stride)
    e.set_packet_feed(MP, W, stride + 4)  # still configuration
    stride += 4
    none = none[:2] + (np.zeros((1, S, stride), np.uint8),)
    state_error(e.add_inputs, 0, np.zeros((1, S, P), np.uint8))  # refused in packet mode
    state_error(e.add_arrivals, 0, np.full((1, S), -1, np.int32))
    with pytest.raises(InvalidRequest):  # out of order
        e.receive_packets(1, *none)
    with pytest.raises(InvalidRequest):  # no packets received for the call
        e.advance_frames(1)
    with pytest.raises(InvalidRequest):  # a malformed note
        e.receive_packets(0, *none, np.full((1, S), 4, np.int32))
    with pytest.raises(InvalidRequest):  # more than input_capacity calls ahead of the next call
        e.receive_packets(0, *(np.repeat(a, cap + 1, axis=0) for a in none))
    # lengths outside the packet row are GGRS_CODEC_E_INVALID, read nowhere
    start, length, packets = (a.copy() for a in none)
    start[0, :3], length[0, :3] = 0, (stride + 1, -3, 1 << 30)
    e.receive_packets(0, start, length, packets)
    with pytest.raises(InvalidRequest):
        e.receive_packets(0, *none)
    with pytest.raises(InvalidRequest):
        e.read_packet_results(0, 2)
    status, ack = e.read_packet_results(0, 1)
    assert (status[0, :3] == M.CODEC_E_INVALID).all() and (status[0, 3:] == 0).all() and (ack == -1).all()
    e.advance_frames(1)
    state_error(e.set_packet_feed, MP, W, stride)  # after the first call
    cur, last, waited, err = e.sessions()
    assert (cur == -1).all() and (last == -1).all() and (waited == 1).all() and (err == 0).all()
    # a first packet that does not start at frame 0 stops its session
    start, length, packets = (a.copy() for a in none)
    start[0, 2] = 1
    e.receive_packets(1, start, length, packets)
    e.advance_frames(1)
    status, ack = e.read_packet_results(1, 1)
    assert status[0, 2] == M.STOPPED and (np.delete(status[0], 2) == 0).all()
    assert (e.sessions()[3] == np.where(np.arange(S) == 2, M.E_PRECONDITION, 0)).all()
