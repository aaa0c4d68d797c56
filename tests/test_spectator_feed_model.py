"""The spectator packet feed's Python model (tests/spectator_feed_model.py) against the model of the
table-fed engine (tests/spectator_model.py) and the rules of include/ggrs_amd.h: what the device
feed is compared with (tests/test_gpu_spectator_packets.py) must itself be right.  No GPU."""
import collections

import numpy as np

from tests import codec_cases as C
from tests import spectator_feed_model as M
from tests import spectator_model as SM

SUBSET = range(0, 130, 5)  # the sessions stepped through the (slow) spectator model here


def subset_of(feed, notes, sessions):
    idx = list(sessions)
    f = {k: (v[:, idx] if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for k, v in feed.items()}
    f["stop_call"] = feed["stop_call"][idx]
    return f, (None if notes is None else notes[:, idx])


def test_undamaged_packets_give_back_rows_and_schedule(oracle):
    """Every frame of every session arrives as sent, at the call the schedule names, whatever the
    overlap of re-sent frames."""
    for P in (1, 2, 4):
        rows, recv, notes, feed = M.parity_case(P)
        assert (feed["ack"] == recv).all() and (feed["recv"] == recv).all()
        assert (feed["stop_call"] == -1).all() and (feed["status"] >= 0).all()
        assert ((feed["status"] == 1) == (np.diff(recv, axis=0, prepend=-1) > 0)).all()
        for s in range(recv.shape[1]):
            upto = recv[-1, s] + 1
            assert (feed["rows"][:upto, s] == rows[:upto, s]).all(), s
            assert not feed["rows"][upto:, s].any()
        assert (feed["length"] <= feed["stride"]).all() and feed["length"].max() > 64
        # re-sent frames are there: some packet starts at or below what was acknowledged
        prev_ack = np.vstack([np.full((1, recv.shape[1]), -1, np.int32), feed["ack"][:-1]])
        assert ((feed["start"] >= 0) & (feed["start"] <= prev_ack)).sum() > recv.shape[1]


def test_spectators_over_the_feed_equal_spectators_over_the_schedule(oracle):
    P, mfb, speed = 2, 10, 3
    rows, recv, notes, feed = M.parity_case(P)
    f, nt = subset_of(feed, notes, SUBSET)
    got = M.run_spectators(f, nt, 512, mfb, speed, ops=M.receive_then_advance(recv.shape[0], 8))
    for i, s in enumerate(SUBSET):
        ref = SM.run(rows[:, s], recv[:, s], notes[:, s], num_players=P, max_frames_behind=mfb, catchup_speed=speed)
        assert (got["current_frame"][i], got["last_recv"][i], got["waited"][i], got["error"][i]) == \
            (ref["current_frame"], ref["last_recv"], ref["waited"], ref["error"]), s
        assert bytes(got["states"][i]) == bytes(ref["state"]), s
        assert (got["advanced"][:, i] == ref["advanced"]).all() and (got["checksums"][:, i] == ref["checksums"]).all()
    assert got["waited"].sum() > 0 and (got["advanced"] > 1).sum() > 0


def test_every_damage_kind_ends_as_the_rules_say(oracle):
    rows, host_upto, damage, feed = M.damage_case()
    calls, S = host_upto.shape
    assert set(feed["applied"].values()) == set(M.DAMAGE)
    for (c, s), kind in feed["applied"].items():
        st, stop = int(feed["status"][c, s]), int(feed["stop_call"][s])
        before = int(feed["ack"][c - 1, s])
        if kind in ("truncate", "random"):  # undecodable: a codec code, dropped whole
            assert st in (-1, -2, -3, M.CODEC_UNSUPPORTED, M.CODEC_E_CAP), (kind, st)
        elif kind == "withhold":
            assert st == 0 and feed["start"][c, s] < 0
        elif kind == "duplicate":  # every frame already held (or its reference gone by now)
            assert st in (0, M.NO_REFERENCE) and feed["start"][c, s] >= 0
        elif kind == "old_reference":
            assert st == M.NO_REFERENCE
        elif kind == "overlong":
            assert st == M.CODEC_E_CAP
        if kind == "gap":
            assert st == M.STOPPED and stop == c
            assert (feed["recv"][c:, s] == M.STOP_WORD).all() and (feed["ack"][c:, s] == before).all()
            assert (feed["status"][c + 1:, s] == 0).all() and (feed["start"][c + 1:, s] == -1).all()
        else:  # dropped or empty: nothing delivered at this call, the session goes on
            assert stop == -1 and feed["ack"][c, s] == before
            assert feed["ack"][-1, s] == host_upto[-1, s]
    damaged = sorted({s for _, s in damage})
    f, _ = subset_of(feed, None, damaged)
    k = M.DAMAGED
    got = M.run_spectators(f, None, k["cap"], k["mfb"], k["speed"], ops=M.receive_then_advance(calls, 8))
    for i, s in enumerate(damaged):
        stop = int(feed["stop_call"][s])
        if stop >= 0:
            assert got["error"][i] == M.E_PRECONDITION and (got["advanced"][stop:, i] == 0).all()
            assert got["current_frame"][i] <= feed["ack"][stop, s]
        else:
            assert got["error"][i] == 0 and got["last_recv"][i] == host_upto[-1, s]


def test_recoded_packets_deliver_or_are_dropped_by_their_kind(oracle):
    """codec_cases.recode's kinds on every third session: the accepting ones leave every status, ack and
    row as the sender's own bytes give them, the rejecting ones are dropped with their code and the
    next packet re-sends the frames; the spectators over the feed run on."""
    rows, host_upto, damage, feed, plain = M.recode_case()
    calls, S = host_upto.shape
    times = collections.Counter(feed["applied"].values())
    assert set(times) == set(M.PF.RECODE) and min(times.values()) >= 5, times
    assert (feed["stop_call"] == -1).all() and (plain["status"] >= 0).all()
    for (c, s), kind in feed["applied"].items():
        if kind in C.ACCEPTING:  # (the bytes differ from the sender's own: packet_feed_model.recoded)
            assert feed["status"][c, s] == plain["status"][c, s] == 1 and feed["ack"][c, s] == plain["ack"][c, s]
        else:
            assert feed["status"][c, s] == C.RECODE_STATUS[kind] and feed["ack"][c, s] == feed["ack"][c - 1, s]
    rejecting = sorted({s for (_, s), kind in feed["applied"].items() if kind in C.REJECTING})
    others = sorted(set(range(S)) - set(rejecting))
    for key in ("status", "ack", "recv", "rows"):  # (not start: a dropped packet shifts the later random overlaps)
        assert (feed[key][:, others] == plain[key][:, others]).all(), key
    assert (feed["ack"][-1] == host_upto[-1]).all()  # a dropped packet's frames come with the next one
    recoded = sorted({s for _, s in feed["applied"]})
    k = M.RECODED
    ops = M.receive_then_advance(calls, 8)
    got = M.run_spectators(subset_of(feed, None, recoded)[0], None, k["cap"], k["mfb"], k["speed"], ops=ops)
    ref = M.run_spectators(subset_of(plain, None, recoded)[0], None, k["cap"], k["mfb"], k["speed"], ops=ops)
    assert (got["error"] == 0).all() and (got["last_recv"] == host_upto[-1, recoded]).all()
    for i, s in enumerate(recoded):
        if s not in rejecting:
            assert bytes(got["states"][i]) == bytes(ref["states"][i]) and (got["checksums"][:, i] == ref["checksums"][:, i]).all()


def test_hosts_on_different_clocks_and_receives_queued_ahead(oracle):
    """The per-session window: with receive and advance call by call no session can need a row that
    left its window; with 64 calls of receives queued before each launch, the fast hosts' sessions
    do, and stop with E_PRECONDITION at that call."""
    rows, host_upto, feed = M.clock_case()
    calls = host_upto.shape[0]
    k = M.CLOCK
    assert host_upto[-1].max() - host_upto[-1].min() > k["cap"]
    f, _ = subset_of(feed, None, SUBSET)
    live = M.run_spectators(f, None, k["cap"], k["mfb"], k["speed"], ops=M.receive_then_advance(calls, 1))
    assert not (live["error"] == M.E_PRECONDITION).any() and (live["error"] == M.E_TOO_FAR_BEHIND).any()
    assert live["waited"].max() > 20 and (live["advanced"] > 1).any()
    ahead = M.run_spectators(f, None, k["cap"], k["mfb"], k["speed"], ops=M.receive_then_advance(calls, 64))
    stopped = ahead["error"] == M.E_PRECONDITION
    assert stopped.any() and not stopped.all()
    for i in np.nonzero(stopped)[0]:  # up to its stop the session ran as in the live loop
        c = int(np.nonzero(ahead["advanced"][:, i] != live["advanced"][:, i])[0][0])
        assert (ahead["advanced"][c:, i] == 0).all() and (ahead["checksums"][:c, i] == live["checksums"][:c, i]).all()


def test_library_exports_the_packet_feed():
    from ggrs_amd import _lib
    names = ("ggrs_spectator_set_packet_feed", "ggrs_spectator_receive_packets", "ggrs_spectator_read_packet_results")
    L = _lib.lib()
    for name in names:
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
