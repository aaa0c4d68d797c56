"""CPU checks of tests/spectator_emit_model.py, the reference of the device's spectator emit
(ggrs_p2p_set_spectator_emit / emit_spectator_packets): the confirmed rows against the oracle's
P2PSession, the endpoints' rules case by case, and the closed loop of a modelled host and its
spectators through a lossy link -- whose tables the GPU end-to-end test
(tests/test_gpu_spectator_emit.py) reuses, so the conditions that test relies on are asserted here on
the model alone."""
import functools

import numpy as np

from tests import packet_feed_model as F
from tests import spectator_emit_model as M
from tests import spectator_feed_model as SF
from tests import spectator_model as SM

E2E = dict(S=130, K=2, P=2, local=(0,), calls=160, mp=8, W=64, tail=10)


@functools.lru_cache(maxsize=None)
def e2e_case():
    """The end-to-end test's inputs and the model's run of them: (rows [calls][S][P], arrive, events
    [calls][S], delay, drop, ack_drop, resend [calls][K][S], the link_run dict per session with its K
    receivers under "receivers")."""
    from oracle import oracle as O
    k = E2E
    S, K, P, calls = k["S"], k["K"], k["P"], k["calls"]
    mask = sum(1 << j for j in k["local"])
    rows = np.stack([O.gen_inputs(O.session_seed(s, 0x5EC7), calls, P, s % 2) for s in range(S)], axis=1)
    arrive, events = M.schedules(S, calls, k["mp"], 23, mask, P, disconnect_every=10)
    arrive[calls - k["tail"]:] = np.arange(calls - k["tail"], calls)[:, None] - 1  # the tail confirms promptly
    pushed, stop = M.pushed_table(rows, arrive, events, P, mask, 0, k["mp"])
    assert (stop < 0).all()
    delay, drop, ack_drop, resend = M.link_tables(calls, K, S, seed=43, tail=k["tail"])
    stride = F.max_packet_bytes(P, k["W"])
    runs = []
    for s in range(S):
        receivers = [SF.Receiver(calls + 16, P, k["mp"], k["W"], stride) for _ in range(K)]
        r = M.link_run(rows[:, s], arrive[:, s], events[:, s], pushed[:, s], mask, K, k["W"], delay[:, :, s],
                       drop[:, :, s], ack_drop[:, :, s], resend[:, :, s], receivers)
        r["receivers"] = receivers
        runs.append(r)
    return rows, arrive, events, delay, drop, ack_drop, resend, runs


def notes_taken(r, k):
    """The note each of spectator k's polls received: the note of the host call whose packet it took."""
    took = r["took"][:, k]
    return np.where(took >= 0, r["notes"][np.maximum(took, 0)], 0).astype(np.int32)


def spectate(recv, notes, rows, P):
    """SM.Spectator over a per-call arrival column -> (the spectator, advanced [calls], checksums
    [calls], {frame: state bytes after advancing it})."""
    sp = SM.Spectator(P)
    adv, cks, states = np.zeros(len(recv), np.uint8), np.zeros(len(recv), np.uint16), {}
    for c in range(len(recv)):
        adv[c] = sp.call(int(recv[c]), int(notes[c]), rows)
        cks[c] = sp.checksum
        if adv[c]:
            states[sp.current_frame] = bytes(sp.state)
    return sp, adv, cks, states


def test_confirmed_rows_replay_to_the_sessions_own_saved_states(oracle):
    """Where no player is disconnected the confirmed rows are the true inputs: a spectator fed them
    densely reaches, at frame f - 1, exactly the state the oracle's P2PSession saved for frame f --
    local bytes (from the row of the call that queued the frame, under input delay and threshold
    stalls) and remote bytes alike.  max_prediction 12 and stalls of 16 calls: one call of a burst
    confirms more than 8 frames."""
    O = oracle
    S, calls, mp = 24, 120, 12
    for P, local, delay in ((2, (0,), 0), (2, (1,), 2), (4, (0, 2), 1)):
        mask = sum(1 << j for j in local)
        rows = np.stack([O.gen_inputs(O.session_seed(s, 0xC0F), calls, P, 0) for s in range(S)], axis=1)
        arrive, events = M.schedules(S, calls, 16, 5 + P, mask, P, disconnect_every=0)
        pushed, stop = M.pushed_table(rows, arrive, events, P, mask, delay, mp)
        m = M.run(rows, arrive, events, pushed, mask, 1, 64, F.max_packet_bytes(P, 64))
        assert m["npush"].max() > 8 and (m["notes"] == 0).all()
        compared = 0
        for s in range(S):
            if stop[s] >= 0:
                continue
            out = O.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=mask,
                                  input_delay=delay, max_prediction=mp)
            nxt = int(m["next"][s])
            dense = np.minimum(np.arange(calls), nxt - 1)
            sp, _, _, states = spectate(dense, np.zeros(calls, np.int32), m["conf_rows"][:, s], P)
            assert sp.error == 0
            for f, st in zip(out["ring_frames"], out["ring_states"]):
                if 1 <= f <= nxt and f - 1 in states:
                    assert bytes(st) == states[f - 1], (P, s, f)
                    compared += 1
        assert compared >= S // 2


def test_confirmed_rows_and_notes_replay_under_disconnects(oracle):
    """The same check where a remote player disconnects in every second session: a spectator fed the
    model's confirmed table as its arrivals, its notes and its confirmed rows -- blank bytes past the
    player's last frame, the note's last_frame from the frozen connect status -- reaches the states
    the oracle's P2PSession saved after replaying that player as InputStatus::Disconnected.  This
    checks `confirmed`, last_frame and the blanking against the oracle, not against the derivation
    the kernel shares with the model."""
    O = oracle
    S, calls, mp = 24, 120, 12
    for P, local, delay in ((2, (0,), 0), (4, (0, 2), 1), (3, (1,), 2)):
        mask = sum(1 << j for j in local)
        rows = np.stack([O.gen_inputs(O.session_seed(s, 0xD15), calls, P, 0) for s in range(S)], axis=1)
        arrive, events = M.schedules(S, calls, 16, 3 + P, mask, P, disconnect_every=2)
        pushed, stop = M.pushed_table(rows, arrive, events, P, mask, delay, mp)
        m = M.run(rows, arrive, events, pushed, mask, 1, 64, F.max_packet_bytes(P, 64), stop_call=stop)
        compared = 0
        for s in range(0, S, 2):
            if stop[s] >= 0:
                continue
            out = O.p2p_sched_run(rows[:, s], arrive[:, s], events[:, s], num_players=P, local_mask=mask,
                                  input_delay=delay, max_prediction=mp)
            nxt = int(m["next"][s])
            recv = np.maximum.accumulate(m["confirmed"][:, s])
            sp, _, _, states = spectate(recv, m["notes"][:, s], m["conf_rows"][:, s], P)
            assert sp.error == 0 and (m["notes"][:, s] != 0).any()
            for f, st in zip(out["ring_frames"], out["ring_states"]):
                if 1 <= f <= nxt and f - 1 in states:
                    assert bytes(st) == states[f - 1], (P, s, f)
                    compared += 1
        assert compared >= S // 4, compared


def test_endpoint_cases(oracle):
    """Several pushes in one call make one packet; acks as packet_emit_model.Sender's; an overflow in
    the middle of a burst closes at the first push past the bound."""
    ep = M.Endpoint(2, 8)
    fr = {f: bytes([f * 5 & 0xff, 200 - f]) for f in range(20)}
    start, data = ep.step(0, pushes=[(f, fr[f]) for f in range(4)])
    assert start == 0 and F.codec_decode(bytes(2), data) == (0, [fr[f] for f in range(4)])
    assert ep.step(1) == (-1, b"")  # nothing pushed, no retry
    start, data = ep.step(2, ack=1, pushes=[(4, fr[4])])
    assert start == 2 and ep.last_acked == (1, fr[1]) and F.codec_decode(fr[1], data) == (0, [fr[2], fr[3], fr[4]])
    assert ep.step(3, ack=0) == (-1, b"") and ep.last_acked[0] == 1  # stale
    start, data = ep.step(4, resend=True)
    assert start == 2 and F.codec_decode(fr[1], data)[1] == [fr[2], fr[3], fr[4]]
    assert ep.step(5, ack=99) == (-1, b"") and ep.last_acked == (4, fr[4]) and not ep.pending  # beyond the newest
    assert ep.step(6, pushes=[(f, fr[f]) for f in range(5, 15)]) == (-1, b"")  # 10 > 8 pending
    assert (ep.status, ep.closed_call, len(ep.pending)) == (M.EMIT_DISCONNECTED, 6, 9)
    assert ep.step(7, ack=14, pushes=[(15, fr[15])], resend=True) == (-1, b"") and len(ep.pending) == 9


def tiny_session(K, max_pending, calls=40, P=2):
    rows = (np.arange(calls * P, dtype=np.uint8).reshape(calls, P) * 37 + 1).astype(np.uint8)
    arrive = (np.arange(calls) - 1).astype(np.int32)
    pushed = np.arange(calls, dtype=np.int32)
    return M.Session(rows, arrive, np.zeros(calls, np.uint8), pushed, 0b01, K, max_pending), rows


def test_overflow_and_lost_rows_leave_the_other_endpoints_running(oracle):
    ses, rows = tiny_session(3, 4)
    closed = None
    for c in range(20):
        conf, note, pushes, sent = ses.call(c, acks=[c - 3, -1, c - 2])  # endpoint 1 never acks
        assert conf == c - 1 and note == 0 and [f for f, _ in pushes] == ([c - 1] if c else [])
        if closed is None and ses.eps[1].status:
            closed = c
        for k in (0, 2):
            if c:
                assert sent[k][0] == ses.eps[k].last_acked[0] + 1
                rc, got = F.codec_decode(ses.eps[k].last_acked[1], sent[k][1])
                assert rc == 0 and got[-1] == bytes(rows[c - 1])
        if closed is not None:
            assert sent[1] == (-1, b"")
    assert closed == 5 and ses.eps[1].status == M.EMIT_DISCONNECTED and ses.eps[0].status == ses.eps[2].status == 0
    # a lost row closes every endpoint still open, after the call's pops, and the session pushes no more
    conf, note, pushes, sent = ses.call(20, acks=[18, -1, 18], held_from=30)
    assert pushes == [] and all(x == (-1, b"") for x in sent)
    assert [ep.status for ep in ses.eps] == [M.EMIT_ROW_LOST, M.EMIT_DISCONNECTED, M.EMIT_ROW_LOST]
    assert ses.eps[0].last_acked[0] == 18 and ses.eps[0].closed_call == 20 and ses.eps[1].closed_call == 5
    assert ses.call(21)[2] == [] and ses.host.next == 19


def test_disconnects_blank_the_later_frames_and_rotate_the_notes(oracle):
    """P = 4, local player 0: player 2 disconnects at call 10 (last frame 7), player 3 at call 14."""
    calls, P = 30, 4
    rows = np.full((calls, P), 9, np.uint8) + np.arange(calls, dtype=np.uint8)[:, None]
    arrive = (np.arange(calls) - 3).astype(np.int32).clip(-1)
    events = np.zeros(calls, np.uint8)
    events[10], events[14] = 1 << 2, 1 << 3
    ses = M.Session(rows, arrive, events, np.arange(calls, dtype=np.int32), 0b0001, 1, 64)
    got = {}
    for c in range(calls):
        conf, note, pushes, _ = ses.call(c)
        got.update(pushes)
        if c < 10:
            assert note == 0
        elif c < 14:
            assert note == SM.note(2, 7)
        else:
            assert note == (SM.note(2, 7), SM.note(3, 11))[c % 2]
    for f, b in got.items():
        assert b[0] == rows[f, 0] and b[1] == rows[f, 1]
        assert b[2] == (rows[f, 2] if f <= 7 else 0) and b[3] == (rows[f, 3] if f <= 11 else 0)
    assert max(got) == calls - 4


def test_stopped_session_takes_no_step(oracle):
    ses, _ = tiny_session(2, 8)
    ses.stop_call = 6
    for c in range(10):
        conf, note, pushes, sent = ses.call(c)
        assert (pushes == [] and sent == [(-1, b"")] * 2) if c >= 6 else (c == 0 or len(pushes) == 1)
    assert ses.host.next == 5 and all(len(ep.pending) == 5 for ep in ses.eps)


def test_lossy_link_rebuilds_the_confirmed_rows_and_the_spectators_follow(oracle):
    """Every receiver ends with exactly the rows the host pushed; a spectator over the link reaches,
    at every frame, the state of one fed the same rows densely; and the conditions of the GPU
    end-to-end test: every spectator advances, none is SpectatorTooFarBehind, no endpoint closes."""
    k = E2E
    rows, arrive, events, delay, drop, ack_drop, resend, runs = e2e_case()
    noted = 0
    for s, r in enumerate(runs):
        ses = r["session"]
        nxt = ses.host.next
        assert nxt > k["calls"] // 2 and sorted(r["pushes"]) == list(range(nxt))
        conf = np.stack([np.frombuffer(r["pushes"][f], np.uint8) for f in range(nxt)])
        dense, _, _, dense_states = spectate(np.minimum(np.arange(k["calls"]), nxt - 1), np.zeros(k["calls"], np.int32),
                                             conf, k["P"])
        for j in range(k["K"]):
            rx = r["receivers"][j]
            assert ses.eps[j].status == 0 and rx.stop_call is None
            # (the last call's packet, one frame of the prompt tail, is still on its way)
            assert rx.last == nxt - 2 and (rx.rows[:nxt - 1] == conf[:nxt - 1]).all(), (s, j)
            notes = notes_taken(r, j)
            sp, adv, _, states = spectate(r["recv"][:, j], notes, rx.rows, k["P"])
            assert sp.error == 0 and adv.sum() > 0, (s, j)
            if not (events[:, s] != 0).any():
                assert all(states[f] == dense_states[f] for f in states)
            else:
                noted += int((notes != 0).any())
    assert noted >= k["S"] // 10
    assert max(int((np.diff(r["recv"][:, 0]) > 8).any()) for r in runs) == 1  # a blackout's burst
