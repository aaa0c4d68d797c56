"""The packet feed's model (tests/packet_feed_model.py: a sender that re-sends what is unacknowledged
and UdpProtocol::on_input restated) on the CPU: undamaged packets give back the schedule they were
built from; under the GPU test's damage list every class of damage occurs, the effective schedule
stays a schedule, and the oracle's P2PSession runs it; the ABI's three layers name the feed's symbols."""
import os
import re

import collections

import numpy as np
import pytest

from tests import codec_cases as C
from tests import packet_feed_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ggrs_p2p_set_packet_feed", "ggrs_p2p_receive_packets", "ggrs_p2p_read_packet_results")


def test_undamaged_packets_give_back_the_schedule(oracle):
    S, calls, mp = 24, 150, 7
    for P, mask in ((2, 0b01), (4, 0b0101), (3, 0)):
        rows = np.stack([oracle.gen_inputs(oracle.session_seed(s, 3), calls, P, s % 2) for s in range(S)], axis=1)
        arrive = np.stack([oracle.stall_schedule(calls, mp, 40 + s, stall_every=40 if s % 3 else 10 ** 9)
                           for s in range(S)], axis=1).astype(np.int32)
        m = M.run(rows, arrive, mask, mp, seed=P)
        assert (m["arrive"] == arrive).all() and (m["ack"] == arrive).all()
        assert (m["rows"] == rows).all() and (m["stop_call"] == -1).all()
        rises = np.diff(np.vstack([np.full((1, S), -1), arrive]), axis=0) > 0
        assert ((m["status"] == 1) == rises).all() and ((m["start"] >= 0) == rises).all()
        # re-sent frames: some packets start at or below the acknowledged frame
        prev = np.vstack([np.full((1, S), -1), arrive[:-1]])
        assert ((m["start"] >= 0) & (m["start"] <= prev)).sum() > S


def test_long_packets_are_capped(oracle):
    """A burst longer than max_packet_inputs goes out as the first max_packet_inputs frames (the
    sender's pending queue), and a packet of max_packet_inputs + 1 frames is dropped with E_CAP."""
    calls, W, mp = 60, 16, 8
    rows = oracle.gen_inputs(7, calls, 2, 0).reshape(calls, 1, 2)
    arrive = np.full((calls, 1), -1, np.int32)
    arrive[40:, 0] = 30
    arrive[50:, 0] = 45
    m = M.run(rows, arrive, 0b01, mp, max_packet_inputs=W, overlap=False)
    assert m["ack"][40, 0] == W - 1 and m["ack"][50, 0] == 2 * W - 1 and (m["status"][[40, 50], 0] == 1).all()
    true_remote = np.ascontiguousarray(rows[:, 0, 1:])
    recv = M.Receiver(true_remote.copy(), mp, W, M.max_packet_bytes(1, W + 1))
    assert recv.receive(20, 0, M._encode(true_remote, 0, W)) == (M.CODEC_E_CAP, -1)
    assert recv.receive(21, 0, M._encode(true_remote, 0, W - 1)) == (1, W - 1)


def test_damaged_packets_leave_a_schedule_the_oracle_runs(oracle):
    P, mask, mp = 2, 0b01, 8
    rows, arrive, damage = M.damage_case(P=P, local_mask=mask, max_prediction=mp)
    calls, S = arrive.shape
    m = M.run(rows, arrive, mask, mp, seed=9, damage=damage)
    assert set(m["applied"].values()) == set(M.DAMAGE) | {"ahead"}
    assert m["applied"] == damage
    damaged = sorted({s for _, s in damage})
    assert damaged == list(range(0, S, 7))
    status_at = {kind: set() for kind in damage.values()}
    for (c, s), kind in damage.items():
        status_at[kind].add(int(m["status"][c, s]))
    assert status_at["truncate"] <= {-1, -2, -3} and status_at["withhold"] == {0} and status_at["duplicate"] == {0}
    assert status_at["old_reference"] == {M.NO_REFERENCE} and status_at["gap"] == status_at["ahead"] == {M.STOPPED}
    assert all(x < 0 for x in status_at["random"])
    ok = 0
    for s in range(S):
        eff, stop = m["arrive"][:, s], int(m["stop_call"][s])
        if s not in damaged:
            assert (eff == arrive[:, s]).all() and stop == -1
            continue
        upto = calls if stop < 0 else stop
        assert (np.diff(eff[:upto]) >= 0).all() and (eff[:upto] <= arrive[:upto, s]).all()
        assert (eff[:upto] < arrive[:upto, s]).any() or damage_kind(damage, s) in ("duplicate", "old_reference", "gap", "ahead")
        out = oracle.p2p_sched_run(m["rows"][:, s], eff, None, num_players=P, local_mask=mask, max_prediction=mp)
        if stop < 0:
            assert out["rc"] == 0, (s, out["rc"])
            ok += 1
        else:  # the arrival table's stop: a frame after its call, at the model's call
            assert out["rc"] == -1 and out["result"].frames_done == stop and eff[stop] > stop, (s, out["rc"])
            assert m["error"][s] == (M.E_INVALID if damage_kind(damage, s) == "ahead" else M.E_PRECONDITION)
            assert (eff[stop + 1:] == m["ack"][stop, s]).all()
    assert 2 * ok >= len(damaged)
    # an undecodable or withheld packet costs frames only until the next one: the sender re-sends
    assert (m["ack"][-1, damaged] == arrive[-1, damaged])[m["stop_call"][damaged] < 0].all()


@pytest.mark.parametrize("P,mask", [(2, 0b01), (3, 0b001)])
def test_recoded_packets_deliver_or_are_dropped_by_their_kind(oracle, P, mask):
    """The same inputs in other bytes (codec_cases.recode) on every third session, at several calls
    each, with 1 and 2 input bytes: the accepting kinds change nothing but the packets, the rejecting
    ones cost the packet (UNSUPPORTED / E_DELTA) and the sender's next one brings the frames."""
    mp = 8
    rows, arrive, damage = M.recode_case(P, mask, max_prediction=mp)
    calls, S = arrive.shape
    m = M.run(rows, arrive, mask, mp, seed=9, damage=damage)
    plain = M.run(rows, arrive, mask, mp, seed=9)
    times = collections.Counter(m["applied"].values())
    assert set(times) == set(M.RECODE) and min(times.values()) >= 5, times
    assert set(m["applied"]) <= set(damage) and (m["stop_call"] == -1).all()
    assert (plain["arrive"] == arrive).all()
    for (c, s), kind in m["applied"].items():
        assert m["start"][c, s] >= 0  # (the bytes differ from the sender's own: recoded())
        if kind in C.ACCEPTING:  # delivered wherever the undamaged packet would have been
            assert m["status"][c, s] == plain["status"][c, s] == 1 and m["ack"][c, s] == arrive[c, s], (c, s, kind)
        else:
            assert m["status"][c, s] == C.RECODE_STATUS[kind] and m["ack"][c, s] == m["ack"][c - 1, s], (c, s, kind)
    accepting = sorted({s for (_, s), kind in m["applied"].items() if kind in C.ACCEPTING})
    rejecting = sorted({s for (_, s), kind in m["applied"].items() if kind in C.REJECTING})
    untouched = sorted(set(range(S)) - set(rejecting))
    for key in ("status", "ack", "arrive"):  # (not start: a dropped packet shifts the later random overlaps)
        assert (m[key][:, untouched] == plain[key][:, untouched]).all(), key
    assert (m["rows"] == rows).all()
    assert ((m["status"] == 1) == (plain["status"] == 1))[:, accepting].all()
    for s in rejecting + accepting[:4]:
        eff = m["arrive"][:, s]
        assert (np.diff(eff) >= 0).all() and (eff <= arrive[:, s]).all()
        assert (s in accepting) or (eff < arrive[:, s]).any()
        out = oracle.p2p_sched_run(m["rows"][:, s], eff, None, num_players=P, local_mask=mask, max_prediction=mp)
        assert out["rc"] == 0, (s, out["rc"])


def test_existing_damage_is_untouched_by_the_recode_kinds(oracle):
    """The kinds apply only where a damage dict names them: the damage case's packets are what they were."""
    assert M.DAMAGE == ("truncate", "random", "withhold", "duplicate", "old_reference", "gap")
    assert not set(M.RECODE) & (set(M.DAMAGE) | {"ahead", "overlong"})
    rows, arrive, damage = M.damage_case()
    assert not set(damage.values()) & set(M.RECODE)


def damage_kind(damage, s):
    return next(kind for (_, ss), kind in damage.items() if ss == s)


def test_abi_names_the_packet_feed():
    """include/ggrs_amd.h, ggrs_amd/_lib.py EXPORTS and the Rust binding declare the feed's calls."""
    from ggrs_amd import _lib
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "ggrs-mi355x", "src", "ffi.rs")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert "GGRS_PACKET_NO_REFERENCE" in header and _lib.GGRS_PACKET_NO_REFERENCE == -16
