"""The two spectator poll units on the CPU (tests/spectator_poll_model.py): each lean model against its
literal restatement over LiteralProtocol on the GPU tests' own inputs, call by call and field by field,
every class of every clock shown not to be vacuous, hand-derived traces, and the header / binding check."""
import os
import re

import numpy as np
import pytest

from tests import spectator_poll_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = M.CASE_START
NAMES = {"host": M.HOST_NAMES, "link": M.LINK_NAMES}


def as_i64(a):
    return np.array([int(v) & (2 ** 64 - 1) for v in a], np.uint64).astype(np.int64)  # (-1: the call fields)


# ---- the lean and the literal model agree

@pytest.mark.parametrize("feed", (False, True))
@pytest.mark.parametrize("kind", M.CLOCKS)
def test_the_spectators_models_agree_after_every_call(kind, feed):
    now, kinds, events = M.host_case(kind)
    n, S = kinds.shape
    status = np.where(np.random.default_rng(5).random(kinds.shape) < 0.2, -3, 1).astype(np.int32) if feed else None
    lean = M.HostEndpoints(S, M.CASE_TIMEOUT, M.CASE_NOTIFY, T0)
    lits = [M.LiteralSpectatorSession(M.CASE_TIMEOUT, M.CASE_NOTIFY, T0) for _ in range(S)]
    queued = []
    for c in range(n):
        got = lean.step(c, now[c], kinds[c], None if status is None else status[c], events[c])
        for s, lit in enumerate(lits):
            decodes = status is None or status[c, s] >= 0
            r = lit.poll_remote_clients(c, int(now[c]), int(kinds[c, s]), decodes, bool(events[c, s]))
            assert tuple(int(g[s]) for g in got) == r[:3], (c, s)
            queued += r[3]
        for g, w in zip(lean.fields(), zip(*(lit.fields() for lit in lits))):
            assert (g.astype(np.int64) == as_i64(w)).all(), c
    # the endpoint never leaves Running, however often its host vanished
    assert all(lit.host.state == M.RUNNING for lit in lits)
    assert "KeepAlive" not in queued and "QualityReport" in queued and "InputAck" in queued


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("kind", M.CLOCKS)
def test_the_links_models_agree_after_every_call(kind, K):
    now, kinds, close_in, over = M.link_case(kind, K, overflow=True)
    n, E = kinds.shape
    lean = M.SpectatorEndpoints(E, M.CASE_TIMEOUT, M.CASE_NOTIFY, T0)
    lits = [M.LiteralSpectatorLink(M.CASE_TIMEOUT, M.CASE_NOTIFY, T0) for _ in range(E)]
    queued = []
    for c in range(n):
        got = lean.step(c, now[c], kinds[c], close_in[c], over[c])
        for e, lit in enumerate(lits):
            r = lit.call(c, int(now[c]), int(kinds[c, e]), bool(close_in[c, e]), bool(over[c, e]))
            assert tuple(int(g[e]) for g in got) == r[:3], (c, e)
            queued += r[3]
        for g, w in zip(lean.fields(), zip(*(lit.fields() for lit in lits))):
            assert (g.astype(np.int64) == as_i64(w)).all(), c
    assert "KeepAlive" not in queued and "InputAck" not in queued and "QualityReport" in queued


# ---- no class of no clock is vacuous

@pytest.mark.parametrize("kind", M.CLOCKS)
def test_every_class_of_the_spectators_raises_what_it_must(kind):
    M.assert_host_case_is_not_vacuous(kind, M.host_run(kind))


@pytest.mark.parametrize("overflow", (False, True))
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("kind", M.CLOCKS)
def test_every_class_of_the_links_raises_what_it_must(kind, K, overflow):
    M.assert_link_case_is_not_vacuous(kind, M.link_run(kind, K, overflow), overflow)


# ---- hand-derived traces: the spectator engine's unit

def host(clocks, kinds=None, events=None, timeout=2000, notify=500):
    n = len(clocks)
    k = np.zeros((n, 1), np.uint8) if kinds is None else np.array(kinds, np.uint8)[:, None]
    e = np.zeros((n, 1), np.uint8) if events is None else np.array(events, np.uint8)[:, None]
    return M.run_host(1, timeout, notify, T0, np.array(clocks, np.uint64), k, e)


def link(clocks, kinds=None, close_in=None, overflow=None, timeout=2000, notify=500):
    n = len(clocks)
    k = np.zeros((n, 1), np.uint8) if kinds is None else np.array(kinds, np.uint8)[:, None]
    ci = np.zeros((n, 1), np.uint8) if close_in is None else np.array(close_in, np.uint8)[:, None]
    ov = None if overflow is None else np.array(overflow, bool)[:, None]
    return M.run_links(1, timeout, notify, T0, np.array(clocks, np.uint64), k, ci, ov)


def col(m, name):
    return m[name][:, 0].tolist()


I, R, D, SH = M.NET_INTERRUPTED, M.NET_RESUMED, M.NET_DISCONNECTED, M.NET_SHUTDOWN


def test_the_spectators_endpoint_never_leaves_running_and_raises_one_disconnected():
    """Silent past the timeout, a message, silent again for longer than 5 s and past the timeout again,
    then a disconnect request: one Disconnected (the timeout's), interrupted / resumed recur after it,
    no Shutdown, acks and reports to the end."""
    t = [T0, T0 + 501, T0 + 2001, T0 + 2100, T0 + 2601, T0 + 9000, T0 + 9100, T0 + 9200]
    m = host(t, kinds=[0, 0, 0, M.K_INPUT, 0, 0, M.K_INPUT, M.K_INPUT], events=[0, 0, 0, 0, 0, 0, 0, 1])
    assert col(m, "net_events") == [0, I, D, R, I, 0, R, 0]
    assert col(m, "send_ack") == [0, 0, 0, 1, 0, 0, 1, 1]
    assert col(m, "send_report") == [0, 1, 1, 0, 1, 1, 0, 0]
    last_recv, last_input, last_report, flags, call = m["model"].fields()
    assert call[0] == 2 and flags[0] == 2 and last_recv[0] == T0 + 9200 and last_input[0] == T0 + 9200
    # the request first: the timeout raises nothing more
    m = host([T0, T0 + 16, T0 + 32, T0 + 2100, T0 + 2200], kinds=[1, 1, 1, 0, 1], events=[0, 1, 1, 0, 0])
    assert col(m, "net_events") == [0, D, 0, I, R] and m["model"].fields()[4][0] == 1
    # both at one call: one event
    m = host([T0, T0 + 2001], kinds=[0, 1], events=[0, 1])
    assert col(m, "net_events") == [0, D] and m["model"].fields()[4][0] == 1


def test_the_spectators_retry_timer_has_no_output_but_keeps_the_field():
    m = host([T0, T0 + 201, T0 + 300, T0 + 402], kinds=[0, 0, 0, 0])
    assert m["model"].fields()[1][0] == T0 + 402 and col(m, "send_ack") == [0, 0, 0, 0]
    assert set(m) == {"send_ack", "send_report", "net_events", "model"}
    # exactly 200 ms does not fire
    m = host([T0, T0 + 200], kinds=[0, 0])
    assert m["model"].fields()[1][0] == T0 and col(m, "send_report") == [0, 0]
    m = host([T0, T0 + 500, T0 + 2000], kinds=[0, 0, 0])
    assert col(m, "net_events") == [0, 0, I]  # 500 is not above notify, 2000 not above the timeout


def test_a_dropped_packet_is_no_decoded_input():
    now = np.array([T0, T0 + 100, T0 + 250], np.uint64)
    kinds = np.full((3, 1), M.K_INPUT, np.uint8)
    status = np.array([[1], [-3], [-3]], np.int32)
    m = M.run_host(1, 2000, 500, T0, now, kinds, np.zeros((3, 1), np.uint8), status=status)
    assert col(m, "send_ack") == [1, 0, 0] and m["model"].fields()[1][0] == T0 + 250  # (the retry reset it)
    assert m["model"].fields()[0][0] == T0 + 250  # a message all the same


# ---- hand-derived traces: the P2P engine's spectator endpoints

def test_a_link_that_receives_only_acks_raises_resend_whenever_200_ms_have_passed():
    t = [T0 + 67 * k for k in range(40)]
    m = link(t, kinds=[M.P.K_INPUT_ACK] * 40)
    fired = [k for k, v in enumerate(col(m, "resend")) if v]
    assert fired == [3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 33, 36, 39]  # 201 ms: every third call
    assert not any(col(m, "net_events"))
    # an Input bit counts as a message and nothing else: the retry recurs all the same
    m2 = link(t, kinds=[M.K_INPUT] * 40)
    assert col(m2, "resend") == col(m, "resend")
    # exactly 200 ms does not fire
    m = link([T0, T0 + 200, T0 + 201])
    assert col(m, "resend") == [0, 0, 1] and col(m, "send_report") == [0, 0, 1]


def test_close_in_closes_without_an_event_and_the_overflow_with_one():
    t = [T0, T0 + 16, T0 + 32, T0 + 5016, T0 + 5017, T0 + 5100]
    m = link(t, kinds=[1] * 6, close_in=[0, 1, 1, 0, 0, 0])
    assert col(m, "net_events") == [0, 0, 0, 0, SH, 0]
    state, *_, shutdown, flags, closed = m["model"].fields()
    assert state[0] == M.SHUTDOWN and closed[0] == 1 and shutdown[0] == T0 + 16 + 5000 and flags[0] == 0
    m = link(t, kinds=[1] * 6, overflow=[0, 1, 1, 1, 1, 1])
    assert col(m, "net_events") == [0, D, 0, 0, SH, 0]
    state, *_, shutdown, flags, closed = m["model"].fields()
    assert state[0] == M.SHUTDOWN and closed[0] == 1 and shutdown[0] == T0 + 16 + 5000 and flags[0] == 0
    # the timeout: interrupted, then the event, the flag set; the timers stop with Running
    m = link([T0, T0 + 501, T0 + 2001, T0 + 2300, T0 + 7001, T0 + 7002])
    assert col(m, "net_events") == [0, I, D, 0, 0, SH] and col(m, "resend") == [0, 1, 1, 0, 0, 0]
    assert m["model"].fields()[5][0] == 3 and m["model"].fields()[6][0] == 2


def test_no_keep_alive_is_ever_queued():
    rng = np.random.default_rng(0xB0B)
    total = 0
    for trial in range(20):
        n = 300
        step = rng.choice((0, 1, 8, 16, 100, 199, 200, 201, 250, 450), n)
        now = 7 + np.cumsum(step)
        kinds = rng.integers(0, 64, n).astype(np.uint8)
        kinds[rng.random(n) < (0.1, 0.5, 0.9)[trial % 3]] = 0
        sess, lnk = M.LiteralSpectatorSession(2000, 500, 7), M.LiteralSpectatorLink(2000, 500, 7)
        for c in range(n):
            q = sess.poll_remote_clients(c, int(now[c]), int(kinds[c]), rng.random() < 0.8, rng.random() < 0.01)[3]
            q += lnk.call(c, int(now[c]), int(kinds[c]), rng.random() < 0.002, False)[3]
            assert "KeepAlive" not in q
            for ep in (sess.host, lnk.ep):
                assert ep.last_send_time >= ep.running_last_quality_report
            total += len(q)
    assert total > 3000


def test_the_six_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "ggrs-mi355x", "src", "ffi.rs")).read()
    from ggrs_amd import _lib, p2p, spectator
    for mod, names in ((spectator, ("ggrs_spectator_set_endpoint_poll", "ggrs_spectator_poll_endpoints",
                                    "ggrs_spectator_read_endpoint_state")),
                       (p2p, ("ggrs_p2p_set_spectator_poll", "ggrs_p2p_poll_spectator_endpoints",
                              "ggrs_p2p_read_spectator_endpoint_state"))):
        src = open(mod.__file__).read()
        for name in names:
            assert re.search(r"^int %s\(" % name, header, re.M), name
            assert name in _lib.EXPORTS, name
            assert "L.%s.argtypes" % name in src, name
            assert re.search(r"pub fn %s\(" % name, ffi), name
    for method in ("set_endpoint_poll", "poll_endpoints", "endpoint_state"):
        assert callable(getattr(spectator.SpectatorEngine, method))
    for method in ("set_spectator_poll", "poll_spectator_endpoints", "spectator_endpoint_state"):
        assert callable(getattr(p2p.P2PEngine, method))
    assert "Not built: the spectator endpoints'" not in header
    assert re.search(r"^#define GGRS_ABI_VERSION 6\b", header, re.M)
