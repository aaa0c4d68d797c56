"""The endpoint poll on the CPU (tests/endpoint_poll_model.py): the lean model against a literal
restatement of UdpProtocol's poll / handle_message / queue_message / disconnect on the GPU tests' own
inputs, the unreachable send_keep_alive, hand-derived traces, and the header / binding check."""
import os
import re

import numpy as np
import pytest

from tests import endpoint_poll_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = M.CASE_START


def literal_run(now, kinds, events, status, rmask, timeout, notify, start, sends=None, on_call=None):
    """The literal model over [n][S] inputs -> run()'s arrays, every queued message, the endpoints."""
    n, S = kinds.shape
    eps = [M.LiteralProtocol(timeout, notify, start) for _ in range(S)]
    closed = np.full(S, -1, np.int32)
    out = {k: np.zeros((n, S), np.uint8) for k in ("resend", "send_ack", "send_report", "net_events")}
    queued = []
    for c in range(n):
        for s, ep in enumerate(eps):
            decodes = status is None or status[c, s] >= 0
            r = ep.call(c, int(now[c]), int(kinds[c, s]), decodes, bool(events[c, s] & rmask),
                        True if sends is None else bool(sends[c, s]))
            for name, v in zip(("resend", "send_ack", "send_report", "net_events"), r):
                out[name][c, s] = v
            if r[4]:
                closed[s] = c
            queued += r[5]
        if on_call:
            on_call(c, eps, closed)
    return out, queued, eps, closed


@pytest.mark.parametrize("feed", (False, True))
@pytest.mark.parametrize("kind", M.CLOCKS)
def test_the_two_models_agree_after_every_call_on_the_gpu_cases(kind, feed):
    now, kinds, events = M.gpu_case(kind)
    rng = np.random.default_rng(5)
    status = np.where(rng.random(kinds.shape) < 0.2, -3, 1).astype(np.int32) if feed else None
    sends = rng.random(kinds.shape) < 0.7
    lean = M.Endpoints(M.CASE_S, M.CASE_TIMEOUT, M.CASE_NOTIFY, T0, M.CASE_RMASK)
    rows = {}

    def after(c, eps, closed):
        rows[c] = lean.step(c, now[c], kinds[c], None if status is None else status[c], events[c])
        got = lean.fields()
        want = list(zip(*(ep.fields() for ep in eps)))
        for g, w in zip(got[:6], want):
            assert (g.astype(np.int64) == np.array(w, np.uint64).astype(np.int64)).all(), c
        assert (got[6] == closed).all(), c

    lit, queued, eps, closed = literal_run(now, kinds, events, status, M.CASE_RMASK, M.CASE_TIMEOUT, M.CASE_NOTIFY, T0,
                                           sends, after)
    for i, name in enumerate(("resend", "send_ack", "send_report", "net_events")):
        got = np.stack([rows[c][i] for c in range(len(now))])
        assert (got == lit[name]).all(), (name, np.argwhere(got != lit[name])[:5])
    assert "KeepAlive" not in queued and "QualityReport" in queued and "InputAck" in queued


@pytest.mark.parametrize("kind", M.CLOCKS)
def test_every_class_raises_what_it_must(kind):
    M.assert_case_is_not_vacuous(kind, M.case_run(kind))


def test_the_literal_model_never_queues_a_keep_alive():
    """Random clocks (steps of 0 .. 450 ms around every threshold, exactly 200 among them), random
    traffic, calls that send an Input and calls that do not, pending output or none: poll's third
    branch never runs, because last_send_time >= running_last_quality_report at every check."""
    rng = np.random.default_rng(0xA11CE)
    total = 0
    for trial in range(40):
        n, S = 300, 8
        step = rng.choice((0, 1, 8, 16, 100, 199, 200, 201, 250, 450), n)
        now = 7 + np.cumsum(step)
        kinds = rng.integers(0, 64, (n, S)).astype(np.uint8)
        kinds[rng.random((n, S)) < (0.1, 0.5, 0.9)[trial % 3]] = 0
        events = (rng.random((n, S)) < 0.002).astype(np.uint8) * 2
        sends = rng.random((n, S)) < (0.0, 0.5, 1.0)[trial // 3 % 3]
        status = np.where(rng.random((n, S)) < 0.3, -1, 0).astype(np.int32)
        checks = []

        def after(c, eps, closed):
            checks.extend(ep.last_send_time >= ep.running_last_quality_report for ep in eps)

        lit, queued, eps, closed = literal_run(now, kinds, events, status, 2, 2000, 500, 7, sends, after)
        assert "KeepAlive" not in queued and all(checks)
        total += len(queued)
    assert total > 10000


def silent(clocks, timeout=2000, notify=500, kinds=None, events=None):
    n = len(clocks)
    k = np.zeros((n, 1), np.uint8) if kinds is None else np.array(kinds, np.uint8)[:, None]
    e = np.zeros((n, 1), np.uint8) if events is None else np.array(events, np.uint8)[:, None]
    return M.run(1, timeout, notify, T0, 2, np.array(clocks, np.uint64), k, e)


def col(m, name):
    return m[name][:, 0].tolist()


def test_hand_derived_traces_of_a_silent_link():
    """start_ms = t0, silence throughout, the reference's defaults (2000, 500)."""
    t = [T0, T0 + 200, T0 + 201, T0 + 401, T0 + 402, T0 + 500, T0 + 501, T0 + 2000, T0 + 2001, T0 + 7001, T0 + 7002,
         T0 + 9000]
    m = silent(t)
    #                            t0  200 201 401 402 500 501 2000 2001 7001 7002 9000
    assert col(m, "resend") == [0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0]      # 201: first above t0 + 200; then 402, 603..
    assert col(m, "send_report") == [0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0]
    assert col(m, "send_ack") == [0] * 12
    assert col(m, "net_events") == [0, 0, 0, 0, 0, 0, M.NET_INTERRUPTED, 0, M.NET_DISCONNECTED, 0, M.NET_SHUTDOWN, 0]
    assert col(m, "events") == [0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0]       # the remote player's bit, at the timeout's call
    state, last_recv, last_input, last_report, shutdown, flags, closed = m["model"].fields()
    assert state[0] == M.SHUTDOWN and closed[0] == 8 and shutdown[0] == T0 + 2001 + 5000 and flags[0] == 3
    assert last_recv[0] == T0 and last_input[0] == T0 + 2000 and last_report[0] == T0 + 2000
    # the retry fires at 2001 as well when the timers were not reset at 2000
    m = silent([T0, T0 + 2001])
    assert col(m, "resend") == [0, 1] and col(m, "send_report") == [0, 1]
    assert col(m, "net_events") == [0, M.NET_INTERRUPTED | M.NET_DISCONNECTED]


def test_a_message_resumes_once_and_the_interruption_can_recur():
    t = [T0, T0 + 501, T0 + 600, T0 + 700, T0 + 1201, T0 + 1300, T0 + 1400]
    m = silent(t, kinds=[0, 0, M.K_KEEP_ALIVE, 0, 0, M.K_INPUT, M.K_INPUT])
    assert col(m, "net_events") == [0, M.NET_INTERRUPTED, M.NET_RESUMED, 0, M.NET_INTERRUPTED, M.NET_RESUMED, 0]
    assert col(m, "send_ack") == [0, 0, 0, 0, 0, 1, 1]
    assert m["model"].fields()[0][0] == M.RUNNING and m["model"].fields()[5][0] == 0


def test_a_message_while_disconnected_is_acknowledged_and_resumes_nothing():
    t = [T0, T0 + 501, T0 + 2001, T0 + 2100, T0 + 2200, T0 + 7001, T0 + 7002, T0 + 7100]
    m = silent(t, kinds=[0, 0, 0, M.K_INPUT, M.K_INPUT_ACK, M.K_INPUT, M.K_INPUT, M.K_INPUT])
    assert col(m, "net_events") == [0, M.NET_INTERRUPTED, M.NET_DISCONNECTED, 0, 0, 0, M.NET_SHUTDOWN, 0]
    assert col(m, "send_ack") == [0, 0, 0, 1, 0, 1, 1, 0]   # acks keep flowing until Shutdown; then nothing
    assert col(m, "resend") == [0, 1, 1, 0, 0, 0, 0, 0]     # the timers stop with Running
    state, last_recv, *_ = m["model"].fields()
    assert state[0] == M.SHUTDOWN and last_recv[0] == T0 + 7002


def test_a_disconnect_request_closes_without_the_timeouts_event():
    m = silent([T0, T0 + 16, T0 + 32, T0 + 5016, T0 + 5017], events=[0, 2, 2, 0, 0], kinds=[1, 1, 1, 1, 1])
    assert col(m, "net_events") == [0, 0, 0, 0, M.NET_SHUTDOWN]
    state, *_, shutdown, flags, closed = m["model"].fields()
    assert closed[0] == 1 and shutdown[0] == T0 + 16 + 5000 and flags[0] == 2  # the second request changes nothing


def test_exactly_the_interval_does_not_fire_and_the_clock_never_goes_back():
    m = silent([T0 + 8 * k for k in range(60)])
    fired = [k for k, v in enumerate(col(m, "resend")) if v]
    assert fired == [26, 52]  # 208 ms: the first clock above 200, then 208 ms after that
    m = silent([T0, T0 + 300, T0 + 100, T0 + 501])
    assert col(m, "resend") == [0, 1, 0, 1] and m["model"].clock == T0 + 501  # 100 is taken as 300
    m2 = silent([T0 + (1 << 32) - 1, T0 + (1 << 32) + 200, T0 + (1 << 32) + 300], timeout=1 << 40, notify=1 << 40)
    assert col(m2, "resend") == [1, 1, 0]  # 64-bit times: nothing wraps at 2^32


def test_the_three_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "ggrs_amd.h")).read()
    from ggrs_amd import _lib, p2p
    src = open(p2p.__file__).read()
    for name in ("ggrs_p2p_set_endpoint_poll", "ggrs_p2p_poll_endpoints", "ggrs_p2p_read_endpoint_state"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTS, name
        assert "L.%s.argtypes" % name in src, name
    for name, value in (("GGRS_NET_INTERRUPTED", 1), ("GGRS_NET_RESUMED", 2), ("GGRS_NET_DISCONNECTED", 4),
                        ("GGRS_NET_SHUTDOWN", 8), ("GGRS_ENDPOINT_RUNNING", 0), ("GGRS_ENDPOINT_DISCONNECTED", 1),
                        ("GGRS_ENDPOINT_SHUTDOWN", 2)):
        assert re.search(r"^#define %s\s+%d\b" % (name, value), header, re.M), name
        assert getattr(_lib, name) == value
    for method in ("set_endpoint_poll", "poll_endpoints", "endpoint_state"):
        assert callable(getattr(p2p.P2PEngine, method))
    assert (M.NET_INTERRUPTED, M.NET_RESUMED, M.NET_DISCONNECTED, M.NET_SHUTDOWN) == (1, 2, 4, 8)
    # the two sentences that left these decisions with the host are gone
    assert "timer stays with the host" not in header and "NetworkResumed and the disconnect timeouts. */" not in header
