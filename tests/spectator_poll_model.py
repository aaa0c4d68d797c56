"""CPU models of the two spectator poll units (include/ggrs_amd.h "Spectator engine: endpoint poll" and
"Spectator endpoint poll"; csrc/spectator_poll.hip, p2p_spec_poll.hip over poll_device.h).

HostEndpoints: the lean model of the spectator engine's unit, the header's steps 1-4 over all sessions of
a call at once.  SpectatorEndpoints: the lean model of the P2P engine's spectator endpoints, steps 0-4
over all K * S endpoints (flat: endpoint k of session s is column k * S + s).  The GPU tests compare the
units with these.

LiteralSpectatorSession: SpectatorSession::poll_remote_clients and handle_event
(p2p_spectator_session.rs:133-156, :199-239) restated over tests/endpoint_poll_model.LiteralProtocol -- the
session only forwards Event::Disconnected, host.disconnect() is never called.
LiteralSpectatorLink: P2PSession's spectator branch of poll_remote_clients (p2p_session.rs:458-464),
handle_event's Event::Disconnected (:866-878) and disconnect_player (:506-509) over the same protocol,
with send_input's overflow event (protocol.rs:443-445) queued before the poll that drains it.  A spectator
sends no Input: an Input tag is handled as a message that decodes nothing (the reference would hit the
assert! of p2p_session.rs:882).  The host's own disconnect_player of an endpoint that already left Running
changes nothing here (the reference would restart its shutdown timer).

host_case / link_case: the clocks and classes the GPU tests and the CPU tests share, by column % 6 over
endpoint_poll_model.gpu_case's three clocks."""
import functools

import numpy as np

from tests import endpoint_poll_model as P
from tests.endpoint_poll_model import (DISCONNECTED, K_INPUT, NET_DISCONNECTED, NET_INTERRUPTED, NET_RESUMED,  # noqa: F401
                                       NET_SHUTDOWN, REPORT_MS, RETRY_MS, RUNNING, SHUTDOWN, SHUTDOWN_MS, U)

CASE_S, CASE_CALLS, CASE_TIMEOUT, CASE_NOTIFY, CASE_START = P.CASE_S, P.CASE_CALLS, P.CASE_TIMEOUT, P.CASE_NOTIFY, P.CASE_START
CLOCKS = P.CLOCKS


class HostEndpoints:
    """S spectators' host endpoints, every clock at `start`; step() is one call's poll of all of them."""

    def __init__(self, S, timeout, notify, start):
        assert notify <= timeout
        self.S, self.timeout, self.notify = S, U(timeout), U(notify)
        self.last_recv = np.full(S, start, U)
        self.last_input_recv = np.full(S, start, U)
        self.last_report = np.full(S, start, U)
        self.notify_sent = np.zeros(S, bool)
        self.event_sent = np.zeros(S, bool)
        self.disconnected_call = np.full(S, -1, np.int32)
        self.clock = U(start)

    def step(self, c, now, kinds, status, events):
        """kinds, events [S] uint8, status [S] int32 (the feed's row) or None -> (send_ack, send_report,
        net_events) [S] uint8."""
        now = max(U(now), self.clock)
        self.clock = now
        net = np.zeros(self.S, np.uint8)
        got = kinds != 0                                                             # 1.
        self.last_recv[got] = now
        resumed = got & self.notify_sent
        self.notify_sent[resumed] = False
        net[resumed] |= NET_RESUMED
        requested = (events != 0) & ~self.event_sent                                 # 2.
        decoded = (kinds & K_INPUT) != 0                                             # 3.
        if status is not None:
            decoded &= status >= 0
        self.last_input_recv[decoded] = now
        retry = self.last_input_recv + U(RETRY_MS) < now                             # 4. (a)
        self.last_input_recv[retry] = now
        report = self.last_report + U(REPORT_MS) < now                               # (b)
        self.last_report[report] = now
        interrupted = ~self.notify_sent & (self.last_recv + self.notify < now)       # (c)
        self.notify_sent[interrupted] = True
        net[interrupted] |= NET_INTERRUPTED
        timed_out = ~self.event_sent & ~requested & (self.last_recv + self.timeout < now)  # (d)
        gone = requested | timed_out
        self.event_sent[gone] = True
        self.disconnected_call[gone] = c
        net[gone] |= NET_DISCONNECTED
        return decoded.astype(np.uint8), report.astype(np.uint8), net

    def fields(self):
        """read_endpoint_state's tuple."""
        flags = self.notify_sent.astype(np.int32) | self.event_sent.astype(np.int32) << 1
        return (self.last_recv.copy(), self.last_input_recv.copy(), self.last_report.copy(), flags,
                self.disconnected_call.copy())


HOST_NAMES = ("send_ack", "send_report", "net_events")


def run_host(S, timeout, notify, start, now, kinds, events, status=None, first_call=0, model=None):
    """-> dict of [n][S] uint8 arrays send_ack, send_report, net_events, and the model."""
    m = model or HostEndpoints(S, timeout, notify, start)
    n = len(now)
    out = {k: np.zeros((n, S), np.uint8) for k in HOST_NAMES}
    for k in range(n):
        r = m.step(first_call + k, now[k], kinds[k], None if status is None else status[k], events[k])
        for name, row in zip(HOST_NAMES, r):
            out[name][k] = row
    out["model"] = m
    return out


class SpectatorEndpoints:
    """E = K * S spectator endpoints of a P2P engine, flat; step() is one call's poll of all of them."""

    def __init__(self, E, timeout, notify, start):
        assert notify <= timeout
        self.E, self.timeout, self.notify = E, U(timeout), U(notify)
        self.last_recv = np.full(E, start, U)
        self.last_input_recv = np.full(E, start, U)
        self.last_report = np.full(E, start, U)
        self.shutdown = np.full(E, start, U)
        self.state = np.zeros(E, np.int32)
        self.notify_sent = np.zeros(E, bool)
        self.event_sent = np.zeros(E, bool)
        self.closed_call = np.full(E, -1, np.int32)
        self.clock = U(start)

    def step(self, c, now, kinds, close_in, overflow):
        """kinds, close_in [E] uint8, overflow [E] bool (spectator emit closed the endpoint with
        GGRS_EMIT_DISCONNECTED before this poll) -> (resend, send_report, net_events) [E] uint8."""
        now = max(U(now), self.clock)
        self.clock = now
        entry = self.state.copy()
        alive = entry != SHUTDOWN                                                    # 0.
        running = entry == RUNNING
        net = np.zeros(self.E, np.uint8)
        got = alive & (kinds != 0)                                                   # 1.
        self.last_recv[got] = now
        resumed = got & self.notify_sent & running
        self.notify_sent[resumed] = False
        net[resumed] |= NET_RESUMED
        resend = running & (self.last_input_recv + U(RETRY_MS) < now)                # 3. (a)
        self.last_input_recv[resend] = now
        report = running & (self.last_report + U(REPORT_MS) < now)                   # (b)
        self.last_report[report] = now
        interrupted = running & ~self.notify_sent & (self.last_recv + self.notify < now)  # (c)
        self.notify_sent[interrupted] = True
        net[interrupted] |= NET_INTERRUPTED
        over = running & overflow                                                    # 2. (the queued event)
        net[over] |= NET_DISCONNECTED
        timed_out = running & ~self.event_sent & (self.last_recv + self.timeout < now)  # (d)
        self.event_sent[timed_out] = True
        net[timed_out] |= NET_DISCONNECTED
        closing = running & ((close_in != 0) | over | timed_out)                     # (e)
        self.state[closing] = DISCONNECTED
        self.shutdown[closing] = now + U(SHUTDOWN_MS)
        self.closed_call[closing] = c
        down = (entry == DISCONNECTED) & (self.shutdown < now)                       # 4.
        self.state[down] = SHUTDOWN
        net[down] |= NET_SHUTDOWN
        return resend.astype(np.uint8), report.astype(np.uint8), net

    def fields(self):
        """read_spectator_endpoint_state's tuple, flat."""
        flags = self.notify_sent.astype(np.int32) | self.event_sent.astype(np.int32) << 1
        return (self.state.copy(), self.last_recv.copy(), self.last_input_recv.copy(), self.last_report.copy(),
                self.shutdown.copy(), flags, self.closed_call.copy())


LINK_NAMES = ("resend", "send_report", "net_events")


def run_links(E, timeout, notify, start, now, kinds, close_in, overflow=None, first_call=0, model=None):
    """now [n], kinds, close_in [n][E] uint8, overflow [n][E] bool or None -> dict of [n][E] uint8 arrays
    resend, send_report, net_events, and the model."""
    m = model or SpectatorEndpoints(E, timeout, notify, start)
    n = len(now)
    out = {k: np.zeros((n, E), np.uint8) for k in LINK_NAMES}
    none = np.zeros(E, bool)
    for k in range(n):
        r = m.step(first_call + k, now[k], kinds[k], close_in[k], none if overflow is None else overflow[k])
        for name, row in zip(LINK_NAMES, r):
            out[name][k] = row
    out["model"] = m
    return out


# ---- the literal restatements

class LiteralSpectatorSession:
    """One SpectatorSession's network side: its host endpoint and its GgrsEvent queue."""

    def __init__(self, timeout, notify, start):
        self.host = P.LiteralProtocol(timeout, notify, start)
        self.event_queue = []
        self.disconnected_call = -1

    def handle_event(self, event, c):                          # :199-239
        name, _ = event
        self.event_queue.append(name)                          # forward to user, nothing else
        if name == "Disconnected":
            self.disconnected_call = c

    def poll_remote_clients(self, c, now, kinds, decodes, disconnect_requested):  # :133-156
        """-> (send_ack, send_report, net_events, the messages queued)."""
        h = self.host
        h.clock = max(now, h.clock)
        for t in range(6):
            if kinds >> t & 1:
                h.handle_message(1 << t, decodes, disconnect_requested and (1 << t) == K_INPUT)
        first = len(self.event_queue)
        for event in h.poll():
            self.handle_event(event, c)
        queued = h.send_all_messages()
        net = 0
        for name in self.event_queue[first:]:
            net |= {"NetworkInterrupted": NET_INTERRUPTED, "NetworkResumed": NET_RESUMED, "Disconnected": NET_DISCONNECTED}[name]
        return int("InputAck" in queued), int("QualityReport" in queued), net, queued

    def fields(self):
        f = self.host.fields()
        return (f[1], f[2], f[3], f[5], self.disconnected_call)


class LiteralSpectatorLink:
    """One spectator endpoint of a P2PSession."""

    def __init__(self, timeout, notify, start):
        self.ep = P.LiteralProtocol(timeout, notify, start)
        self.ep.pending_output = True  # (confirmed inputs are pending: the retry has something to send)
        self.events = []
        self.closed_call = -1

    def disconnect_player(self, c):                            # :506-509 -> :645-652
        if self.ep.state == RUNNING:
            self.closed_call = c
            self.ep.disconnect()

    def call(self, c, now, kinds, close_in, overflow_queued):
        """-> (resend, send_report, net_events, the messages queued)."""
        ep = self.ep
        ep.clock = max(now, ep.clock)
        ep.retry_fired = ep.shut_down_now = False
        if overflow_queued and ep.state == RUNNING:            # send_input's, at the call before (protocol.rs:443-445)
            ep.event_queue.append(("Disconnected", "overflow"))
        for t in range(6):
            if kinds >> t & 1:
                ep.handle_message(1 << t, decodes=False)
        net = 0
        for name, _ in ep.poll():                              # p2p_session.rs:458-464, handle_event :866-878
            self.events.append(name)
            if name == "NetworkInterrupted":
                net |= NET_INTERRUPTED
            elif name == "NetworkResumed":
                net |= NET_RESUMED
            else:
                net |= NET_DISCONNECTED
                self.disconnect_player(c)
        if close_in:                                           # the host's own, no event
            self.disconnect_player(c)
        if ep.shut_down_now:
            net |= NET_SHUTDOWN
        queued = list(ep.send_queue)
        ep.send_all_messages()
        return int(ep.retry_fired), int("QualityReport" in queued), net, queued

    def fields(self):
        return self.ep.fields() + (self.closed_call,)


# ---- the cases the GPU tests run (S = 130, 200 calls, timeout 640 ms, notify 160 ms)

def host_case(kind, S=CASE_S, calls=CASE_CALLS):
    """(now [calls] uint64, kinds, events [calls][S] uint8) for the spectator engine: gpu_case's, whose
    class-4 events bytes stand for an accepted Input's disconnect_requested (a second one follows)."""
    return P.gpu_case(kind, S, calls)


@functools.lru_cache(maxsize=None)
def link_case(kind, K, S=CASE_S, calls=CASE_CALLS, overflow=False):
    """(now, kinds [calls][K * S], close_in [calls][K * S] uint8, overflow [calls][K * S] bool) for the P2P
    side: gpu_case over K * S columns, class by column % 6.  Class 4 is closed by close_in -- with
    overflow=True every second endpoint of it by an emit overflow instead, seen from the call of its
    events byte on."""
    now, kinds, events = P.gpu_case(kind, K * S, calls)
    close_in = (events != 0).astype(np.uint8)
    over = np.zeros((calls, K * S), bool)
    if overflow:
        for e in range(4, K * S, 12):
            first = int(np.argmax(close_in[:, e] != 0))
            close_in[:, e] = 0
            over[first:, e] = True
    return now, kinds, close_in, over


def host_run(kind, status=None):
    now, kinds, events = host_case(kind)
    return run_host(CASE_S, CASE_TIMEOUT, CASE_NOTIFY, CASE_START, now, kinds, events, status=status)


def link_run(kind, K, overflow=False):
    now, kinds, close_in, over = link_case(kind, K, overflow=overflow)
    return run_links(K * CASE_S, CASE_TIMEOUT, CASE_NOTIFY, CASE_START, now, kinds, close_in, over)


def count(net, bit):
    return ((net & bit) != 0).sum(axis=0)


def assert_host_case_is_not_vacuous(kind, m):
    """Every class raises what it must under clock `kind` (m: run_host()'s result)."""
    cls = np.arange(m["net_events"].shape[1]) % 6
    net = m["net_events"]
    assert not (net & NET_SHUTDOWN).any()
    assert (count(net, NET_DISCONNECTED) <= 1).all()
    assert (m["model"].disconnected_call >= 0).tolist() == (count(net, NET_DISCONNECTED) == 1).tolist()
    # class 0: a report whenever 200 ms have passed, an ack at every call, and nothing else
    assert m["send_report"].any(axis=0)[cls == 0].all() and m["send_ack"][:, cls == 0].all() and not net[:, cls == 0].any()
    assert not net[:, cls == 1].any() and m["send_ack"].any(axis=0)[cls == 1].all()
    # class 2: INTERRUPTED then RESUMED, twice, and nothing else
    two = net[:, cls == 2]
    assert (count(two, NET_INTERRUPTED) == 2).all() and (count(two, NET_RESUMED) == 2).all() and not (two & NET_DISCONNECTED).any()
    # class 3: INTERRUPTED, the timeout's DISCONNECTED, and RESUMED when the messages come back: still Running
    three = net[:, cls == 3]
    assert (count(three, NET_INTERRUPTED) >= 1).all() and (count(three, NET_DISCONNECTED) == 1).all()
    assert (count(three, NET_RESUMED) >= 1).all()
    assert m["send_ack"][-1, cls == 3].all()
    # class 4: the request's DISCONNECTED, once; acks and reports go on
    four = net[:, cls == 4]
    assert (count(four, NET_DISCONNECTED) == 1).all() and not (four & (NET_INTERRUPTED | NET_RESUMED)).any()
    assert m["send_ack"][-1, cls == 4].all()
    # class 5: no Input, so no ack; the link is never silent
    assert not m["send_ack"][:, cls == 5].any() and not net[:, cls == 5].any()


def assert_link_case_is_not_vacuous(kind, m, overflow=False):
    """The same for the P2P side (m: run_links()'s result)."""
    E = m["net_events"].shape[1]
    cls = np.arange(E) % 6
    net = m["net_events"]
    mod = m["model"]
    assert not net[:, cls == 0].any()
    # no Input ever resets the retry: every endpoint that stays Running keeps raising resend
    assert (m["resend"][:, cls == 0].sum(axis=0) >= 2).all() and m["send_report"].any(axis=0)[cls <= 2].all()
    assert not net[:, cls == 1].any()
    two = net[:, cls == 2]
    assert (count(two, NET_INTERRUPTED) == 2).all() and (count(two, NET_RESUMED) == 2).all()
    assert not (two & (NET_DISCONNECTED | NET_SHUTDOWN)).any()
    three = net[:, cls == 3]
    assert (count(three, NET_INTERRUPTED) == 1).all() and (count(three, NET_DISCONNECTED) == 1).all()
    assert not (three & NET_RESUMED).any() and (mod.closed_call[cls == 3] >= 0).all()
    over = np.zeros(E, bool)
    if overflow:
        over[4::12] = True
    four = (cls == 4) & ~over
    assert not (net[:, four] & NET_DISCONNECTED).any() and (mod.closed_call[four] >= 0).all()  # close_in: no event
    assert not mod.event_sent[cls == 4].any()
    if overflow:
        assert over.sum() >= 10 and (count(net[:, over], NET_DISCONNECTED) == 1).all() and (mod.closed_call[over] >= 0).all()
    assert not net[:, cls == 5].any() and (mod.closed_call[cls == 5] == -1).all()
    gone = (cls == 3) | (cls == 4)
    if kind != "const8":
        assert (count(net[:, gone], NET_SHUTDOWN) == 1).all() and (mod.state[gone] == SHUTDOWN).all()
    else:
        assert (mod.state[gone] == DISCONNECTED).all()
    # a closed endpoint raises no resend and no report afterwards
    for e in np.nonzero(gone)[0][:20]:
        c = mod.closed_call[e]
        assert not m["resend"][c + 1:, e].any() and not m["send_report"][c + 1:, e].any()
