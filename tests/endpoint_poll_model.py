"""CPU models of the endpoint poll (include/ggrs_amd.h "Endpoint poll"; csrc/p2p_poll.hip, poll_device.h).

Endpoints: the lean model, the header's steps 0-5 over all sessions of a call at once -- what the GPU
tests compare the unit with.

LiteralProtocol: UdpProtocol's poll, handle_message, on_input's clock and ack, queue_message,
send_quality_report, send_keep_alive and disconnect (src/network/protocol.rs:311-376, :497-562, :608,
:634) restated line for line for one endpoint, with last_send_time and a send queue, over the unit's
one clock per poll.  It shows that the lean model left nothing out (the two agree event for event and
field for field) and that send_keep_alive never fires.  A remote player's bit in the events byte is
taken as a received disconnect_requested (on_input, :569-574), which is what sets
disconnect_event_sent; the host's own disconnect_player would call disconnect() without it -- the
unit cannot tell the two apart and the flag is read by nobody once the endpoint left Running.

gpu_case: the clocks and session classes the GPU tests and the CPU tests share."""
import functools

import numpy as np

RETRY_MS = REPORT_MS = KEEP_ALIVE_MS = 200  # RUNNING_RETRY_INTERVAL, QUALITY_REPORT_INTERVAL, KEEP_ALIVE_INTERVAL
SHUTDOWN_MS = 5000                          # UDP_SHUTDOWN_TIMER
RUNNING, DISCONNECTED, SHUTDOWN = 0, 1, 2
NET_INTERRUPTED, NET_RESUMED, NET_DISCONNECTED, NET_SHUTDOWN = 1, 2, 4, 8
K_INPUT, K_INPUT_ACK, K_QUALITY_REPORT, K_QUALITY_REPLY, K_CHECKSUM_REPORT, K_KEEP_ALIVE = (1 << t for t in range(6))
U = np.uint64


class Endpoints:
    """S endpoints, every clock at `start`; step() is one call's poll of all of them."""

    def __init__(self, S, timeout, notify, start, rmask):
        assert notify <= timeout
        self.S, self.timeout, self.notify, self.rmask = S, U(timeout), U(notify), rmask
        self.last_recv = np.full(S, start, U)
        self.last_input_recv = np.full(S, start, U)
        self.last_report = np.full(S, start, U)
        self.shutdown = np.full(S, start, U)
        self.state = np.zeros(S, np.int32)
        self.notify_sent = np.zeros(S, bool)
        self.event_sent = np.zeros(S, bool)
        self.closed_call = np.full(S, -1, np.int32)
        self.clock = U(start)

    def step(self, c, now, kinds, status, events):
        """kinds [S] uint8, status [S] int32 (the feed's row) or None, events [S] uint8 (the call's
        stored byte) -> (resend, send_ack, send_report, net_events, events after the poll) [S] uint8."""
        now = max(U(now), self.clock)  # an Instant never goes back
        self.clock = now
        entry = self.state.copy()
        alive = entry != SHUTDOWN                                                   # 0.
        running = entry == RUNNING
        net = np.zeros(self.S, np.uint8)
        got = alive & (kinds != 0)                                                  # 1.
        self.last_recv[got] = now
        resumed = got & self.notify_sent & running
        self.notify_sent[resumed] = False
        net[resumed] |= NET_RESUMED
        decoded = alive & ((kinds & K_INPUT) != 0)                                  # 2.
        if status is not None:
            decoded &= status >= 0
        self.last_input_recv[decoded] = now
        ack = decoded.copy()
        ext = (events & self.rmask) != 0                                            # 3.
        resend = running & (self.last_input_recv + U(RETRY_MS) < now)               # 4. (a)
        self.last_input_recv[resend] = now
        report = running & (self.last_report + U(REPORT_MS) < now)                  # (b)
        self.last_report[report] = now
        interrupted = running & ~self.notify_sent & (self.last_recv + self.notify < now)  # (c)
        self.notify_sent[interrupted] = True
        net[interrupted] |= NET_INTERRUPTED
        self.event_sent[running & ext] = True                                       # (d)
        timed_out = running & ~self.event_sent & (self.last_recv + self.timeout < now)
        self.event_sent[timed_out] = True
        net[timed_out] |= NET_DISCONNECTED
        events = events.copy()
        events[timed_out] |= self.rmask
        closing = running & (ext | timed_out)                                       # (e)
        self.state[closing] = DISCONNECTED
        self.shutdown[closing] = now + U(SHUTDOWN_MS)
        self.closed_call[closing] = c
        down = (entry == DISCONNECTED) & (self.shutdown < now)                      # 5.
        self.state[down] = SHUTDOWN
        net[down] |= NET_SHUTDOWN
        return resend.astype(np.uint8), ack.astype(np.uint8), report.astype(np.uint8), net, events

    def fields(self):
        """read_endpoint_state's tuple."""
        flags = self.notify_sent.astype(np.int32) | self.event_sent.astype(np.int32) << 1
        return (self.state.copy(), self.last_recv.copy(), self.last_input_recv.copy(), self.last_report.copy(),
                self.shutdown.copy(), flags, self.closed_call.copy())


def run(S, timeout, notify, start, rmask, now, kinds, events, status=None, first_call=0, model=None):
    """Calls first_call .. of a (new) Endpoints over now [n], kinds [n][S], events [n][S], status [n][S]
    or None -> dict of [n][S] uint8 arrays resend, send_ack, send_report, net_events, events, and the
    model (its fields() is the final state)."""
    m = model or Endpoints(S, timeout, notify, start, rmask)
    n = len(now)
    out = {k: np.zeros((n, S), np.uint8) for k in ("resend", "send_ack", "send_report", "net_events", "events")}
    for k in range(n):
        r = m.step(first_call + k, now[k], kinds[k], None if status is None else status[k], events[k])
        for name, row in zip(("resend", "send_ack", "send_report", "net_events", "events"), r):
            out[name][k] = row
    out["model"] = m
    return out


class LiteralProtocol:
    """One UdpProtocol, its send side reduced to what queue_message is called with."""

    def __init__(self, timeout, notify, start):
        self.clock = start
        self.send_queue, self.event_queue = [], []
        self.state = RUNNING                                   # :218
        self.running_last_quality_report = self.instant_now()  # :219
        self.running_last_input_recv = self.instant_now()      # :220
        self.disconnect_notify_sent = False
        self.disconnect_event_sent = False
        self.disconnect_timeout, self.disconnect_notify_start = timeout, notify
        self.shutdown_timeout = self.instant_now()             # :227
        self.last_send_time = self.instant_now()               # :251
        self.last_recv_time = self.instant_now()               # :252
        self.pending_output = False
        self.retry_fired = self.shut_down_now = False

    def instant_now(self):
        return self.clock

    def queue_message(self, body):                             # :515-528
        self.last_send_time = self.instant_now()
        self.send_queue.append(body)

    def send_pending_output(self):                             # :450-: an Input when anything is pending
        self.retry_fired = True
        if self.pending_output:
            self.queue_message("Input")

    def send_input_ack(self):
        self.queue_message("InputAck")

    def send_keep_alive(self):                                 # :497-499
        self.queue_message("KeepAlive")

    def send_quality_report(self):                             # :501-513
        self.running_last_quality_report = self.instant_now()
        self.queue_message("QualityReport")

    def disconnect(self):                                      # :311-319
        if self.state == SHUTDOWN:
            return
        self.state = DISCONNECTED
        self.shutdown_timeout = self.instant_now() + SHUTDOWN_MS

    def poll(self):                                            # :329-376
        now = self.instant_now()
        if self.state == RUNNING:
            if self.running_last_input_recv + RETRY_MS < now:
                self.send_pending_output()
                self.running_last_input_recv = self.instant_now()
            if self.running_last_quality_report + REPORT_MS < now:
                self.send_quality_report()
            if self.last_send_time + KEEP_ALIVE_MS < now:
                self.send_keep_alive()
            if not self.disconnect_notify_sent and self.last_recv_time + self.disconnect_notify_start < now:
                self.event_queue.append(("NetworkInterrupted", self.disconnect_timeout - self.disconnect_notify_start))
                self.disconnect_notify_sent = True
            if not self.disconnect_event_sent and self.last_recv_time + self.disconnect_timeout < now:
                self.event_queue.append(("Disconnected", "timeout"))
                self.disconnect_event_sent = True
        elif self.state == DISCONNECTED:
            if self.shutdown_timeout < self.instant_now():
                self.state = SHUTDOWN
                self.shut_down_now = True
        drained, self.event_queue = self.event_queue, []
        return drained

    def handle_message(self, tag, decodes=True, disconnect_requested=False):  # :534-562
        if self.state == SHUTDOWN:
            return
        self.last_recv_time = self.instant_now()
        if self.disconnect_notify_sent and self.state == RUNNING:
            self.disconnect_notify_sent = False
            self.event_queue.append(("NetworkResumed", None))
        if tag == K_INPUT:
            self.on_input(decodes, disconnect_requested)
        elif tag == K_QUALITY_REPORT:                          # on_quality_report, :649-653
            self.queue_message("QualityReply")

    def on_input(self, decodes, disconnect_requested):         # :564-641
        if disconnect_requested:
            self.disconnect_request()
        if decodes:
            self.running_last_input_recv = self.instant_now()  # :608
            self.send_input_ack()                              # :634

    def disconnect_request(self):                              # :569-574
        if self.state == SHUTDOWN:                             # (handle_message returned, :538-541)
            return
        if self.state != DISCONNECTED and not self.disconnect_event_sent:
            self.event_queue.append(("Disconnected", "requested"))
            self.disconnect_event_sent = True

    def send_all_messages(self):                               # :397-407
        sent, self.send_queue = self.send_queue, []
        return [] if self.state == SHUTDOWN else sent

    def call(self, c, now, kinds, decodes, ext, sends_input):
        """Call c of the session that owns the endpoint: the messages of its poll (kinds' bits in tag
        order), a disconnect request when ext, poll() and its events handled
        (disconnect_player_at_frame calls disconnect), then advance_frame's send_input when the call
        queued a frame.  -> (resend, send_ack, send_report, net_events, whether the endpoint closed at
        this call, every message queued during the call -- before send_all_messages drops a shut-down
        endpoint's)."""
        self.clock = max(now, self.clock)
        self.retry_fired = self.shut_down_now = False
        for t in range(6):
            if kinds >> t & 1:
                self.handle_message(1 << t, decodes)
        if ext:
            self.disconnect_request()
        net = 0
        closed = False
        for name, why in self.poll():
            if name == "NetworkInterrupted":
                net |= NET_INTERRUPTED
            elif name == "NetworkResumed":
                net |= NET_RESUMED
            elif name == "Disconnected":
                if why == "timeout":
                    net |= NET_DISCONNECTED
                self.disconnect()
                closed = True
        if self.shut_down_now:
            net |= NET_SHUTDOWN
        polled = list(self.send_queue)
        if sends_input and self.state == RUNNING:              # send_input, :417-448
            self.pending_output = True
            self.queue_message("Input")
        queued = list(self.send_queue)
        self.send_all_messages()
        return int(self.retry_fired), int("InputAck" in polled), int("QualityReport" in polled), net, closed, queued

    def fields(self):
        return (self.state, self.last_recv_time, self.running_last_input_recv, self.running_last_quality_report,
                self.shutdown_timeout, int(self.disconnect_notify_sent) | int(self.disconnect_event_sent) << 1)


# ---- the cases the GPU tests run (S = 130, 200 calls, timeout 640 ms, notify 160 ms)

CASE_S, CASE_CALLS, CASE_TIMEOUT, CASE_NOTIFY = 130, 200, 640, 160
CASE_START = 3 * (1 << 32) - 1000  # the clock crosses a multiple of 2^32
CASE_RMASK = 0b10                  # players (local 0, remote 1)
CLOCKS = ("jitter", "const8", "const100")
STALLS = {50: 260, 110: 700, 170: 5200}  # the jittered clock's long steps (call: ms)


def case_clock(kind, calls=CASE_CALLS, start=CASE_START):
    if kind == "const8":
        step = np.full(calls, 8)
    elif kind == "const100":
        step = np.full(calls, 100)
    else:
        step = np.random.default_rng(0x9011).choice((8, 16, 17, 24), calls)
        for c, ms in STALLS.items():
            step[c] = ms
    step[0] = 0
    return (U(start) + np.cumsum(step).astype(U)).astype(U)


@functools.lru_cache(maxsize=None)
def gpu_case(kind, S=CASE_S, calls=CASE_CALLS):
    """(now [calls] uint64, kinds [calls][S] uint8, events [calls][S] uint8) by s % 6: 0 a message at
    every call; 1 silences shorter than every threshold; 2 silent past notify, then back, twice; 3
    silent past the timeout, then messages again; 4 a disconnect request in the events row (and a
    second one once it is Disconnected); 5 non-Input messages only."""
    now = case_clock(kind, calls)
    t = (now - now[0]).astype(np.int64)  # ms since the start
    kinds = np.zeros((calls, S), np.uint8)
    events = np.zeros((calls, S), np.uint8)
    for s in range(S):
        cls, shift = s % 6, 10 * (s // 6 % 5)
        msg = K_INPUT | (K_QUALITY_REPORT if s % 4 == 1 else 0)
        col = np.full(calls, msg, np.uint8)
        col[::12] |= K_QUALITY_REPLY
        if cls == 1:
            last = 0
            for c in range(1, calls):
                if (c + s) % 7 in (1, 2, 3) and t[c] - t[last] < 150:
                    col[c] = 0
                else:
                    last = c
        elif cls == 2:
            for a in (300 + shift, 900 + shift):
                col[(t >= a) & (t < a + 300)] = 0
        elif cls == 3:
            col[(t >= 500 + shift) & (t < 1400 + shift)] = 0
        elif cls == 4:
            events[np.argmax(t >= 700 + shift), s] = CASE_RMASK
            events[np.argmax(t >= 1000 + shift), s] = CASE_RMASK
        elif cls == 5:
            col[:] = K_INPUT_ACK | (K_CHECKSUM_REPORT if s % 4 == 1 else 0)
            col[::12] = K_KEEP_ALIVE
        kinds[:, s] = col
    return now, kinds, events


def case_run(kind, status=None):
    now, kinds, events = gpu_case(kind)
    return run(CASE_S, CASE_TIMEOUT, CASE_NOTIFY, CASE_START, CASE_RMASK, now, kinds, events, status=status)


def assert_case_is_not_vacuous(kind, m):
    """Every class raises what it must under clock `kind` (m: run()'s result), so parity with this
    model cannot pass vacuously.  SHUTDOWN needs 5,000 ms after the disconnect, which the constant
    8 ms clock (1.6 s in all) never reaches."""
    cls = np.arange(CASE_S) % 6
    net = m["net_events"]
    bit = lambda b: (net & b).any(axis=0)  # noqa: E731
    any_ = lambda name: m[name].any(axis=0)  # noqa: E731
    # class 0: a report whenever 200 ms have passed, an ack at every call, and nothing else
    assert any_("send_report")[cls == 0].all() and m["send_ack"][:, cls == 0].all()
    assert not net[:, cls == 0].any() and not m["resend"][:, cls == 0].any()
    # class 1: nothing of the link's state, acks and reports
    assert not net[:, cls == 1].any() and any_("send_ack")[cls == 1].all() and any_("send_report")[cls == 1].all()
    # class 2: INTERRUPTED then RESUMED, twice, and nothing else
    two = net[:, cls == 2]
    assert ((two & NET_INTERRUPTED) != 0).sum(axis=0).tolist() == [2] * two.shape[1]
    assert ((two & NET_RESUMED) != 0).sum(axis=0).tolist() == [2] * two.shape[1]
    assert not (two & (NET_DISCONNECTED | NET_SHUTDOWN)).any() and any_("resend")[cls == 2].all()
    # class 3: INTERRUPTED, the timeout's DISCONNECTED with the remote bit in the events row, acks afterwards
    assert bit(NET_INTERRUPTED)[cls == 3].all() and bit(NET_DISCONNECTED)[cls == 3].all()
    assert not bit(NET_RESUMED)[cls == 3].any() and any_("resend")[cls == 3].all()
    assert ((m["events"] & CASE_RMASK) != 0).sum(axis=0)[cls == 3].tolist() == [1] * int((cls == 3).sum())
    # class 4: closed by the request, never by the timeout
    assert not bit(NET_DISCONNECTED)[cls == 4].any() and (m["model"].closed_call[cls == 4] >= 0).all()
    # class 5: no Input, so no ack, and the retry timer fires on its own; the link is never silent
    assert not m["send_ack"][:, cls == 5].any() and any_("resend")[cls == 5].all() and not net[:, cls == 5].any()
    if kind != "const8":
        assert bit(NET_SHUTDOWN)[(cls == 3) | (cls == 4)].all()
        assert (m["model"].state[(cls == 3) | (cls == 4)] == SHUTDOWN).all()
    else:
        assert (m["model"].state[(cls == 3) | (cls == 4)] == DISCONNECTED).all()
