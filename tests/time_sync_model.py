"""Python restatement of the P2P engine's time sync (ggrs_p2p_set_time_sync / time_sync,
csrc/p2p_time_sync.hip) -- the reference the device is compared against.  A helper, not a test file;
it lives here because oracle/ is frozen.

TimeSync: src/time_sync.rs literally -- two 30-entry lists, re-summed on every call, the averages in
numpy.float32 in the reference's operation order.
Endpoint: the words of UdpProtocol that time sync reads (round_trip_time, the two advantages, the
window, whether it runs): on_quality_reply, on_quality_report (protocol.rs:649-653),
update_local_frame_advantage (:260-269), the push inside send_input (:433-437).
Session: P2PSession::check_wait_recommendation (p2p_session.rs:804-817) over max_frame_advantage
(:786-802), one endpoint holding all remote players; step() is one call in include/ggrs_amd.h's order.
run(): a whole table of calls for S sessions, driven by the oracle's per-call `advanced`, the arrival
rows, the events and the two input tables -- never by the engine.
"""
import numpy as np

from tests.packet_emit_model import pushes

NULL_FRAME = -1
KEEP = -2 ** 31  # GGRS_TIME_SYNC_KEEP
FRAME_WINDOW_SIZE = 30
MIN_RECOMMENDATION = 3
RECOMMENDATION_INTERVAL = 60
MAX_RTT = 1 << 20
F32 = np.float32


def trunc_div(a, b):
    """a / b truncated towards zero, in exact integers."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class TimeSync:
    def __init__(self):
        self.local = [0] * FRAME_WINDOW_SIZE
        self.remote = [0] * FRAME_WINDOW_SIZE

    def advance_frame(self, frame, local_adv, remote_adv):
        self.local[frame % len(self.local)] = local_adv
        self.remote[frame % len(self.remote)] = remote_adv

    def average_frame_advantage(self):
        local_sum = sum(self.local)
        local_avg = F32(local_sum) / F32(len(self.local))
        remote_sum = sum(self.remote)
        remote_avg = F32(remote_sum) / F32(len(self.remote))
        return int((remote_avg - local_avg) / F32(2.0))  # `as i32`: towards zero

    def exact_average(self):
        """What exact integer arithmetic would give instead (the tests count where it differs)."""
        return trunc_div(sum(self.remote) - sum(self.local), 2 * FRAME_WINDOW_SIZE)


class Endpoint:
    def __init__(self, fps):
        self.fps = fps
        self.round_trip_time = 0
        self.remote_frame_advantage = 0
        self.local_frame_advantage = 0
        self.time_sync = TimeSync()
        self.running, self.closed_call = True, -1

    def on_quality_reply(self, rtt_ms):
        self.round_trip_time = min(rtt_ms, MAX_RTT)  # (the engine's stated clamp)

    def on_quality_report(self, frame_advantage):
        self.remote_frame_advantage = max(-32768, min(32767, frame_advantage))  # (an i16 on the wire)

    def update_local_frame_advantage(self, local_frame, last_recv_frame):
        if local_frame == NULL_FRAME or last_recv_frame == NULL_FRAME:
            return
        ping = self.round_trip_time // 2
        remote_frame = last_recv_frame + (ping * self.fps) // 1000
        self.local_frame_advantage = remote_frame - local_frame

    def send_input(self, frame):
        if not self.running:
            return
        self.time_sync.advance_frame(frame, self.local_frame_advantage, self.remote_frame_advantage)


class Session:
    def __init__(self, fps=60):
        self.endpoint = Endpoint(fps)
        self.next_recommended_sleep = 0
        self.frames_ahead = 0
        self.inexact = 0  # calls whose f32 average differed from the exact-integer one

    def step(self, c, cur, last_recv, pushed, rtt_ms=-1, remote_advantage=KEEP, close=False, stopped=False):
        """Call c of a session at current_frame `cur` (at the call's start) whose endpoint's
        last_recv_frame after the poll is `last_recv`; pushed: the frame the call's add_local_input
        queued (NULL_FRAME: dropped).  -> (local_advantage, frames_ahead, skip_frames)."""
        ep = self.endpoint
        if stopped:
            return ep.local_frame_advantage, 0, 0
        if ep.running:
            if rtt_ms >= 0:
                ep.on_quality_reply(int(rtt_ms))
            if remote_advantage != KEEP:
                ep.on_quality_report(int(remote_advantage))
            ep.update_local_frame_advantage(cur, last_recv)
            if close:
                ep.running, ep.closed_call = False, c
        # check_wait_recommendation
        self.frames_ahead = 0
        if ep.running:
            self.frames_ahead = ep.time_sync.average_frame_advantage()
            self.inexact += self.frames_ahead != ep.time_sync.exact_average()
        skip = 0
        if cur > self.next_recommended_sleep and self.frames_ahead >= MIN_RECOMMENDATION:
            self.next_recommended_sleep = cur + RECOMMENDATION_INTERVAL
            skip = self.frames_ahead
        if pushed != NULL_FRAME:
            ep.send_input(int(pushed))
        return ep.local_frame_advantage, self.frames_ahead, skip

    def state(self):
        """time_sync_state()'s words of one session."""
        ep = self.endpoint
        return (ep.local_frame_advantage, ep.remote_frame_advantage, ep.round_trip_time, self.next_recommended_sleep,
                ep.closed_call, np.array([ep.time_sync.local, ep.time_sync.remote], np.int32))


def tables(advanced, input_delay, stop_call=None):
    """(cur [calls][S], pushed [calls][S]) from the oracle's per-call `advanced` [calls][S]: the
    session's current_frame at each call's start and the frame its add_local_input queued
    (packet_emit_model.pushes); past stop_call[s] (-1: none) the columns mean nothing."""
    calls, S = advanced.shape
    cur = np.zeros((calls, S), np.int32)
    cur[1:] = np.cumsum(advanced[:-1].astype(np.int32), axis=0)
    pushed = np.stack([pushes(advanced[:, s], input_delay) for s in range(S)], axis=1)
    if stop_call is not None:
        for s in np.nonzero(stop_call >= 0)[0]:
            pushed[stop_call[s]:, s] = NULL_FRAME
    return cur, pushed


def new_outputs(calls, S):
    return dict(local_advantage=np.zeros((calls, S), np.int32), frames_ahead=np.zeros((calls, S), np.int32),
                skip_frames=np.zeros((calls, S), np.int32))


def final_state(sessions):
    """The sessions' state() stacked as time_sync_state() returns it, plus `inexact` [S]."""
    st = [x.state() for x in sessions]
    out = [np.array([v[i] for v in st], np.int32) for i in range(5)]
    return tuple(out) + (np.stack([v[5] for v in st], axis=2), np.array([x.inexact for x in sessions]))


def run(cur, pushed, recv, events, rmask, fps=60, rtt_ms=None, remote_advantage=None, stop_call=None):
    """cur, pushed [calls][S] (tables()), recv [calls][S] the endpoint's last_recv_frame after each
    call, events [calls][S] u8, rmask the remote players' bits, rtt_ms / remote_advantage [calls][S]
    or None, stop_call [S] (-1: none).  Returns dict(local_advantage, frames_ahead, skip_frames
    [calls][S], state = final_state())."""
    calls, S = cur.shape
    out = new_outputs(calls, S)
    sessions = [Session(fps) for _ in range(S)]
    for s, x in enumerate(sessions):
        for c in range(calls):
            stopped = stop_call is not None and 0 <= stop_call[s] <= c
            r = x.step(c, int(cur[c, s]), int(recv[c, s]), int(pushed[c, s]),
                       -1 if rtt_ms is None else int(rtt_ms[c, s]),
                       KEEP if remote_advantage is None else int(remote_advantage[c, s]),
                       bool(events is not None and events[c, s] & rmask), stopped)
            out["local_advantage"][c, s], out["frames_ahead"][c, s], out["skip_frames"][c, s] = r
    out["state"] = final_state(sessions)
    return out


def input_tables(S, calls, seed):
    """(rtt_ms, remote_advantage) [calls][S] int32 as a live host would hand them: rtt_ms piecewise
    constant per session from {0, 16, 33, 50, 100, 250, 1000}, reported on about 5 % of the calls (-1
    elsewhere); remote_advantage KEEP on about 80 % of the calls, else a per-session base in [-12, 12]
    plus noise in [-3, 3]; a few +-32767 and one out-of-range 40000."""
    rng = np.random.default_rng(seed)
    rtt = np.full((calls, S), -1, np.int32)
    hit = rng.random((calls, S)) < 0.05
    rtt[hit] = rng.choice(np.array([0, 16, 33, 50, 100, 250, 1000], np.int32), int(hit.sum()))
    base = rng.integers(-12, 13, S)
    radv = (base[None, :] + rng.integers(-3, 4, (calls, S))).astype(np.int32)
    radv[rng.random((calls, S)) < 0.8] = KEEP
    for k, v in enumerate((32767, -32767, 32767, -32767)):
        radv[(37 * (k + 1)) % calls, (11 * k + 3) % S] = v
    radv[calls // 2, 7 % S] = 40000
    return rtt, radv
