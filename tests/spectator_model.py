"""Python restatement of SpectatorSession (caspark/ggrs 0.10.2, src/sessions/p2p_spectator_session.rs)
stepped call by call over the oracle's ex_game step (oracle.state_advance) and checksum
(oracle.fletcher16) -- the reference the device spectator engine (ggrs_spectator_*, csrc/spectator.hip)
is compared against.  A helper, not a test file; it lives here because oracle/ is frozen.

One call c of a session (advance_frame :103-129, inputs_at_frame :168-197, Event::Input :218-231,
UdpProtocol::on_input's status merge, src/network/protocol.rs:575-585):
  1. the call's connect-status note is merged into the host endpoint's status (disconnected sticky,
     last_frame the maximum); the host's frames (last_recv, recv_upto[c]] arrive, and with an
     arrival the session copies the endpoint's status (a note is visible only with an Event::Input);
  2. n = catchup_speed if last_recv - current_frame > max_frames_behind else 1;
  3. n times, f = current_frame + 1: last_recv < f -> PredictionThreshold; the buffer slot f % 60
     already holds a newer frame (last_recv >= f + 60) -> SpectatorTooFarBehind; else AdvanceFrame
     with input row f, player k Disconnected iff disconnected[k] and last_frame[k] < f.
     An error leaves the loop (`?`); the frames advanced before it stay advanced.
The ABI's two per-session stops (include/ggrs_amd.h): an arrival naming a frame >= row_hi (not added
when the launch started) stops the session with GGRS_E_INVALID before anything else in that call; a
frame to advance whose row is below row_lo (no longer held) stops it with GGRS_E_PRECONDITION.  A
stopped session changes no more.
"""
import numpy as np

from oracle import oracle as O

SPECTATOR_BUFFER_SIZE = 60
NULL_FRAME = -1
E_INVALID, E_PRECONDITION, E_TOO_FAR_BEHIND = -1, -2, -5
STATUS_DISCONNECTED = 2


def note(player, frame):
    """GGRS_SPECTATOR_NOTE"""
    return 1 | player << 1 | (frame + 1) << 3


class Spectator:
    """One session."""

    def __init__(self, num_players, max_frames_behind=10, catchup_speed=1):
        self.P = num_players
        self.max_frames_behind, self.catchup_speed = max_frames_behind, catchup_speed
        self.current_frame = NULL_FRAME
        self.last_recv = NULL_FRAME
        self.state = O.state_new(num_players)
        self.checksum = O.fletcher16(self.state)
        # the endpoint's peer_connect_status and the session's host_connect_status: [disconnected, last_frame]
        self.endpoint = [[False, NULL_FRAME] for _ in range(num_players)]
        self.host_connect_status = [[False, NULL_FRAME] for _ in range(num_players)]
        self.waited = 0
        self.error = 0

    @property
    def stopped(self):
        return self.error in (E_INVALID, E_PRECONDITION)

    def call(self, recv_upto, note_word, rows, row_lo=0, row_hi=None):
        """One advance_frame; rows[f] = the host's confirmed inputs of frame f ([P] u8).  Returns the
        number of AdvanceFrame requests executed."""
        row_hi = len(rows) if row_hi is None else row_hi
        if self.stopped:
            return 0
        if recv_upto > self.last_recv and recv_upto >= row_hi:
            self.error = E_INVALID
            return 0
        if note_word & 1:
            k, fr = (note_word >> 1) & 3, (note_word >> 3) - 1
            self.endpoint[k][0] = True
            self.endpoint[k][1] = max(self.endpoint[k][1], fr)
        if recv_upto > self.last_recv:  # Event::Input for every new frame
            self.last_recv = int(recv_upto)
            self.host_connect_status = [list(e) for e in self.endpoint]
        behind = self.last_recv - self.current_frame
        n = self.catchup_speed if behind > self.max_frames_behind else 1
        advanced = 0
        for _ in range(n):
            f = self.current_frame + 1
            if self.last_recv < f:  # slot frame < frame_to_grab
                self.waited += 1
                break
            if self.last_recv >= f + SPECTATOR_BUFFER_SIZE:  # slot frame > frame_to_grab
                self.error = E_TOO_FAR_BEHIND
                break
            if f < row_lo:
                self.error = E_PRECONDITION
                break
            status = np.zeros(self.P, np.uint8)
            for k, (disc, last) in enumerate(self.host_connect_status):
                if disc and last < f:
                    status[k] = STATUS_DISCONNECTED
            self.state = O.state_advance(self.state, rows[f], status)
            self.current_frame = f
            advanced += 1
        if advanced:
            self.checksum = O.fletcher16(self.state)
        return advanced


def run(rows, recv_upto, notes=None, num_players=2, max_frames_behind=10, catchup_speed=1, windows=None):
    """A session over len(recv_upto) calls.  windows: [(n_calls, row_lo, row_hi)] per launch (default:
    one launch holding every row).  Returns dict(current_frame, last_recv, waited, error, state,
    advanced [calls] u8, checksums [calls] u16)."""
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, num_players)
    calls = len(recv_upto)
    s = Spectator(num_players, max_frames_behind, catchup_speed)
    adv, cks = np.zeros(calls, np.uint8), np.zeros(calls, np.uint16)
    windows = windows or [(calls, 0, len(rows))]
    c = 0
    for n, lo, hi in windows:
        for _ in range(n):
            adv[c] = s.call(int(recv_upto[c]), 0 if notes is None else int(notes[c]), rows, lo, hi)
            cks[c] = s.checksum
            c += 1
    assert c == calls
    return dict(current_frame=s.current_frame, last_recv=s.last_recv, waited=s.waited, error=s.error,
                state=s.state.copy(), advanced=adv, checksums=cks)


def schedules(S, calls, P, seed):
    """[calls][S] recv_upto and notes for the parity families: s % 3 != 2 jitter with stalls
    (oracle.stall_schedule(calls, 8, seed)), else a fixed lag s % 7 + 1; s % 8 == 7: from call 100 the
    host runs 3 frames per call; s % 8 == 3: from call 60 the host jumps 40 frames ahead, then runs at
    call pace; s % 5 == 0: one note for player s % P at call 50 + s % 100 with last frame 40 + s % 100.
    One more family, s % 24 == 5 (fixed-lag sessions outside the ones above), so that the slowest
    legal catch-up (max_frames_behind 59) is exercised often: from call 60, every 32 calls the host is
    silent for 22 calls -- the spectator uses up what it has and waits -- then delivers 60 frames at
    once, exactly the buffer: a spectator that had caught up is 60 behind (catch-up, not lost), one
    that had not is lost."""
    recv = np.zeros((calls, S), np.int32)
    notes = np.zeros((calls, S), np.int32)
    c = np.arange(calls)
    for s in range(S):
        if s % 3 != 2:
            r = O.stall_schedule(calls, 8, seed * 1000 + s).astype(np.int64)
        else:
            r = np.maximum(c - (s % 7 + 1), -1)
        if s % 8 == 7:
            r = r + np.where(c >= 100, 2 * (c - 99), 0)
        if s % 8 == 3:
            r = r + np.where(c >= 60, 40, 0)
        if s % 24 == 5:
            for t in range(60, calls - 31, 32):
                r[t:t + 22] = r[t - 1]
                r[t + 22:] = r[t - 1] + 60 + np.arange(len(r) - t - 22)
        recv[:, s] = np.maximum.accumulate(r)
        if s % 5 == 0 and 50 + s % 100 < calls:
            notes[50 + s % 100, s] = note(s % P, 40 + s % 100)
    return recv, notes
