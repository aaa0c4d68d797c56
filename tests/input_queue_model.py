"""The frame bookkeeping of one remote player's InputQueue in a P2P session, restated from the
reference in plain Python, sharing no code with oracle/: where the queue's 128 entries run out.

Only frames are kept (no inputs, no predictions): the tail's frame, the length, last_added_frame
and last_requested_frame.  Restated:
  * add_input -> add_input_by_frame (input_queue.rs:170-230): frames arrive in sequence, each adds
    one entry, and `assert!(self.length <= INPUT_QUEUE_LENGTH)` (:207) is the panic looked for;
  * discard_confirmed_frames (:83-101), with its three branches;
  * input()'s `self.last_requested_frame = requested_frame` (:110);
  * SyncLayer::set_last_confirmed_frame's clamp to the current frame and its `> 0` guard
    (sync_layer.rs:313-340; without sparse saving);
  * P2PSession::advance_frame's order (p2p_session.rs:265-426): poll_remote_clients (the burst of
    remote frames), confirmed_frame, set_last_confirmed_frame (the discard), add_local_input, then
    the AdvanceFrame, whose synchronized_inputs requests the current frame from every queue.
A session without disconnects and without rollbacks' replays is enough for the bookkeeping: a
replay ends by requesting frame current - 1 (after load_frame's reset_prediction cleared
last_requested_frame), which is what the queue already held from the frame's first simulation.
"""

NULL_FRAME = -1
INPUT_QUEUE_LENGTH = 128  # input_queue.rs:6


class QueueOverflow(Exception):
    pass


class RemoteQueueFrames:
    def __init__(self):
        self.tail_frame = NULL_FRAME  # inputs[tail].frame: a blank input until the first add
        self.length = 0
        self.last_added_frame = NULL_FRAME
        self.last_requested_frame = NULL_FRAME

    def add_input(self, frame):
        # (frame_delay 0 for a remote player: the sequence check of :172-177 and advance_queue_head
        # pass a frame through when it is last_added_frame + 1)
        assert frame == self.last_added_frame + 1
        if self.length == 0:
            self.tail_frame = frame  # head == tail: the entry written is the tail's
        self.length += 1
        if self.length > INPUT_QUEUE_LENGTH:
            raise QueueOverflow(frame)
        self.last_added_frame = frame

    def discard_confirmed_frames(self, frame):
        if self.last_requested_frame != NULL_FRAME:
            frame = min(frame, self.last_requested_frame)
        if frame >= self.last_added_frame:
            # "delete all but most recent": tail = head, the slot AFTER the newest entry, whose frame
            # is whatever that slot held 128 adds ago (blank before the first wrap); never taken by
            # a connected remote player's queue (frame <= confirmed - 1 < last_added_frame)
            raise AssertionError("discard past the newest remote input")
        elif frame <= self.tail_frame:
            pass
        else:
            offset = frame - self.tail_frame
            self.tail_frame += offset
            self.length -= offset

    def input(self, requested_frame):
        self.last_requested_frame = requested_frame
        assert requested_frame >= self.tail_frame


def first_overflow_call(arrive, advanced, local_players, input_delay, max_prediction):
    """The first call whose poll would push a remote InputQueue past 128 entries, or None.
    arrive[c]: the newest remote frame call c's poll delivered; advanced[c]: whether call c emitted
    its own AdvanceFrame (taken from the session under test: the threshold is not restated here)."""
    q = RemoteQueueFrames()
    current, local_last, lockstep = 0, NULL_FRAME, max_prediction == 0
    for c in range(len(arrive)):
        # poll_remote_clients
        try:
            for g in range(q.last_added_frame + 1, int(arrive[c]) + 1):
                q.add_input(g)
        except QueueOverflow:
            return c
        if c >= len(advanced):
            return None
        # confirmed_frame: the minimum over the connected players' last frames
        confirmed = q.last_added_frame if not local_players else min(q.last_added_frame, local_last)
        # set_last_confirmed_frame
        frame = min(confirmed, current)
        if frame > 0:
            q.discard_confirmed_frames(frame - 1)
        # add_local_input: frame current + delay, dropped unless it is the next in sequence
        if local_players and (local_last == NULL_FRAME or current + input_delay == local_last + 1):
            local_last = current + input_delay
        # the AdvanceFrame: synchronized_inputs, then current_frame += 1
        if advanced[c]:
            if lockstep:
                assert frame == current
            q.input(current)
            current += 1
    return None
