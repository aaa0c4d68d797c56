"""CPU checks of tests/packet_emit_model.py, the reference of the device's packet emit
(ggrs_p2p_set_packet_emit / emit_packets): the sender's rules case by case, and the closed loop of
two modelled peers through a lossy link -- whose tables the GPU pair test (tests/test_gpu_p2p_emit.py)
reuses, so the conditions that test relies on are asserted here on the model alone."""
import functools

import numpy as np

from tests import packet_emit_model as E
from tests import packet_feed_model as F

PAIR_S, PAIR_CALLS, PAIR_TAIL = 130, 240, 40  # 200 lossy calls and a loss-free tail


@functools.lru_cache(maxsize=None)
def pair_case():
    """The pair test's inputs and the model's run of them: (rows_a, rows_b [calls][S][2], delay, drop
    [2][calls][S], resend [calls][S], the peers (A, B) per session)."""
    from oracle import oracle as O
    S, calls = PAIR_S, PAIR_CALLS
    rows_a = np.stack([O.gen_inputs(O.session_seed(s, 0xE317A), calls, 2, s % 2) for s in range(S)], axis=1)
    rows_b = np.stack([O.gen_inputs(O.session_seed(s, 0xE317B), calls, 2, (s + 1) % 2) for s in range(S)], axis=1)
    delay, drop, resend = E.link_tables(S, calls, seed=41, tail=PAIR_TAIL)
    peers = [E.pair_run(rows_a[:, s].copy(), rows_b[:, s].copy(), delay[:, :, s], drop[:, :, s], resend[:, s])
             for s in range(S)]
    return rows_a, rows_b, delay, drop, resend, peers


def decode(reference, data):
    rc, inputs = F.codec_decode(reference, data)
    assert rc == 0
    return inputs


def test_ack_cases(oracle):
    """No ack, a stale one, one in the middle of the queue, one beyond the newest pending frame."""
    snd = E.Sender(2, 16)
    frames = {f: bytes([f * 7 & 0xff, 255 - f]) for f in range(12)}
    for f in range(6):
        start, data = snd.step(f, push=(f, frames[f]))
        assert start == 0 and decode(bytes(2), data) == [frames[g] for g in range(f + 1)]
    assert snd.last_acked == (E.NULL_FRAME, bytes(2)) and len(snd.pending) == 6
    start, data = snd.step(6, ack=2, push=(6, frames[6]))  # mid-queue
    assert snd.last_acked == (2, frames[2]) and start == 3
    assert decode(frames[2], data) == [frames[g] for g in range(3, 7)]
    assert snd.step(7, ack=1) == (-1, b"") and snd.last_acked[0] == 2  # stale, nothing pushed: no packet
    assert snd.step(8, ack=2)[0] == -1 and [f for f, _ in snd.pending] == [3, 4, 5, 6]  # at last_acked: stale
    start, data = snd.step(9, ack=2, resend=True)  # the retry timer
    assert start == 3 and decode(frames[2], data) == [frames[g] for g in range(3, 7)]
    assert snd.step(10, ack=40) == (-1, b"")  # beyond the newest: pops everything
    assert snd.last_acked == (6, frames[6]) and snd.pending == []
    assert snd.step(11, resend=True) == (-1, b"")  # nothing pending: no retry
    start, data = snd.step(12, push=(7, frames[7]), resend=True)  # at most one packet
    assert start == 7 and decode(frames[6], data) == [frames[7]]


def test_overflow_and_close_at_the_exact_call(oracle):
    snd = E.Sender(1, 4)
    for f in range(4):
        assert snd.step(f, push=(f, bytes([f + 1])))[0] == 0
    assert snd.status == 0 and len(snd.pending) == 4
    assert snd.step(4, push=(4, b"\x09")) == (-1, b"")  # the fifth unacknowledged input
    assert (snd.status, snd.closed_call) == (E.EMIT_DISCONNECTED, 4)
    assert snd.step(5, ack=3, push=(5, b"\x01"), resend=True) == (-1, b"") and len(snd.pending) == 5
    snd = E.Sender(1, 4)
    snd.step(0, push=(0, b"\x05"))
    snd.step(1, push=(1, b"\x06"))
    assert snd.step(2, ack=0, close=True, push=(2, b"\x07"), resend=True) == (-1, b"")  # the closing call: ack, no push
    assert (snd.status, snd.closed_call, snd.last_acked[0], len(snd.pending)) == (E.EMIT_CLOSED, 2, 0, 1)
    assert snd.step(3, push=(3, b"\x08")) == (-1, b"")
    snd = E.Sender(1, 4)  # a stopped session takes no step
    snd.step(0, push=(0, b"\x05"))
    assert snd.step(1, ack=0, push=(1, b"\x06"), stopped=True) == (-1, b"") and len(snd.pending) == 1


def test_pushes_follow_the_session_frame(oracle):
    adv = np.array([1, 1, 0, 0, 1, 1], np.uint8)  # two calls at the prediction threshold
    assert E.pushes(adv, 0).tolist() == [0, 1, 2, -1, -1, 3]
    assert E.pushes(adv, 2).tolist() == [2, 3, 4, -1, -1, 5]


def test_closed_loop_reconstructs_every_sent_frame(oracle):
    """Two modelled peers per session over delays of 1-4 calls, 25 % loss, a 20-call blackout in every
    fifth session and resend flags at c % 4 == s % 4: every frame a peer sent is in the other's rows,
    no receiver stops, pending stays within 64 (the GPU pair test's cap), and the blackout sessions
    hit the prediction threshold."""
    rows_a, rows_b, delay, drop, resend, peers = pair_case()
    assert delay.min() == 1 and delay.max() == 4
    assert 0.2 < drop[:, :PAIR_CALLS - PAIR_TAIL].mean() < 0.4
    for s, (A, B) in enumerate(peers):
        for X, Y in ((A, B), (B, A)):
            assert X.recv.stop_call is None, s
            assert X.snd.status == 0 and X.snd.max_seen <= 64, (s, X.snd.max_seen)
            # the loss-free tail delivered and confirmed everything but the messages still in flight
            # (a packet takes one call, its ack another)
            assert len(X.sent) > 150 and len(X.snd.pending) <= 2, s
            assert Y.recv.last >= max(X.sent) - 1, s
            for f, b in X.sent.items():
                assert f > Y.recv.last or Y.remote[f].tobytes() == b, (s, f)
        if s % 5 == 0:
            assert A.skipped > 0 and B.skipped > 0, s
    # (the prediction threshold bounds what a blacked-out peer queues: max_prediction and the frames in flight)
    assert max(max(A.snd.max_seen, B.snd.max_seen) for A, B in peers) > 8


def test_lib_binds_the_emit_symbols():
    from ggrs_amd import _lib
    for name in ("ggrs_p2p_set_packet_emit", "ggrs_p2p_emit_packets", "ggrs_p2p_read_emit_state"):
        assert name in _lib.EXPORTS
    assert (_lib.GGRS_EMIT_CLOSED, _lib.GGRS_EMIT_DISCONNECTED) == (-18, -19)
