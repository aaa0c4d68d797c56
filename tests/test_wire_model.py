"""CPU checks of tests/wire_model.py, the reference of the device's wire envelope (ggrs_wire_unpack /
ggrs_wire_pack): the layout against hand-derived bytes, every way a datagram is refused, the poll
reductions against the literal handle_message fold, and the one-packet rule against the packet feed
model's receiver fed every Input of a poll."""
import numpy as np
import pytest

from tests import packet_feed_model as F
from tests import wire_model as W

NOW = 1 << 40

# The six known answers, derived by hand from messages.rs and bincode 1.3's layout with magic 0x1234
KNOWN = [
    (W.Message(0x1234, W.KeepAlive()), "34 12 05 00 00 00", 6),
    (W.Message(0x1234, W.InputAck(7)), "34 12 01 00 00 00 07 00 00 00", 10),
    (W.Message(0x1234, W.QualityReport(-3, 0x0102)), "34 12 02 00 00 00 fd ff 02 01" + " 00" * 14, 24),
    (W.Message(0x1234, W.QualityReply(0x0102)), "34 12 03 00 00 00 02 01" + " 00" * 14, 22),
    (W.Message(0x1234, W.ChecksumReport(0xBEEF, 20)), "34 12 04 00 00 00 ef be" + " 00" * 14 + " 14 00 00 00", 26),
    (W.Message(0x1234, W.Input([(False, -1), (True, 5)], False, 3, 2, b"\xaa\xbb")),
     "34 12 00 00 00 00 02 00 00 00 00 00 00 00 00 ff ff ff ff 01 05 00 00 00 00 03 00 00 00 02 00 00 00 02 00 00 00 00 00 "
     "00 00 aa bb", 43),
]


@pytest.mark.parametrize("msg,hexbytes,length", KNOWN, ids=[type(m.body).__name__ for m, _, _ in KNOWN])
def test_known_answers_both_directions(msg, hexbytes, length):
    data = bytes.fromhex(hexbytes)
    assert len(data) == length
    assert W.serialize(msg) == data
    assert W.deserialize(data) == msg
    assert (msg, data) in W.known_answers()  # what the GPU tests reuse


def test_lengths_follow_the_layout():
    assert len(W.serialize(W.Message(1, W.Input([(False, 0)] * 3, False, 0, 0, bytes(17))))) == 31 + 5 * 3 + 17
    assert W.max_datagram_bytes(2, 128) == 176 and W.max_datagram_bytes(4, 1012) == 1072
    assert W.max_datagram_bytes(1, 12) == 48  # 31 + 5 + 12 is a multiple of 16 already


def test_round_trip_of_random_messages_of_every_tag():
    rng = np.random.default_rng(3)
    for k in range(600):
        msg = W.random_message(rng, k % 6, num_statuses=1 + k % 4, max_body=40, now_ms=NOW, extra_statuses=k % 3)
        data = W.serialize(msg)
        assert W.deserialize(data) == msg
        st, got = W.classify(data, len(data), 256, 1 + k % 4, 40, NOW)
        assert st == k % 6 + 1 and got == msg


@pytest.mark.parametrize("ns", (2, 4))
def test_every_refusal_and_its_accepted_neighbour(ns):
    """Every truncation of every known answer, trailing bytes, bool byte 2, tag 6, the two oversized
    Vec lengths in either Vec, a short and a long status vector, E_CAP, E_CLOCK, E_RANGE."""
    cases = W.hostile_cases(ns, 16, NOW)
    names = [name for name, _, _ in cases]
    assert sum(n.startswith("truncated") for n in names) == sum(length - 1 for _, _, length in KNOWN)
    for code in (W.E_BINCODE, W.E_SHAPE, W.E_CAP, W.E_CLOCK, W.E_RANGE, 1, 2, 3, 4, 5, 6):
        assert any(want == code for _, _, want in cases), code
    for name, data, want in cases:
        st, msg = W.classify(data, len(data), 512, ns, 16, NOW)
        assert st == want, name
        assert (msg is not None) == (want > 0)
    # a datagram longer than its buffer, and the empty slot
    assert W.classify(bytes(600), 600, 512, ns, 16, NOW)[0] == W.E_BINCODE
    assert W.classify(b"", 0, 512, ns, 16, NOW)[0] == 0 and W.classify(b"", -3, 512, ns, 16, NOW)[0] == 0


def test_oversized_vec_lengths_are_compared_as_u64():
    raw = W.serialize(W.Message(1, W.Input([(False, 1), (False, 2)], False, 0, 0, b"abc")))
    for big in (0xFFFFFFFFFFFFFFFF, 0x100000002):  # the second is 2 after narrowing to 32 bits
        for at in (6, 14 + 10 + 9):
            bad = raw[:at] + big.to_bytes(8, "little") + raw[at + 8:]
            with pytest.raises(W.BincodeError):
                W.deserialize(bad)


def test_random_bytes_never_raise():
    rng = np.random.default_rng(11)
    seen = set()
    for k in range(2000):
        n = int(rng.integers(0, 80))
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if k % 2:  # a plausible header in front, so that the bodies' checks are reached
            data = (bytes([k & 255, 0, k % 7, 0, 0, 0]) + data)[:max(n, 1)]
        st, _ = W.classify(data, len(data), 64, 2, 8, NOW)
        seen.add(st)
    assert W.E_BINCODE in seen and len(seen) > 4


def random_poll(rng, slots, ns, max_body):
    """Up to `slots` slots: valid messages of every tag, refused ones and empty slots."""
    hostile = W.hostile_cases(ns, max_body, NOW)
    poll = []
    for _ in range(slots):
        r = rng.random()
        if r < 0.15:
            poll.append((b"", 0))
        elif r < 0.3:
            data = hostile[int(rng.integers(len(hostile)))][1]
            poll.append((data, len(data)))
        else:
            data = W.serialize(W.random_message(rng, int(rng.integers(6)), ns, max_body, NOW))
            poll.append((data, len(data)))
    return poll


def test_reductions_equal_the_literal_fold():
    """ack_in (through the pending pops), the connect status, the disconnect event, the advantage, the
    round trip, the reply and the newest checksum report of unpack_poll against handle_message applied
    to every accepted message of the poll in order."""
    rng = np.random.default_rng(5)
    for k in range(400):
        ns = 1 + k % 4
        poll = random_poll(rng, 1 + k % 8, ns, 12)
        pending = sorted(int(x) for x in rng.integers(0, 1 << 20, 12))
        ep = W.Endpoint(ns, pending)
        for data, length in poll:
            st, msg = W.classify(data, length, 512, ns, 12, NOW)
            if msg is not None:
                ep.handle_message(msg, NOW)
        out = W.unpack_poll(poll, 512, ns, 0b10, k, 12, NOW)
        # pop_pending_output is monotone: one pop at the maximum equals the pops in order
        ref = W.Endpoint(ns, pending)
        ref.pop_pending_output(out["ack_in"])
        assert ref.pending == ep.pending
        assert bool(out["events"]) == ep.disconnect_event and out["events"] in (0, 0b10)
        assert [bool(out["disc_mask"] >> i & 1) for i in range(ns)] == [st[0] for st in ep.status]
        assert out["last_frame"] == [st[1] for st in ep.status]
        if ep.remote_frame_advantage is None:
            assert out["remote_advantage"] == W.TIME_SYNC_KEEP and out["ping"] is None
        else:
            assert out["remote_advantage"] == ep.remote_frame_advantage
            assert int.from_bytes(out["ping"], "little") == ep.replies[-1]  # one reply, to the last report
        assert out["rtt_ms"] == (-1 if ep.round_trip_time is None else min(ep.round_trip_time, W.INT32_MAX))
        if ep.pending_checksums:
            # the report with the greatest frame, the last one of equal frames (a HashMap insert replaces)
            assert out["report_frame"] == max(ep.pending_checksums)
            assert out["report_checksum"] == ep.pending_checksums[out["report_frame"]]
        else:
            assert out["report_frame"] == W.NULL_FRAME
        assert len(ep.inputs) == sum(st == 1 for st in out["slot_status"])
        if ep.inputs:
            top = max(s for s, _ in ep.inputs)
            assert out["start_frame"] == top
            assert out["packet"] == [d for s, d in ep.inputs if s == top][-1]  # ties to the later slot
        else:
            assert (out["start_frame"], out["packet_len"]) == (-1, 0)
        players = [i for i in range(ns) if out["disc_mask"] >> i & 1]
        if players:
            p = players[k % len(players)]
            assert out["notes"] == W.spectator_note(p, out["last_frame"][p])
        else:
            assert out["notes"] == 0


def test_notes_are_the_spectator_feeds_words():
    assert W.spectator_note(1, 5) == 1 | 1 << 1 | 6 << 3  # GGRS_SPECTATOR_NOTE(1, 5)
    poll = [(d, len(d)) for d in [W.serialize(W.Message(1, W.Input([(True, 4), (False, 9), (True, -1)], False, 0, 0, b"x")))]]
    notes = [W.unpack_poll(poll, 64, 3, 0, c, 4, NOW)["notes"] for c in range(4)]
    assert notes == [W.spectator_note(0, 4), W.spectator_note(2, -1)] * 2


def test_pack_slots():
    kw = dict(start_frame=3, packet_len=2, ack_frame=2, packet=b"\xaa\xbb\xcc", disc_mask=0b10, last_frame=[-1, 5])
    known = dict((type(m.body).__name__, d) for m, d in W.known_answers())
    out = W.pack_call(0x1234, 0x0102, 2, 16, send_ack=1, keep_alive=1, send_report=1, local_advantage=-3,
                      kinds=1 << W.QUALITY_REPORT, ping=(0x0102).to_bytes(16, "little"), report_frame=20,
                      report_checksum=0xBEEF, **kw)
    assert out == [known["Input"], known["QualityReport"], known["QualityReply"], known["ChecksumReport"]]
    # no packet: the ack alone; nothing at all: the keep-alive, and only then
    assert W.pack_call(0x1234, 0, 2, 16, send_ack=1, keep_alive=1, ack_frame=7, start_frame=-1, packet_len=0,
                       packet=b"") == [known["InputAck"], b"", b"", b""]
    assert W.pack_call(0x1234, 0, 2, 16, keep_alive=1) == [known["KeepAlive"], b"", b"", b""]
    assert W.pack_call(0x1234, 0, 2, 16, keep_alive=1, report_frame=0)[0] == b""
    assert W.pack_call(0x1234, 0, 2, 16) == [b""] * 4
    # the advantage is clamped as send_quality_report clamps it; a packet longer than its row is no packet
    assert W.deserialize(W.pack_call(1, 9, 2, 16, send_report=1, local_advantage=40000)[1]).body == W.QualityReport(32767, 9)
    assert W.pack_call(1, 9, 2, 16, start_frame=0, packet_len=17, packet=bytes(17)) == [b""] * 4
    # what pack writes, unpack accepts, field by field
    got = W.unpack_poll([(d, len(d)) for d in out], 64, 2, 0b10, 0, 16, 0x0102)
    assert got["slot_status"] == [1, 3, 4, 5] and got["kinds"] == 0b11101
    assert (got["start_frame"], got["packet"], got["ack_in"]) == (3, b"\xaa\xbb", 2)
    assert (got["disc_mask"], got["last_frame"]) == (0b10, [-1, 5])
    assert (got["remote_advantage"], got["rtt_ms"], got["report_frame"], got["report_checksum"]) == (-3, 0, 20, 0xBEEF)


def _link_polls(sender, delay, drop, calls):
    """A direction's surviving Input messages, poll by poll: [[(start, bytes)]] per call.  The message
    of call c' arrives at call c' + delay[c'] unless dropped; the messages of one poll in the link's
    own order (tests/packet_emit_model.py's route: by sending call)."""
    polls = [[] for _ in range(calls)]
    for c2 in range(calls):
        c = c2 + int(delay[c2])
        if not drop[c2] and sender.start[c2] >= 0 and c < calls:
            polls[c].append((int(sender.start[c2]), sender.data[c2]))
    return polls


def test_one_packet_of_a_poll_delivers_what_all_of_them_would(oracle):
    """The pair case's traffic (tests/test_packet_emit_model.py: delays of 1-4 calls, so up to four
    messages to a poll, 25 % loss, blackouts), both directions of every session, every surviving Input
    wrapped into a datagram: a packet feed receiver given unpack_poll's one packet per poll has the
    same rows and the same last_recv after every poll as one given every Input of the poll in arrival
    order, and neither ever stops.  (The polls are the recorded loop's own: the rule rests on the
    sender having learned start_frame - 1 from an ack this receiver sent, so a recorded trace cannot be
    replayed under another poll schedule.)"""
    from tests.test_packet_emit_model import PAIR_CALLS, pair_case
    rows_a, rows_b, delay, drop, resend, peers = pair_case()
    stride = F.max_packet_bytes(1, 64)
    dstride = W.max_datagram_bytes(2, stride)
    several = 0
    for s in range(len(peers)):
        for d in (0, 1):
            every = F.Receiver(np.zeros((PAIR_CALLS, 1), np.uint8), 8, 64, stride)
            one = F.Receiver(np.zeros((PAIR_CALLS, 1), np.uint8), 8, 64, stride)
            for c, msgs in enumerate(_link_polls(peers[s][d], delay[d, :, s], drop[d, :, s], PAIR_CALLS)):
                slots = []
                for start, data in msgs:
                    every.receive(c, start, data)
                    dg = W.serialize(W.Message(s, W.Input([(False, -1)] * 2, False, start, -1, data)))
                    slots.append((dg, len(dg)))
                several += len(msgs) > 1
                out = W.unpack_poll(slots, dstride, 2, 0b10, c, stride, 0)
                assert out["slot_status"] == [1] * len(msgs)
                one.receive(c, out["start_frame"], out["packet"])
                assert every.stop_call is None and one.stop_call is None, (s, d, c)
                assert one.last == every.last, (s, d, c)
                assert (one.remote == every.remote).all(), (s, d, c)
            assert every.last > 150, (s, d)
    assert several > 20 * len(peers)


def test_reversed_equal_start_packets_lose_the_tail_until_the_next_resend():
    """The stated divergence: two packets of one start_frame arriving with the shorter one last."""
    def dgram(start, data):
        d = W.serialize(W.Message(1, W.Input([(False, -1)] * 2, False, start, -1, data)))
        return d, len(d)
    poll = [dgram(4, b"longer tail"), dgram(4, b"short")]
    out = W.unpack_poll(poll, 96, 2, 0, 0, 32, 0)
    assert (out["start_frame"], out["packet"]) == (4, b"short")
    out = W.unpack_poll(poll[::-1] + [dgram(3, b"older")], 96, 2, 0, 0, 32, 0)
    assert (out["start_frame"], out["packet"]) == (4, b"longer tail")
