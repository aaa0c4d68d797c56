"""GPU check of what packet emit and spectator emit share on the host (csrc/p2p_engine.h's
PacketEmitState): the staging layout of a launch's six arrays and the group arithmetic, at more than
one call per launch.  130 sessions (two full blocks and a block of two), 20 calls emitted in one
launch (more than one group of slots), each emit on two identically driven engines -- once through
host arrays (the staging buffer), once through device tensors with out= -- and both against the
model: start_frame, packet_len, the per-call word and each packet row's first packet_len bytes (the
bytes past them are written on neither path)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import packet_feed_model as F  # noqa: E402
from tests import spectator_emit_model as M  # noqa: E402
from tests import test_gpu_p2p_emit as PE  # noqa: E402
from tests import test_gpu_spectator_emit as SE  # noqa: E402

pytestmark = pytest.mark.gpu

S, N = 130, 20  # sessions; the calls of the launch under test


def emit_both_ways(emit_host, emit_dev, c0, ack, resend, m_start, m_len, m_word, m_packets):
    """Calls c0 .. c0 + N - 1 through host arrays and through device tensors; every output of both
    against the model's rows c0 .. c0 + N - 1."""
    sl = slice(c0, c0 + N)
    host = emit_host(c0, N, ack[sl], resend[sl])
    dev = torch.device("cuda")
    out = (torch.full(m_start[sl].shape, -7, dtype=torch.int32, device=dev),
           torch.full(m_len[sl].shape, -7, dtype=torch.int32, device=dev),
           torch.full(m_word[sl].shape, -7, dtype=torch.int32, device=dev),
           torch.full(m_packets[sl].shape, 0xA5, dtype=torch.uint8, device=dev))
    got = emit_dev(c0, N, torch.from_numpy(ack[sl].copy()).to(dev), torch.from_numpy(resend[sl].copy()).to(dev), out=out)
    torch.cuda.synchronize()
    device = tuple(t.cpu().numpy() for t in got)
    for name, h, d, want in zip(("start", "len", "word"), host, device, (m_start[sl], m_len[sl], m_word[sl])):
        assert (h == want).all(), (name, "host", np.argwhere(h != want)[:5])
        assert (d == want).all(), (name, "device", np.argwhere(d != want)[:5])
    length = m_len[sl]
    body = np.arange(m_packets.shape[-1]) < length[..., None]
    assert (length > 0).sum() > length.size // 4
    for path, pk in (("host", host[3]), ("device", device[3])):
        assert (np.where(body, pk, 0) == m_packets[sl]).all(), path
    return host, device


def test_packet_emit_20_calls_in_one_launch_host_and_device(oracle):
    """P = 2, one local player; calls 100 .. 119 of the parity case's tables in one launch (groups of
    8, 8 and 4 calls), after calls 0 .. 99 in another."""
    P, local, delay, mp, c0 = 2, (0,), 0, 8, 100
    rows, arrive, events, ack, resend, m = PE.parity_case(P, local, delay, mp)
    engines = [PE.engine(P, local, delay, mp) for _ in range(2)]
    for e in engines:
        e.add_inputs(0, rows[:c0 + N])
        e.add_arrivals(0, arrive[:c0 + N], events[:c0 + N])
        e.advance_frames(c0 + N)
        PE.assert_emitted(e.emit_packets(0, c0, ack[:c0], resend[:c0]), m, 0, c0)
    emit_both_ways(engines[0].emit_packets, engines[1].emit_packets, c0, ack, resend, m["start"], m["length"], m["ack"],
                   m["packets"])
    assert all((a == b).all() for a, b in zip(engines[0].emit_state(), engines[1].emit_state()))


@functools.lru_cache(maxsize=None)
def spectator_case(P, local, mp, K, max_pending, calls):
    """Stalls and bursts, a disconnect in every fifth session, acks withheld for calls 30 .. 49 in
    every fourth session of each endpoint (past max_pending: the endpoint closes)."""
    mask = sum(1 << k for k in local)
    rows = np.random.default_rng(0x57A6).integers(0, 256, (calls, S, P)).astype(np.uint8)
    arrive, events = M.schedules(S, calls, 12, 53, mask, P, disconnect_every=5)
    pushed, stop = M.pushed_table(rows, arrive, events, P, mask, 0, mp)
    confirmed = M.confirmed_table(arrive, events, pushed, mask, P)
    ack, resend = M.acks(confirmed, K, 11, silence=(30, 50))
    m = M.run(rows, arrive, events, pushed, mask, K, max_pending, F.max_packet_bytes(P, max_pending), ack, resend, stop)
    return rows, arrive, events, ack, resend, m


def test_spectator_emit_20_calls_in_one_launch_host_and_device(oracle):
    """K = 3 endpoints, max_pending_inputs 16: 60 (call, endpoint) slots in one launch, the groups
    cut where the LDS budget says, not at a call's end; calls 40 .. 59, after calls 0 .. 39."""
    P, local, mp, K, max_pending, c0 = 2, (0,), 8, 3, 16, 40
    rows, arrive, events, ack, resend, m = spectator_case(P, local, mp, K, max_pending, c0 + N)
    assert (m["status"] == M.EMIT_DISCONNECTED).sum() > 10 and (m["status"] == 0).sum() > S * K // 2
    engines = [SE.engine(P, local, 0, mp, K, cap=c0 + N, max_pending=max_pending) for _ in range(2)]
    for e in engines:
        e.add_inputs(0, rows)
        e.add_arrivals(0, arrive, events)
        e.advance_frames(c0 + N)
        SE.assert_emitted(e.emit_spectator_packets(0, c0, ack[:c0], resend[:c0]), m)
    emit_both_ways(engines[0].emit_spectator_packets, engines[1].emit_spectator_packets, c0, ack, resend, m["start"],
                   m["length"], m["notes"], m["packets"])
    SE.assert_state(engines[0], m)
    SE.assert_state(engines[1], m)
