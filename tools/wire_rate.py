#!/usr/bin/env python3
"""Device time of the wire envelope (ggrs_wire_unpack / ggrs_wire_pack) beside the units it feeds.

    python tools/wire_rate.py [--sessions 65536] [--launches 6] [--warmup 1] [--check-sessions 4096]
                              [--out profiles/wire_rate.json]

One P2PEngine (2 players, player 0 local, arrival schedules with the packet feed and packet emit, 16
inputs a packet) runs the bench's jitter schedule (synth.jitter_arrivals).  Its peer's traffic is that
of tools/p2p_ingest_rate.py -- every call where a session's schedule rises, its new frames plus 0..2
re-sent ones, encoded on the device -- with the peer's acks lagging as its inputs do, a QualityReport
at every 12th call, a QualityReply two calls later and a ChecksumReport at every 16th call.  Per
launch of 64 calls, everything in device memory:
  pack      ggrs_wire_pack of the peer's arrays into datagrams [64][4][S][dgram_stride]
  unpack    ggrs_wire_unpack of those datagrams (M = 4), every output
  ingest    ggrs_p2p_receive_packets of unpack's start_frame / packet_len / packets
  advance   ggrs_p2p_advance_frames, the scheduled launch of the same calls
  emit      ggrs_p2p_emit_packets with unpack's ack_in
Before the timed launches every output of both directions is compared with tests/wire_model.py on the
first --check-sessions sessions, and after every launch unpack's packet arrays are compared with the
arrays packed, every session.  Prints one JSON line: median (min - max) us per call of each, the
ratios to ingest and emit, and the bytes each direction has to move per call over its time as a
fraction of the 8 TB/s HBM peak.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

W = 16            # inputs a packet, both directions
HBM_PEAK = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--max-prediction", type=int, default=9)
    ap.add_argument("--launches", type=int, default=6, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--check-sessions", type=int, default=4096, help="sessions compared with the model first")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, build, codec, synth, wire
    from p2p_ingest_rate import sender_packets
    from tests import wire_model as M
    build.build()
    S, P, mp, n, ns = a.sessions, 2, a.max_prediction, 64, 2
    total = (a.warmup + a.launches) * n
    rows = synth.gen_inputs(0, S, total, P, synth.MODEL_HELD)
    arrive = synth.jitter_arrivals(0, S, total, mp)
    dev = torch.device("cuda:0")
    remote_d = torch.from_numpy(np.ascontiguousarray(rows[:, :, 1])).to(dev)
    arrive_d = torch.from_numpy(arrive).to(dev)
    stride = codec.max_packet_bytes(1, W)
    dstride = wire.max_datagram_bytes(ns, stride)
    A = P2PEngine(S, num_players=P, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=2 * n)
    A.set_arrival_schedule(True)
    A.set_packet_feed(W, stride)
    A.set_packet_emit(W, stride)

    rng = np.random.default_rng(9)
    magic = torch.from_numpy(rng.integers(0, 1 << 16, S).astype(np.uint16).view(np.int16)).to(dev)
    now_all = (1 << 41) + 16 * np.arange(total, dtype=np.int64)
    ones = torch.ones((n, S), dtype=torch.uint8, device=dev)
    calls = torch.arange(total, device=dev)
    ms = dict(pack=[], unpack=[], ingest=[], advance=[], emit=[])
    bytes_in, bytes_out = [], []
    prev = torch.full((S,), -1, dtype=torch.int32, device=dev)
    checked = dict(sessions=0, datagrams=0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1)

    def peer_arrays(c0):
        """What the peer's units would hand its pack for calls c0 .. c0 + n - 1."""
        start, length, packets, _ = sender_packets(torch, codec, remote_d, arrive_d, prev, c0, n, stride)
        c = calls[c0:c0 + n, None]
        every = lambda k, off=0: ((c % k == off) & (ones > 0)).to(torch.uint8).contiguous()  # noqa: E731
        now = torch.from_numpy(now_all[c0:c0 + n]).to(dev)
        ping = torch.zeros((n, S, 16), dtype=torch.uint8, device=dev)
        ping[:, :, :8] = (now[:, None] - 32).contiguous().view(torch.uint8).reshape(n, 1, 8)
        return now, dict(
            start_frame=start, packet_len=length, ack_frame=arrive_d[c0:c0 + n].contiguous(), packets=packets,
            send_ack=ones, send_report=every(12), local_advantage=((c + torch.arange(S, device=dev)) % 7 - 3).to(torch.int32),
            kinds=(every(12, 2) << M.QUALITY_REPORT).contiguous(), ping=ping,
            report_frame=torch.where(every(16) > 0, (c - c % 16).to(torch.int32), -1).to(torch.int32).contiguous(),
            report_checksum=((c * 31 + torch.arange(S, device=dev)) & 0xFFFF).to(torch.int16).contiguous())

    def check_with_model(now, arrays, dg, ln, out):
        k = min(a.check_sessions, S)
        now_h = now.cpu().numpy().view(np.uint64)
        host = lambda t: t.cpu().numpy()  # noqa: E731
        u16 = lambda x: x.view(np.uint16) if x.dtype == np.int16 else x  # noqa: E731
        sub = {}
        for name, t in arrays.items():
            x = host(t)
            sub[name] = u16(np.ascontiguousarray(x[:, :k] if name != "last_frame" else x[:, :, :k]))
        mdg, mln = M.pack_batch(u16(host(magic))[:k], now_h, ns, stride, dstride, **sub)
        gdg, gln = host(dg)[:, :, :k], host(ln)[:, :, :k]
        assert (gln == mln).all(), "pack's lengths differ from the model's"
        assert (np.where(np.arange(dstride) < gln[..., None], gdg, 0) == mdg).all(), "pack's datagrams differ from the model's"
        want = M.unpack_batch(np.ascontiguousarray(gdg), np.ascontiguousarray(gln), now_h, ns, 0b10, 0, stride)
        for name, m in want.items():
            g = u16(host(out[name]))
            g = g[:, :, :k] if name in ("slot_status", "last_frame") else g[:, :k]
            if name == "packets":
                g = np.where(np.arange(stride) < want["packet_len"][..., None], g, 0)
            assert (g == m).all(), f"unpack's {name} differs from the model's"
        checked["sessions"], checked["datagrams"] = k, int((mln > 0).sum())

    c0 = 0
    for j in range(a.warmup + a.launches):
        now, arrays = peer_arrays(c0)
        (dg, ln), t_pack = timed(lambda: wire.pack(magic, now, ns, stride, **arrays))
        out, t_unpack = timed(lambda: wire.unpack(dg, ln, now, ns, 0b10, stride, first_call=c0))
        if j == 0:
            check_with_model(now, arrays, dg, ln, wire.unpack(dg, ln, now, ns, 0b10, stride, first_call=0))
        # what came out is what went in, every session
        has = arrays["start_frame"] >= 0
        assert bool((out["start_frame"] == arrays["start_frame"]).all()) and bool((out["ack_in"] == arrays["ack_frame"]).all())
        assert bool((out["packet_len"] == arrays["packet_len"]).all())
        body = torch.arange(stride, device=dev)[None, None, :] < arrays["packet_len"][:, :, None]
        assert bool(((out["packets"] == arrays["packets"]) | ~body).all())
        A.add_inputs(c0, rows[c0:c0 + n])
        torch.cuda.synchronize()
        A.timing_reset()
        A.receive_packets(c0, out["start_frame"], out["packet_len"], out["packets"], out["events"])
        t_ingest, _ = A.timing_read()
        A.timing_reset()
        A.advance_frames(n)
        t_adv, _ = A.timing_read()
        emitted = (torch.empty((n, S), dtype=torch.int32, device=dev), torch.empty((n, S), dtype=torch.int32, device=dev),
                   torch.empty((n, S), dtype=torch.int32, device=dev), torch.zeros((n, S, stride), dtype=torch.uint8, device=dev))
        A.timing_reset()
        A.emit_packets(c0, n, out["ack_in"], None, out=emitted)
        t_emit, _ = A.timing_read()
        A.synchronize()
        if j >= a.warmup:
            for key, t in (("pack", t_pack), ("unpack", t_unpack), ("ingest", t_ingest), ("advance", t_adv), ("emit", t_emit)):
                ms[key].append(t / n)
            dgram_bytes = float(ln.sum()) / n
            packet_bytes = float(arrays["packet_len"].sum()) / n
            # the bytes each direction has to move per call: the datagrams' own bytes and their lengths, the
            # packets' bytes, and every per-session word of the other arrays
            words_out = 4 * 4 + 4 * 8 + 1 * 3 + 2 + 16 + 4 * ns  # slot_status and unpack's [n][S] outputs
            words_in = 4 * 6 + 1 * 4 + 2 + 16                    # pack's inputs as given here
            bytes_in.append(dgram_bytes + 4 * 4 * S + packet_bytes + words_out * S)
            bytes_out.append(dgram_bytes + 4 * 4 * S + packet_bytes + words_in * S)
        prev = arrive_d[c0 + n - 1]
        c0 += n

    assert (A.sessions()[2] == 0).all(), "a session stopped"
    stat = lambda v: dict(median=round(1e3 * float(np.median(v)), 3), min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3))  # noqa: E731
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(sessions=S, players=P, max_prediction=mp, inputs_per_packet=W, packet_stride=stride, dgram_stride=dstride,
               slots_per_poll=4, calls_per_launch=n, timed_launches=a.launches,
               traffic="tools/p2p_ingest_rate.py's sender packets on synth.jitter_arrivals, an ack every call, a "
                       "QualityReport every 12th call, a QualityReply two calls later, a ChecksumReport every 16th",
               compared_with_model=checked, us_per_call={k: stat(v) for k, v in ms.items()},
               unpack_over_ingest=round(med["unpack"] / med["ingest"], 3), pack_over_emit=round(med["pack"] / med["emit"], 3),
               unpack_over_advance=round(med["unpack"] / med["advance"], 3),
               pack_over_advance=round(med["pack"] / med["advance"], 3),
               unpack_bytes_per_call=round(float(np.median(bytes_in))), pack_bytes_per_call=round(float(np.median(bytes_out))),
               unpack_fraction_of_hbm_peak=round(float(np.median(bytes_in)) / (med["unpack"] * 1e-3) / HBM_PEAK, 4),
               pack_fraction_of_hbm_peak=round(float(np.median(bytes_out)) / (med["pack"] * 1e-3) / HBM_PEAK, 4))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
