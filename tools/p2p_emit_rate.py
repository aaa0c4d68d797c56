#!/usr/bin/env python3
"""Device time of the P2P engine's packet emit beside the codec's encode and the calls it follows.

    python tools/p2p_emit_rate.py [--sessions 65536] [--max-prediction 9] [--launches 4] [--warmup 1]
                                  [--single-calls 64] [--out profiles/p2p_emit_rate.json]

One P2PEngine (2 players, player 0 local, arrival schedules with ggrs_p2p_set_packet_emit, 16 pending
inputs) runs the bench's jitter schedule (synth.jitter_arrivals: a lag of 1 .. max_prediction - 1
calls per call); the peer's acks lag as its inputs do (ack_in[c] = the schedule's frame of call c).
The emitted packets stay in device memory (on_device).  Timed on the device, per call:
  (a) emit      ggrs_p2p_emit_packets: 64 calls per launch, and one call per launch
  (b) encode    ggrs_codec_encode over the same packets from dense reference / pending / count arrays
                built beforehand -- the floor for (a), and today's path without its host gather
  (c) advance   ggrs_p2p_advance_frames on the same engine: 64 calls per launch, and one
Prints one JSON line with the medians and the ratios (a)/(b), (a)/(c).  After each timed launch every
emitted packet is compared with (b)'s.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W = 16  # max_pending_inputs: the schedule's lag and the ack's, at most max_prediction - 1 each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--max-prediction", type=int, default=9)
    ap.add_argument("--launches", type=int, default=4, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--single-calls", type=int, default=64, help="timed one-call launches after them")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, build, codec, synth
    build.build()
    S, P, mp, n = a.sessions, 2, a.max_prediction, 64
    total = (a.warmup + a.launches) * n + a.single_calls
    rows = synth.gen_inputs(0, S, total, P, synth.MODEL_HELD)
    arrive = synth.jitter_arrivals(0, S, total, mp)
    dev = torch.device("cuda:0")
    local_d = torch.from_numpy(np.ascontiguousarray(rows[:, :, 0])).to(dev)
    ack_d = torch.from_numpy(arrive).to(dev)
    stride = codec.max_packet_bytes(1, W)
    A = P2PEngine(S, num_players=P, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=2 * n)
    A.set_arrival_schedule(True)
    A.set_packet_emit(W, stride)

    sess = torch.arange(S, device=dev)
    sent = torch.zeros((total + 1, S), dtype=torch.uint8, device=dev)  # the byte sent for each frame
    queued = torch.zeros(S, dtype=torch.int64, device=dev)             # frames queued so far
    ms = dict(emit64=[], encode64=[], advance64=[], emit1=[], encode1=[], advance1=[])
    sizes = []
    packets_checked = 0

    def step(c0, k, tag, timed):
        nonlocal queued, packets_checked
        A.add_inputs(c0, rows[c0:c0 + k])
        A.add_arrivals(c0, arrive[c0:c0 + k])
        A.timing_reset()
        A.advance_frames(k)
        t_adv, _ = A.timing_read()
        out = (torch.empty((k, S), dtype=torch.int32, device=dev), torch.empty((k, S), dtype=torch.int32, device=dev),
               torch.empty((k, S), dtype=torch.int32, device=dev), torch.zeros((k, S, stride), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        A.timing_reset()
        A.emit_packets(c0, k, ack_d[c0:c0 + k], None, out=out)
        t_emit, _ = A.timing_read()
        A.synchronize()
        start, length, ack, packets = out
        # (b) the dense arrays a host would gather: a call sent a packet exactly when it queued a frame
        # (no resend flags), the frames are consecutive from 0 (no input delay)
        has = start >= 0
        newest = queued[None, :] + torch.cumsum(has.long(), 0) - 1  # the frame queued by each sending call
        sent[torch.where(has, newest, torch.full_like(newest, total)), sess[None, :].expand(k, S)] = local_d[c0:c0 + k]
        queued = queued + has.sum(0)
        count = torch.where(has, newest - start + 1, torch.zeros_like(newest)).to(torch.int32)
        assert int(count.max()) <= W
        frames = torch.clamp(start.long()[:, :, None] + torch.arange(W, device=dev), min=0, max=total)
        cols = sess[None, :, None].expand(k, S, W)
        pending = sent[frames, cols].reshape(k * S, W, 1).contiguous()
        ref = torch.where(start > 0, sent[torch.clamp(start.long() - 1, min=0), sess[None, :].expand(k, S)],
                          torch.zeros_like(start, dtype=torch.uint8)).reshape(k * S, 1).contiguous()
        count = count.reshape(-1).contiguous()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enc, enc_len = codec.encode(ref, pending, count, stride=stride)
        e1.record()
        e1.synchronize()
        enc_len = torch.where(has.reshape(-1), enc_len, torch.zeros_like(enc_len)).reshape(k, S)
        assert bool((enc_len == length).all()), "emit's packet lengths differ from ggrs_codec_encode's"
        body = torch.arange(stride, device=dev)[None, None, :] < length[:, :, None]
        assert bool(((packets == enc.reshape(k, S, stride)) | ~body).all()), "emit's packets differ from ggrs_codec_encode's"
        packets_checked += int(has.sum())
        if timed:
            ms["emit" + tag].append(t_emit / k)
            ms["encode" + tag].append(e0.elapsed_time(e1) / k)
            ms["advance" + tag].append(t_adv / k)
            sizes.append(float(length.sum()) / max(1, int(has.sum())))

    c0 = 0
    for j in range(a.warmup + a.launches):
        step(c0, n, "64", j >= a.warmup)
        c0 += n
    for _ in range(a.single_calls):
        step(c0, 1, "1", True)
        c0 += 1

    last_acked, pending, status, closed = A.emit_state()
    assert (status == 0).all() and (A.sessions()[2] == 0).all(), "a stream closed or a session stopped"
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = dict(sessions=S, players=P, max_prediction=mp, max_pending_inputs=W, out_stride=stride,
               schedule="synth.jitter_arrivals (lag 1 .. max_prediction - 1), acks lagging the same",
               mean_packet_bytes=round(float(np.mean(sizes)), 2), timed_launches=a.launches, single_calls=a.single_calls,
               packets_equal_codec_encode=packets_checked, max_pending_at_end=int(pending.max()))
    for tag in ("64", "1"):
        i, d, v = med["emit" + tag], med["encode" + tag], med["advance" + tag]
        out["calls_per_launch_" + tag] = dict(
            emit_us_per_call=round(1e3 * i, 3), encode_us_per_call=round(1e3 * d, 3),
            advance_us_per_call=round(1e3 * v, 3), emit_over_encode=round(i / d, 3), emit_over_advance=round(i / v, 3),
            emit_us_min_max=[round(1e3 * min(ms["emit" + tag]), 3), round(1e3 * max(ms["emit" + tag]), 3)])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
