#!/usr/bin/env python3
"""Device time of the P2P engine's packet feed beside the codec's decode and the calls it feeds.

    python tools/p2p_ingest_rate.py [--sessions 65536] [--max-prediction 9] [--launches 4] [--warmup 1]
                                    [--single-calls 64] [--out profiles/p2p_ingest_rate.json]

One packet-fed P2PEngine (2 players, player 0 local, arrival schedules with ggrs_p2p_set_packet_feed)
runs the bench's jitter schedule (synth.jitter_arrivals: a lag of 1 .. max_prediction - 1 calls per
call, so the remote inputs come in bursts).  The sender's packets -- every call where a session's
schedule rises, its new frames plus 0..2 re-sent ones, encoded on the device (ggrs_codec_encode) --
stay in device memory and are received in place (on_device).  Timed on the device, per call:
  (a) ingest    ggrs_p2p_receive_packets: 64 calls per launch, and one call per launch
  (b) decode    ggrs_codec_decode (the default form) over the same packets with the references the
                caller would have to supply -- the existing kernel, the floor for (a)
  (c) advance   ggrs_p2p_advance_frames on the same engine: 64 calls per launch, and one
Prints one JSON line with the medians and the ratios (a)/(b), (a)/(c).  After the timed region
every session's state is compared once against an engine fed the rows and the arrival table up
front.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W = 16  # max_packet_inputs: a burst of the schedule is at most max_prediction frames, plus the re-sent ones


def sender_packets(torch, codec, remote, arrive, prev, c0, n, stride):
    """The packets of calls c0 .. c0 + n - 1 on the device: (start [n][S] i32, length [n][S] i32,
    packets [n][S][stride] u8, ref [n*S][1] u8).  remote [calls][S] u8 and arrive [calls][S] i32 are
    device tensors, prev [S] the schedule at call c0 - 1."""
    S = arrive.shape[1]
    a = arrive[c0:c0 + n]
    before = torch.cat([prev[None, :], a[:-1]])
    rises = a > before
    calls = torch.arange(c0, c0 + n, device=a.device, dtype=torch.int32)[:, None]
    sess = torch.arange(S, device=a.device, dtype=torch.int32)[None, :]
    overlap = (calls + sess) % 3
    start = torch.clamp(before + 1 - overlap, min=0)
    start = torch.where(before < 0, torch.zeros_like(start), start)  # (the first packet starts at frame 0)
    count = torch.where(rises, a - start + 1, torch.zeros_like(a))
    assert int(count.max()) <= W
    frames = torch.clamp(start[:, :, None] + torch.arange(W, device=a.device, dtype=torch.int32), max=remote.shape[0] - 1)
    cols = sess[:, :, None].expand(n, S, W).long()
    pending = remote[frames.long(), cols].reshape(n * S, W, 1)
    ref = torch.where(start > 0, remote[torch.clamp(start - 1, min=0).long(), sess.expand(n, S).long()],
                      torch.zeros_like(start, dtype=torch.uint8)).reshape(n * S, 1)
    packets, length = codec.encode(ref.contiguous(), pending.contiguous(), count.reshape(-1).contiguous(), stride=stride)
    length = torch.where(rises.reshape(-1), length, torch.zeros_like(length))
    start = torch.where(rises, start, torch.full_like(start, -1))
    return (start.contiguous(), length.reshape(n, S).contiguous(), packets.reshape(n, S, stride).contiguous(),
            ref.contiguous())


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
    cap = 2 * n
    rows = synth.gen_inputs(0, S, total, P, synth.MODEL_HELD)
    arrive = synth.jitter_arrivals(0, S, total, mp)
    junk = rows.copy()
    junk[:, :, 1] = np.random.default_rng(1).integers(0, 256, (total, S), dtype=np.uint8)
    dev = torch.device("cuda:0")
    remote_d = torch.from_numpy(np.ascontiguousarray(rows[:, :, 1])).to(dev)
    arrive_d = torch.from_numpy(arrive).to(dev)
    stride = codec.max_packet_bytes(1, W)

    def engine(feed):
        e = P2PEngine(S, num_players=P, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=cap)
        e.set_arrival_schedule(True)
        if feed:
            e.set_packet_feed(W, stride)
        return e

    A, B = engine(True), engine(False)
    ms = dict(ingest64=[], decode64=[], advance64=[], ingest1=[], decode1=[], advance1=[])
    sizes = []

    def step(c0, k, tag, timed):
        prev = arrive_d[c0 - 1] if c0 else torch.full((S,), -1, dtype=torch.int32, device=dev)
        start, length, packets, ref = sender_packets(torch, codec, remote_d, arrive_d, prev, c0, k, stride)
        A.add_inputs(c0, junk[c0:c0 + k])
        torch.cuda.synchronize()
        A.timing_reset()
        A.receive_packets(c0, start, length, packets)
        t_ingest, _ = A.timing_read()
        # (b) the batch decode of the same packets (torch's stream; events around the one launch)
        out = torch.empty((k * S, W, 1), dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        codec.decode(ref, packets.reshape(k * S, stride), length.reshape(-1), W, out=out)
        e1.record()
        e1.synchronize()
        A.timing_reset()
        A.advance_frames(k)
        t_adv, _ = A.timing_read()
        if timed:
            ms["ingest" + tag].append(t_ingest / k)
            ms["decode" + tag].append(e0.elapsed_time(e1) / k)
            ms["advance" + tag].append(t_adv / k)
            sizes.append(float(length.sum()) / max(1, int((length > 0).sum())))
        B.add_inputs(c0, rows[c0:c0 + k])
        B.add_arrivals(c0, arrive[c0:c0 + k])
        B.advance_frames(k)

    c0 = 0
    for j in range(a.warmup + a.launches):
        step(c0, n, "64", j >= a.warmup)
        c0 += n
    for _ in range(a.single_calls):
        step(c0, 1, "1", True)
        c0 += 1

    # after the timed region: the packet-fed engine against the one fed up front, every session
    status, ack = A.packet_results(c0 - n, n)
    assert (ack == arrive[c0 - n:c0]).all() and (status >= 0).all(), "the feed dropped or stopped a packet"
    same = bool((A.states() == B.states()).all())
    fa, fb = A.sessions(), B.sessions()
    same = same and all(bool((x == y).all()) for x, y in zip(fa, fb)) and bool((fa[2] == 0).all())
    rb = A.stats()[0]
    assert same, "the packet-fed engine's states differ from the schedule-fed engine's"

    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = dict(sessions=S, players=P, max_prediction=mp, max_packet_inputs=W, packet_stride=stride,
               schedule="synth.jitter_arrivals (lag 1 .. max_prediction - 1), 0..2 re-sent frames per packet",
               mean_packet_bytes=round(float(np.mean(sizes)), 2), timed_launches=a.launches, single_calls=a.single_calls,
               states_equal_up_front_path=same, rollbacks=int(rb.astype(np.int64).sum()))
    for tag in ("64", "1"):
        i, d, v = med["ingest" + tag], med["decode" + tag], med["advance" + tag]
        out["calls_per_launch_" + tag] = dict(
            ingest_us_per_call=round(1e3 * i, 3), decode_us_per_call=round(1e3 * d, 3),
            advance_us_per_call=round(1e3 * v, 3), ingest_over_decode=round(i / d, 3),
            ingest_over_advance=round(i / v, 3),
            ingest_us_min_max=[round(1e3 * min(ms["ingest" + tag]), 3), round(1e3 * max(ms["ingest" + tag]), 3)])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
