#!/usr/bin/env python3
"""Device time of the spectator engine's packet feed beside the kernels it can be compared with.

    python tools/spectator_ingest_rate.py [--sessions 65536] [--launches 4] [--warmup 1]
                                          [--out profiles/spectator_ingest_rate.json]

One packet-fed SpectatorEngine (2 players, max_frames_behind 10, catchup_speed 3) follows hosts whose
packets arrive by tools/spectator_rate.py's table (jittered lags of 1..7 calls, a 12-call stall about
every 40 calls, the sessions of a wave on different networks).  The sender's packets -- every call
where a session's schedule rises, its new frames plus 0..2 re-sent ones, encoded on the device
(ggrs_codec_encode) -- stay in device memory and are received in place (on_device), 64 calls per
launch.  Timed on the device in the same run, launch by launch in turn, per call:
  ingest            ggrs_spectator_receive_packets
  ingest_lockstep   the same for an engine whose hosts all follow one schedule: every lane of a wave
                    stores into the same input row, so the difference to `ingest` is what the
                    scattered row stores of hosts at different frames cost
  spectator_feed    ggrs_spectator_advance_frames of the packet-fed engine (the kFeed kernel form:
                    per-session input windows)
  spectator_table   ggrs_spectator_advance_frames of an engine fed the same rows and recv_upto through
                    add_inputs / add_arrivals (the kernel as it was before the feed)
  decode_chunked    ggrs_codec_decode_chunked over the same packets, moved into its chunked layout
                    beforehand (untimed), with the references the caller would have to supply: the
                    existing batch decode
  p2p_ingest        ggrs_p2p_receive_packets of a P2PEngine with two remote players, given the same
                    packets (same count, same bytes)
Prints one JSON line with the medians (and min, max) in us per call and the ratios.  After the timed
region the packet-fed engine is compared once with the table-fed one, every session.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

W = 32  # max_packet_inputs: a burst of the schedule is at most 12 + 7 frames, plus the re-sent ones
MP = 8  # the hosts' max_prediction


def to_chunked(torch, packets, length):
    """packets [n][S][stride] u8, length [n][S] i32 -> the same packets in the codec's chunked layout
    (ggrs_amd.codec.chunk_offsets: each block of 256 packets back to back, dword-padded, at 256 * block
    * stride; a length outside [1, stride] takes none), [n * S][stride] u8.  The chunked encoder
    itself does not take packets of this size."""
    n, S, stride = packets.shape
    assert S % 256 == 0
    out = torch.zeros((n, S * stride), dtype=torch.uint8, device=packets.device)
    j = torch.arange(stride, device=packets.device)
    base = (torch.arange(S, device=packets.device) // 256) * (256 * stride)
    for k in range(n):  # (call by call: the index tensors stay small)
        ln = length[k].long()
        cb = torch.where((ln >= 1) & (ln <= stride), (ln + 3) & ~3, torch.zeros_like(ln))
        ends = torch.cumsum(cb.reshape(-1, 256), 1).reshape(-1)
        mask = j[None, :] < cb[:, None]
        out[k][((base + ends - cb)[:, None] + j[None, :])[mask]] = packets[k][mask]
    return out.reshape(n * S, stride)


def sender_packets(torch, codec, rows, arrive, prev, c0, n, stride):
    """The packets of calls c0 .. c0 + n - 1 on the device: (start [n][S] i32, length [n][S] i32,
    packets [n][S][stride] u8, ref [n*S][P] u8, count [n][S] i32).  rows [frames][S][P] u8 and arrive
    [calls][S] i32 are device tensors, prev [S] the schedule at call c0 - 1."""
    S, P = rows.shape[1], rows.shape[2]
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
    frames = torch.clamp(start[:, :, None] + torch.arange(W, device=a.device, dtype=torch.int32), max=rows.shape[0] - 1)
    cols = sess[:, :, None].expand(n, S, W).long()
    pending = rows[frames.long(), cols].reshape(n * S, W, P)
    ref = torch.where((start > 0)[:, :, None], rows[torch.clamp(start - 1, min=0).long(), sess.expand(n, S).long()],
                      torch.zeros((n, S, P), dtype=torch.uint8, device=a.device)).reshape(n * S, P)
    packets, length = codec.encode(ref.contiguous(), pending.contiguous(), count.reshape(-1).contiguous(), stride=stride)
    length = torch.where(rises.reshape(-1), length, torch.zeros_like(length))
    start = torch.where(rises, start, torch.full_like(start, -1))
    return (start.contiguous(), length.reshape(n, S).contiguous(), packets.reshape(n, S, stride).contiguous(),
            ref.contiguous(), count.contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=4, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, SpectatorEngine, build, codec
    from spectator_rate import arrival_table
    build.build()
    S, P, n = a.sessions, 2, 64
    total = (a.warmup + a.launches) * n
    cap = 2 * n
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 16, (total, S, P), dtype=np.uint8)
    arrive = arrival_table(total, S, 1)
    lock = np.ascontiguousarray(np.repeat(arrive[:, :1], S, axis=1))  # every host on session 0's schedule
    junk = rng.integers(0, 256, (total, S, 3), dtype=np.uint8)
    dev = torch.device("cuda:0")
    rows_d = torch.from_numpy(rows).to(dev)
    arrive_d, lock_d = torch.from_numpy(arrive).to(dev), torch.from_numpy(lock).to(dev)
    stride = codec.max_packet_bytes(P, W)

    def spectator(feed):
        e = SpectatorEngine(S, P, 10, 3, input_capacity=cap)
        if feed:
            e.set_packet_feed(MP, W, stride)
        return e

    fed, fed_lock, table = spectator(True), spectator(True), spectator(False)
    p2p = P2PEngine(S, num_players=3, local_players=(0,), max_prediction=MP + 1, remote_latency=1, input_capacity=cap)
    p2p.set_arrival_schedule(True)
    p2p.set_packet_feed(W, stride)
    ms = dict(ingest=[], ingest_lockstep=[], spectator_feed=[], spectator_table=[], decode_chunked=[], p2p_ingest=[])
    sizes, counts = [], []
    decode_ok = True

    def timed(e, call, *args):
        e.timing_reset()
        call(*args)
        t, launches = e.timing_read()
        assert launches == 1, launches
        return t / n

    for j in range(a.warmup + a.launches):
        c0 = j * n
        none = torch.full((S,), -1, dtype=torch.int32, device=dev)
        pk = sender_packets(torch, codec, rows_d, arrive_d, arrive_d[c0 - 1] if c0 else none, c0, n, stride)
        pk_lock = sender_packets(torch, codec, rows_d, lock_d, lock_d[c0 - 1] if c0 else none, c0, n, stride)
        chunked = to_chunked(torch, pk[2], pk[1])
        p2p.add_inputs(c0, junk[c0:c0 + n])
        table.add_inputs(c0, rows[c0:c0 + n])
        table.add_arrivals(c0, arrive[c0:c0 + n])
        torch.cuda.synchronize()
        t = {}
        t["ingest"] = timed(fed, fed.receive_packets, c0, *pk[:3])
        t["ingest_lockstep"] = timed(fed_lock, fed_lock.receive_packets, c0, *pk_lock[:3])
        t["p2p_ingest"] = timed(p2p, p2p.receive_packets, c0, *pk[:3])
        out = torch.empty((n * S, W, P), dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, cnt, st = codec.decode(pk[3], chunked, pk[1].reshape(-1), W, chunked=True, out=out)
        e1.record()
        e1.synchronize()
        has = pk[1].reshape(-1) > 0  # (a packet of length 0 is no packet: the decode reports it as malformed)
        decode_ok = decode_ok and bool((st[has] == 0).all()) and bool((cnt[has] == pk[4].reshape(-1)[has]).all())
        t["decode_chunked"] = e0.elapsed_time(e1) / n
        t["spectator_feed"] = timed(fed, fed.advance_frames, n)
        t["spectator_table"] = timed(table, table.advance_frames, n)
        fed_lock.advance_frames(n)
        p2p.advance_frames(n)
        if j >= a.warmup:
            for k, v in t.items():
                ms[k].append(v)
            sizes.append(float(pk[1].sum()) / max(1, int((pk[1] > 0).sum())))
            counts.append(float((pk[1] > 0).sum()) / (n * S))

    # after the timed region: the packet-fed engine against the table-fed one, every session
    status, ack = fed.read_packet_results(total - n, n)
    assert (ack == arrive[total - n:]).all() and (status >= 0).all(), "the feed dropped or stopped a packet"
    same = bool((fed.states() == table.states()).all())
    same = same and all(bool((x == y).all()) for x, y in zip(fed.sessions(), table.sessions()))
    assert same, "the packet-fed engine's sessions differ from the table-fed engine's"
    assert (fed.sessions()[3] == 0).all(), "a spectator stopped or was lost"
    assert (fed_lock.read_packet_results(total - n, n)[1] == lock[total - n:]).all()
    p2p_same = bool((p2p.packet_results(total - n, n)[1] == arrive[total - n:]).all())  # it delivered as much

    def us(k):
        return round(1e3 * float(np.median(ms[k])), 3)

    out = dict(sessions=S, players=P, calls_per_launch=n, timed_launches=a.launches, warmup_launches=a.warmup,
               max_prediction=MP, max_packet_inputs=W, packet_stride=stride, input_capacity=cap,
               schedule="tools/spectator_rate.py arrival_table: lags 1..7 calls, 12-call stalls about every 40 calls; "
                        "0..2 re-sent frames per packet",
               mean_packet_bytes=round(float(np.mean(sizes)), 2), packets_per_session_call=round(float(np.mean(counts)), 3),
               sessions_equal_table_fed_engine=same, p2p_feed_delivered_the_same_frames=p2p_same,
               decode_chunked_decoded_every_packet=decode_ok)
    for k in ms:
        out[k + "_us_per_call"] = us(k)
        out[k + "_us_min_max"] = [round(1e3 * min(ms[k]), 3), round(1e3 * max(ms[k]), 3)]
    out["spectator_feed_over_table"] = round(us("spectator_feed") / us("spectator_table"), 3)
    out["ingest_over_p2p_ingest"] = round(us("ingest") / us("p2p_ingest"), 3)
    out["ingest_over_decode_chunked"] = round(us("ingest") / us("decode_chunked"), 3)
    out["ingest_over_ingest_lockstep"] = round(us("ingest") / us("ingest_lockstep"), 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
