#!/usr/bin/env python3
"""Device time of the P2P engine's spectator emit beside packet emit, the codec's chunked batch encode
and the calls it follows, and what configuring it costs the scheduled launch.

    python tools/spectator_emit_rate.py [--sessions 65536] [--max-prediction 9] [--launches 6] [--warmup 1]
                                        [--parent-lib ggrs_amd/exp/libggrs_amd_parent.so] [--commit TEXT]
                                        [--out profiles/spectator_emit_rate.json]

2 players, player 0 local, arrival schedules, the bench's jitter schedule (synth.jitter_arrivals: a lag
of 1 .. max_prediction - 1 calls per call), 64 calls per launch, 16 pending inputs; every spectator
acks the frame the schedule delivered two calls ago.  The emitted packets stay in device memory.
  1. the emit launch, K = 1 and K = 4: two engines with packet emit and spectator emit run the same
     calls, one encoding every endpoint's packet on its own (GGRS_SPEC_EMIT_DEDUP=0), one copying the
     row of an earlier endpoint with the same last_acked (the default), launch by launch in
     alternating order; ggrs_p2p_emit_spectator_packets, ggrs_p2p_emit_packets and
     ggrs_p2p_advance_frames are timed on the device, us per call.  Every emitted packet is compared
     with ggrs_codec_encode over dense reference / pending / count arrays built from the packet emit's
     pushes and the input rows, and the chunked batch encode of those arrays (K times: the same
     packets) is timed beside the emit.
  2. the scheduled launch: three engines -- spectator emit configured, packet emit only, neither --
     run the same calls, launch by launch in turn, ggrs_p2p_advance_frames timed.
  3. with --parent-lib, the parent commit's library built beside this one: "neither" on both
     libraries in one process, launch by launch in alternating order; both medians, the pairs'
     spread (max - min of each side) and whether the medians agree within it.
Prints one JSON line with medians, minima and maxima.  Needs a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W = 16  # max_pending_inputs: the schedule's lag and the ack's


class RawEngine:
    """An any-network P2P engine with neither emit, over a library given by path (the parent's has
    not every symbol the package binds)."""

    def __init__(self, path, S, P, mp, cap):
        from ggrs_amd.p2p import P2PConfig
        L = ctypes.CDLL(path)
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.ggrs_p2p_engine_create.argtypes = [ctypes.POINTER(P2PConfig), ctypes.POINTER(vp)]
        L.ggrs_p2p_engine_destroy.argtypes = [vp]
        L.ggrs_p2p_set_arrival_schedule.argtypes = [vp, i32]
        L.ggrs_p2p_add_inputs.argtypes = [vp, i32, i32, vp]
        L.ggrs_p2p_add_arrivals.argtypes = [vp, i32, i32, vp, vp]
        L.ggrs_p2p_advance_frames.argtypes = [vp, i32]
        L.ggrs_p2p_timing_reset.argtypes = [vp]
        L.ggrs_p2p_timing_read.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i32)]
        L.ggrs_p2p_synchronize.argtypes = [vp]
        L.ggrs_p2p_read_states.argtypes = [vp, vp]
        self.L, self.h, self.S, self.P = L, vp(), S, P
        cfg = P2PConfig(S, P, 1, 0, mp, 1, 0, cap, 0, 0)
        self.ok(L.ggrs_p2p_engine_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        self.ok(L.ggrs_p2p_set_arrival_schedule(self.h, 1))

    @staticmethod
    def ok(rc):
        if rc:
            raise RuntimeError(f"engine call failed: {rc}")

    def launch(self, c0, rows, arrive):
        """-> ms of ggrs_p2p_advance_frames over the rows' calls"""
        n = rows.shape[0]
        rows, arrive = np.ascontiguousarray(rows), np.ascontiguousarray(arrive)
        self.ok(self.L.ggrs_p2p_add_inputs(self.h, c0, n, rows.ctypes.data_as(ctypes.c_void_p)))
        self.ok(self.L.ggrs_p2p_add_arrivals(self.h, c0, n, arrive.ctypes.data_as(ctypes.c_void_p), None))
        self.ok(self.L.ggrs_p2p_timing_reset(self.h))
        self.ok(self.L.ggrs_p2p_advance_frames(self.h, n))
        ms, cnt = ctypes.c_float(), ctypes.c_int32()
        self.ok(self.L.ggrs_p2p_timing_read(self.h, ctypes.byref(ms), ctypes.byref(cnt)))
        self.ok(self.L.ggrs_p2p_synchronize(self.h))
        return ms.value

    def states(self):
        out = np.zeros((self.S, 36 + 20 * self.P), np.uint8)
        self.ok(self.L.ggrs_p2p_read_states(self.h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def close(self):
        self.L.ggrs_p2p_engine_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--max-prediction", type=int, default=9)
    ap.add_argument("--launches", type=int, default=6, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library, for part 3")
    ap.add_argument("--commit", default="", help="provenance: what was built (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, _lib, build, codec, synth
    build.build()
    S, P, mp, n = a.sessions, 2, a.max_prediction, 64
    total = (a.warmup + a.launches) * n
    rows = synth.gen_inputs(0, S, total, P, synth.MODEL_HELD)
    arrive = synth.jitter_arrivals(0, S, total, mp)
    dev = torch.device("cuda:0")
    ack = np.full_like(arrive, -1)
    ack[2:] = arrive[:-2]
    rows_d = torch.from_numpy(rows).to(dev)
    arrive_d = torch.from_numpy(arrive).to(dev)
    sess = torch.arange(S, device=dev)

    def engine(spec_k, emit):
        e = P2PEngine(S, num_players=P, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=2 * n)
        e.set_arrival_schedule(True)
        if emit:
            e.set_packet_emit(W)
        if spec_k:
            e.set_spectator_emit(spec_k, W)
        return e

    def stats(v):
        return dict(median=round(1e3 * float(np.median(v)), 3), min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3))

    out = dict(sessions=S, players=P, max_prediction=mp, max_pending_inputs=W, calls_per_launch=n,
               schedule="synth.jitter_arrivals (lag 1 .. max_prediction - 1), spectators ack two calls late",
               timed_launches=a.launches, unit="us per call",
               provenance=dict(commit=a.commit, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                               hip=str(torch.version.hip), tool="tools/spectator_emit_rate.py"))

    # ---- 1. the emit launches
    for K in (1, 4):
        engines = dict(dedup=engine(K, True), each=engine(K, True))
        ack_d = torch.from_numpy(np.ascontiguousarray(np.repeat(ack[:, None, :], K, axis=1))).to(dev)
        stride = engines["dedup"].spectator_stride
        ms = dict(spectator_emit=[], spectator_emit_each_endpoint_encoded=[], packet_emit=[], advance=[], chunked_encode=[])
        bytes_out, checked = [], 0
        conf = torch.zeros((total + 1, S, P), dtype=torch.uint8, device=dev)  # the confirmed rows by frame
        conf[:total, :, 1] = rows_d[:, :, 1]
        queued = torch.zeros(S, dtype=torch.int64, device=dev)             # frames queued so far
        deliv = torch.full((S,), -1, dtype=torch.int64, device=dev)        # the newest remote frame
        for j in range(a.warmup + a.launches):
            c0 = j * n
            outs, t_spec = {}, {}
            for name in (("dedup", "each") if j % 2 == 0 else ("each", "dedup")):
                e = engines[name]
                e.add_inputs(c0, rows[c0:c0 + n])
                e.add_arrivals(c0, arrive[c0:c0 + n])
                e.timing_reset()
                e.advance_frames(n)
                t_adv, _ = e.timing_read()
                so = (torch.empty((n, K, S), dtype=torch.int32, device=dev), torch.empty((n, K, S), dtype=torch.int32, device=dev),
                      torch.empty((n, S), dtype=torch.int32, device=dev), torch.zeros((n, K, S, stride), dtype=torch.uint8, device=dev))
                torch.cuda.synchronize()
                os.environ["GGRS_SPEC_EMIT_DEDUP"] = "1" if name == "dedup" else "0"
                e.timing_reset()
                e.emit_spectator_packets(c0, n, ack_d[c0:c0 + n], None, out=so)
                t_spec[name], _ = e.timing_read()
                e.synchronize()
                outs[name] = so
            os.environ.pop("GGRS_SPEC_EMIT_DEDUP")
            e = engines["dedup"]
            po = (torch.empty((n, S), dtype=torch.int32, device=dev), torch.empty((n, S), dtype=torch.int32, device=dev),
                  torch.empty((n, S), dtype=torch.int32, device=dev),
                  torch.zeros((n, S, e.out_stride), dtype=torch.uint8, device=dev))
            e.timing_reset()
            e.emit_packets(c0, n, arrive_d[c0:c0 + n], None, out=po)
            t_emit, _ = e.timing_read()
            e.synchronize()
            start, length, notes, packets = outs["dedup"]
            body = torch.arange(stride, device=dev)[None, None, None, :] < length[..., None]
            other = outs["each"]
            assert bool((other[0] == start).all() and (other[1] == length).all()), "the two forms' packets differ"
            assert bool(((other[3] == packets) | ~body).all()), "the two forms' packets differ"
            assert bool((start == start[:, :1]).all() and (length == length[:, :1]).all())  # (equal acks)
            # the dense arrays a host would gather: a call queued a local frame exactly when packet emit sent
            # one (no resend flags, no input delay), and pushed the frames up to min(the local players' last
            # queued frame before the call, the newest remote frame)
            has = po[0] >= 0
            before = queued[None, :] + torch.cumsum(has.long(), 0) - has.long()  # frames queued before each call
            conf[torch.where(has, before, torch.full_like(before, total)), sess[None, :].expand(n, S), 0] = rows_d[c0:c0 + n, :, 0]
            queued = queued + has.sum(0)
            run = torch.cummax(torch.maximum(arrive_d[c0:c0 + n].long(), deliv[None, :]), 0)[0]
            deliv = run[-1]
            newest = torch.minimum(before - 1, run)
            st0, shas = start[:, 0].long(), start[:, 0] >= 0
            count = torch.where(shas, newest - st0 + 1, torch.zeros_like(newest)).to(torch.int32)
            assert 1 <= int(count[shas].min()) and int(count.max()) <= W
            frames = torch.clamp(st0[:, :, None] + torch.arange(W, device=dev), min=0, max=total)
            pending = conf[frames, sess[None, :, None].expand(n, S, W)].reshape(n * S, W, P).contiguous()
            ref = torch.where((st0 > 0)[:, :, None], conf[torch.clamp(st0 - 1, min=0), sess[None, :].expand(n, S)],
                              torch.zeros((n, S, P), dtype=torch.uint8, device=dev)).reshape(n * S, P).contiguous()
            count = count.reshape(-1).contiguous()
            enc, enc_len = codec.encode(ref, pending, count, stride=stride)
            enc_len = torch.where(shas.reshape(-1), enc_len, torch.zeros_like(enc_len)).reshape(n, S)
            assert bool((enc_len == length[:, 0]).all()), "the emit's packet lengths differ from ggrs_codec_encode's"
            assert bool(((packets[:, 0] == enc.reshape(n, S, stride)) | ~body[:, 0]).all()), \
                "the emit's packets differ from ggrs_codec_encode's"
            checked += K * int(shas.sum())
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                codec.encode(ref, pending, count, stride=stride, chunked=True)
            e1.record()
            e1.synchronize()
            if j >= a.warmup:
                ms["spectator_emit"].append(t_spec["dedup"] / n)
                ms["spectator_emit_each_endpoint_encoded"].append(t_spec["each"] / n)
                ms["packet_emit"].append(t_emit / n)
                ms["advance"].append(t_adv / n)
                ms["chunked_encode"].append(e0.elapsed_time(e1) / n)
                bytes_out.append(float(length.sum()) / max(1, int((start >= 0).sum())))
        for e in engines.values():
            state = e.read_spectator_emit_state()
            assert (state[3] == 0).all() and (e.sessions()[2] == 0).all(), "an endpoint closed or a session stopped"
            e.close()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out["K%d" % K] = dict({k: stats(v) for k, v in ms.items()}, out_stride=stride,
                              mean_packet_bytes=round(float(np.mean(bytes_out)), 2), packets_equal_codec_encode=checked,
                              each_over_dedup=round(med["spectator_emit_each_endpoint_encoded"] / med["spectator_emit"], 3),
                              spectator_emit_over_packet_emit=round(med["spectator_emit"] / med["packet_emit"], 3),
                              spectator_emit_over_chunked_encode=round(med["spectator_emit"] / med["chunked_encode"], 3),
                              spectator_emit_over_advance=round(med["spectator_emit"] / med["advance"], 3))
        del conf, outs, po, pending, ref, enc
        torch.cuda.empty_cache()

    # ---- 2. the scheduled launch, three configurations in turn
    engines = dict(spectator_emit=engine(4, False), packet_emit_only=engine(0, True), neither=engine(0, False))
    ms = {k: [] for k in engines}
    for j in range(a.warmup + a.launches):
        c0 = j * n
        for name, e in engines.items():
            e.add_inputs(c0, rows[c0:c0 + n])
            e.add_arrivals(c0, arrive[c0:c0 + n])
            e.timing_reset()
            e.advance_frames(n)
            t, _ = e.timing_read()
            e.synchronize()
            if j >= a.warmup:
                ms[name].append(t / n)
    ref_states = engines["neither"].states()
    assert all((e.states() == ref_states).all() for e in engines.values()), "the configurations' sessions differ"
    out["scheduled_launch"] = {k: stats(v) for k, v in ms.items()}
    out["scheduled_launch"]["spectator_emit_over_neither"] = round(float(np.median(ms["spectator_emit"]) /
                                                                         np.median(ms["neither"])), 4)
    for e in engines.values():
        e.close()

    # ---- 3. "neither" against the parent commit's library
    if a.parent_lib:
        pair = dict(this=RawEngine(_lib.LIB_PATH, S, P, mp, 2 * n), parent=RawEngine(os.path.abspath(a.parent_lib), S, P, mp, 2 * n))
        ms = {k: [] for k in pair}
        for j in range(a.warmup + a.launches):
            c0 = j * n
            for name in (("this", "parent") if j % 2 == 0 else ("parent", "this")):
                t = pair[name].launch(c0, rows[c0:c0 + n], arrive[c0:c0 + n])
                if j >= a.warmup:
                    ms[name].append(t / n)
        assert (pair["this"].states() == pair["parent"].states()).all() and (pair["this"].states() == ref_states).all(), \
            "the parent library's sessions differ"
        spread = max(max(v) - min(v) for v in ms.values())
        diff = abs(float(np.median(ms["this"])) - float(np.median(ms["parent"])))
        out["neither_vs_parent"] = dict(this=stats(ms["this"]), parent=stats(ms["parent"]),
                                        spread_us=round(1e3 * spread, 3), median_difference_us=round(1e3 * diff, 3),
                                        agree_within_spread=bool(diff <= spread), states_equal=True)
        for e in pair.values():
            e.close()
    else:
        out["neither_vs_parent"] = "not measured (no --parent-lib)"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
