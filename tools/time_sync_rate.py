#!/usr/bin/env python3
"""Device time of the P2P engine's time sync beside packet emit on the same calls, in both window
forms, and what configuring it costs the scheduled launch.

    python tools/time_sync_rate.py [--sessions 65536] [--max-prediction 9] [--launches 6] [--warmup 1]
                                   [--check-sessions 4096] [--parent-lib ggrs_amd/exp/libggrs_amd_parent.so]
                                   [--commit TEXT] [--out profiles/time_sync_rate.json]

2 players, player 0 local, arrival schedules, the bench's jitter schedule (synth.jitter_arrivals: a lag
of 1 .. max_prediction - 1 calls per call), 64 calls per launch, 60 fps; rtt_ms and remote_advantage as
tests/time_sync_model.input_tables draws them.  Every array stays in device memory.
  1. the time-sync launch: two engines with packet emit and time sync run the same calls, one holding
     a block's windows in LDS for the launch (GGRS_TIME_SYNC_LDS=1), one touching a push's slot in HBM
     (=0), launch by launch in alternating order; ggrs_p2p_time_sync, ggrs_p2p_emit_packets (the
     yardstick) and ggrs_p2p_advance_frames are timed on the device, us per call.  Every output of both
     forms is first compared with tests/time_sync_model.py on the first --check-sessions sessions,
     driven by the oracle's P2PSession, and the two forms with each other on all of them.
  2. the scheduled launch: three engines -- time sync configured, packet emit configured (both store
     the per-call word and run the same kernel instantiation), neither -- run the same calls, launch by
     launch in turn, ggrs_p2p_advance_frames timed.
  3. with --parent-lib, the parent commit's library built beside this one: "neither" on both
     libraries in one process, launch by launch in alternating order; both medians, the pairs'
     spread (max - min of each side) and whether the medians agree within it.
Prints one JSON line with medians, minima and maxima.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FPS, W = 60, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--max-prediction", type=int, default=9)
    ap.add_argument("--launches", type=int, default=6, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--check-sessions", type=int, default=4096, help="sessions compared with the model")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library, for part 3")
    ap.add_argument("--commit", default="", help="provenance: what was built (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, _lib, build, synth
    from oracle import oracle as O
    from spectator_emit_rate import RawEngine
    from tests import time_sync_model as T
    build.build()
    O.build()
    S, P, mp, n = a.sessions, 2, a.max_prediction, 64
    total = (a.warmup + a.launches) * n
    rows = synth.gen_inputs(0, S, total, P, synth.MODEL_HELD)
    arrive = synth.jitter_arrivals(0, S, total, mp)
    rtt, radv = T.input_tables(S, total, 5)
    dev = torch.device("cuda:0")
    arrive_d, rtt_d, radv_d = (torch.from_numpy(x).to(dev) for x in (arrive, rtt, radv))

    # the model over the checked slice, from the oracle's session per session
    C = min(a.check_sessions, S)
    advanced = np.zeros((total, C), np.uint8)
    for s in range(C):
        out = O.p2p_sched_run(rows[:, s], arrive[:, s], None, num_players=P, local_mask=1, max_prediction=mp)
        assert out["rc"] == 0
        advanced[:, s] = out["advanced"]
    cur, pushed = T.tables(advanced, 0)
    model = T.run(cur, pushed, np.maximum.accumulate(arrive[:, :C], axis=0), None, 0b10, FPS, rtt[:, :C], radv[:, :C])
    names = ("local_advantage", "frames_ahead", "skip_frames")

    def engine(time_sync, emit):
        e = P2PEngine(S, num_players=P, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=2 * n)
        e.set_arrival_schedule(True)
        if emit:
            e.set_packet_emit(W)
        if time_sync:
            e.set_time_sync(FPS)
        return e

    def stats(v):
        return dict(median=round(1e3 * float(np.median(v)), 3), min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3))

    out = dict(sessions=S, players=P, max_prediction=mp, fps=FPS, calls_per_launch=n,
               schedule="synth.jitter_arrivals (lag 1 .. max_prediction - 1); rtt_ms on 5 % of the calls, "
                        "remote_advantage on 20 %",
               timed_launches=a.launches, unit="us per call",
               provenance=dict(commit=a.commit, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                               hip=str(torch.version.hip), tool="tools/time_sync_rate.py"))

    # ---- 1. the time-sync launch, both window forms, beside packet emit
    engines = dict(lds=engine(True, True), hbm=engine(True, True))
    ms = dict(time_sync_windows_in_lds=[], time_sync_windows_in_hbm=[], packet_emit=[], advance=[])
    recommended = 0
    for j in range(a.warmup + a.launches):
        c0 = j * n
        outs, t_ts = {}, {}
        for name in (("lds", "hbm") if j % 2 == 0 else ("hbm", "lds")):
            e = engines[name]
            e.add_inputs(c0, rows[c0:c0 + n])
            e.add_arrivals(c0, arrive[c0:c0 + n])
            e.timing_reset()
            e.advance_frames(n)
            t_adv, _ = e.timing_read()
            to = tuple(torch.empty((n, S), dtype=torch.int32, device=dev) for _ in range(3))
            torch.cuda.synchronize()
            os.environ["GGRS_TIME_SYNC_LDS"] = "1" if name == "lds" else "0"
            e.timing_reset()
            e.time_sync(c0, n, rtt_d[c0:c0 + n], radv_d[c0:c0 + n], out=to)
            t_ts[name], _ = e.timing_read()
            e.synchronize()
            outs[name] = to
        os.environ.pop("GGRS_TIME_SYNC_LDS")
        e = engines["lds"]
        po = (torch.empty((n, S), dtype=torch.int32, device=dev), torch.empty((n, S), dtype=torch.int32, device=dev),
              torch.empty((n, S), dtype=torch.int32, device=dev),
              torch.zeros((n, S, e.out_stride), dtype=torch.uint8, device=dev))
        e.timing_reset()
        e.emit_packets(c0, n, arrive_d[c0:c0 + n], None, out=po)
        t_emit, _ = e.timing_read()
        e.synchronize()
        for name, x, y in zip(names, outs["lds"], outs["hbm"]):
            assert bool((x == y).all()), f"the two window forms' {name} differ"
            assert (x[:, :C].cpu().numpy() == model[name][c0:c0 + n]).all(), f"{name} differs from the model"
        recommended += int((outs["lds"][2] > 0).sum())
        if j >= a.warmup:
            ms["time_sync_windows_in_lds"].append(t_ts["lds"] / n)
            ms["time_sync_windows_in_hbm"].append(t_ts["hbm"] / n)
            ms["packet_emit"].append(t_emit / n)
            ms["advance"].append(t_adv / n)
    for e in engines.values():
        state = e.time_sync_state()
        for got, want in zip(state, model["state"]):
            assert (got[..., :C] == want).all(), "the final state differs from the model"
        assert (state[4] < 0).all() and (e.sessions()[2] == 0).all(), "an endpoint closed or a session stopped"
        e.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out["time_sync"] = dict({k: stats(v) for k, v in ms.items()}, sessions_compared_with_the_model=C,
                            wait_recommendations=recommended,
                            lds_over_hbm=round(med["time_sync_windows_in_lds"] / med["time_sync_windows_in_hbm"], 3),
                            lds_over_packet_emit=round(med["time_sync_windows_in_lds"] / med["packet_emit"], 3),
                            lds_over_advance=round(med["time_sync_windows_in_lds"] / med["advance"], 3))
    del outs, po
    torch.cuda.empty_cache()

    # ---- 2. the scheduled launch, three configurations in turn
    engines = dict(time_sync=engine(True, False), packet_emit=engine(False, True), neither=engine(False, False))
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
    spread = max(max(v) - min(v) for v in (ms["time_sync"], ms["packet_emit"]))
    diff = abs(float(np.median(ms["time_sync"])) - float(np.median(ms["packet_emit"])))
    out["scheduled_launch"].update(time_sync_vs_packet_emit=dict(spread_us=round(1e3 * spread, 3),
                                                                 median_difference_us=round(1e3 * diff, 3),
                                                                 agree_within_spread=bool(diff <= spread)),
                                   time_sync_over_neither=round(float(np.median(ms["time_sync"]) /
                                                                      np.median(ms["neither"])), 4))
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
