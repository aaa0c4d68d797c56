#!/usr/bin/env python3
"""Rate of the spectator engine against the P2P engine in lockstep mode, same arrival table.

    python tools/spectator_rate.py [--sessions 65536] [--players 2] [--calls 256] [--launches 8]
                                   [--warmup 2] [--out profiles/spectator_rate.json]

Three engines run the same jittered arrival table with network stalls (one table column per
session, lags 1..7 calls, a 12-call stall about every 40 calls):
  spectator (10, 1)   max_frames_behind 10, catchup_speed 1
  spectator (10, 3)   the same, catching up 3 frames per call after a stall
  lockstep            P2PEngine(max_prediction=0) under arrival schedules, player 0 local with input
                      delay 2 (so that a call whose remote frame has arrived can advance), the
                      nearest earlier capability: at most one frame per call, nothing saved
Launches of --calls calls alternate between the engines; each is timed on the device (one event
pair around the launch).  Prints one JSON line: per engine the advanced session-frames per second,
ms per launch (median and spread over the timed launches), ns per advanced frame and the
algorithmic bytes per launch (input rows and arrival rows read, states and session words
written); and the spectator's time per advanced frame over the lockstep engine's.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def arrival_table(calls, sessions, seed, distinct=1024):
    """[calls][sessions] int32, non-decreasing per column, <= call - 1: `distinct` schedules dealt to
    the sessions in a fixed shuffle, so the lanes of a wave follow different networks."""
    rng = np.random.default_rng(seed)
    d = min(distinct, sessions)
    c = np.arange(calls)[:, None]
    upto = c - rng.integers(1, 8, (calls, d))
    for k in range(d):
        t = int(rng.integers(20, 41))
        while t < calls:
            upto[t:t + 12, k] = np.minimum(upto[t:t + 12, k], upto[t - 1, k])
            t += 12 + int(rng.integers(20, 41))
    upto = np.maximum.accumulate(np.maximum(upto, -1), axis=0).astype(np.int32)
    return np.ascontiguousarray(upto[:, rng.integers(0, d, sessions)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--players", type=int, default=2)
    ap.add_argument("--calls", type=int, default=256, help="calls per launch")
    ap.add_argument("--launches", type=int, default=8, help="timed launches per engine")
    ap.add_argument("--warmup", type=int, default=2, help="untimed launches per engine")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch  # noqa: F401  (loads the HIP runtime before the engine library)
    from ggrs_amd import P2PEngine, SpectatorEngine, build
    build.build()
    S, P, n = a.sessions, a.players, a.calls
    total = (a.warmup + a.launches) * n
    cap = 2 * n
    arrive = arrival_table(total, S, a.seed)
    rng = np.random.default_rng(a.seed + 1)

    lock = P2PEngine(S, num_players=P, local_players=(0,), input_delay=2, max_prediction=0, remote_latency=1,
                     input_capacity=cap)
    lock.set_arrival_schedule(True)
    engines = {"spectator_10_1": SpectatorEngine(S, P, 10, 1, input_capacity=cap),
               "spectator_10_3": SpectatorEngine(S, P, 10, 3, input_capacity=cap),
               "lockstep": lock}
    ms = {k: [] for k in engines}
    for j in range(a.warmup + a.launches):
        rows = rng.integers(0, 16, (n, S, P), dtype=np.uint8)
        for name, e in engines.items():  # alternate the engines launch by launch
            e.add_inputs(j * n, rows)
            e.add_arrivals(j * n, arrive[j * n:(j + 1) * n])
            e.timing_reset()
            e.advance_frames(n)
            t, launches = e.timing_read()
            assert launches == 1, (name, launches)
            if j >= a.warmup:
                ms[name].append(t)

    def frames_of(name, e):
        if name == "lockstep":
            frames, _, errors = e.sessions()
            assert (errors == 0).all(), "a lockstep session stopped"
            return int(frames.astype(np.int64).sum())
        cur, _, _, errors = e.sessions()
        assert (errors == 0).all(), "a spectator session stopped or was lost"
        return int((cur.astype(np.int64) + 1).sum())

    out = dict(sessions=S, players=P, calls_per_launch=n, timed_launches=a.launches, warmup_launches=a.warmup,
               schedule="lags 1..7 calls, 12-call stalls about every 40 calls")
    fields = 1 + 5 * P
    for name, e in engines.items():
        frames = frames_of(name, e)  # over every launch; per launch the same share
        per_launch = frames / (a.warmup + a.launches)
        med = float(np.median(ms[name]))
        words = (5 + 2 * P) if name != "lockstep" else 0  # the spectator's session words
        out[name] = dict(
            ms_per_launch=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
            advanced_frames_per_launch=round(per_launch, 1),
            session_frames_per_s=round(per_launch / (med * 1e-3), 1),
            ns_per_advanced_frame=round(med * 1e6 / per_launch, 4),
            algorithmic_bytes_per_launch=int(4 * per_launch + (8 if name != "lockstep" else 5) * n * S
                                             + 2 * 4 * (fields + words) * S))
    for k in ("spectator_10_1", "spectator_10_3"):
        out[f"{k}_time_per_frame_over_lockstep"] = round(
            out[k]["ns_per_advanced_frame"] / out["lockstep"]["ns_per_advanced_frame"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
