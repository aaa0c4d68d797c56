#!/usr/bin/env python3
"""Device time of the P2P engine's checksum comparison (ggrs_p2p_compare_reports) in both kernel forms,
beside the scheduled launch of the same calls and the host path it replaces.

    python tools/desync_compare_rate.py [--sessions 65536] [--max-prediction 8] [--launches 6] [--warmup 1]
                                        [--check-sessions 4096] [--intervals 10,1] [--cache DIR]
                                        [--prepare-only] [--commit TEXT] [--out profiles/desync_compare_rate.json]

2 players, two coupled engines (peer A: player 0 local, peer B: player 1 local), arrival schedules with
jitter and stalls past max_prediction (synth.jitter_arrivals), one match in three with one input
corrupted in flight, 64 calls per launch.  The matches are the oracle's two-peer runs
(oracle_p2p_sched_desync_pair_run) of --check-sessions sessions, repeated to fill --sessions: every
session of the timed engines desyncs as a real pair does, and every output is known.
  1. the comparison: two pairs of engines run the same calls, one pair holding a block's tables in LDS
     for the launch (GGRS_DESYNC_COMPARE_LDS=1), one touching them in HBM (=0), launch by launch in
     alternating order; the peers' rows cross with ggrs_p2p_add_remote_reports_from; peer A's
     ggrs_p2p_compare_reports and ggrs_p2p_advance_frames are timed on the device, us per call.
     Afterwards every event, summary and table of all four engines is compared with
     tests/desync_compare_model.py (exactly on the first --check-sessions sessions, the others being
     their copies).
  2. the host path: a pair of --check-sessions sessions with ggrs_amd.desync.SchedDesyncDetector; peer
     A's receive() + poll() per launch (ggrs_p2p_read_reports, then the Python loops) on the wall clock,
     us per call; its events are the model's.
--cache DIR keeps the oracle's and the model's outputs (--prepare-only: compute them and stop; needs no
GPU).  Prints one JSON line with medians, minima and maxima.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

N = 64
STATE = ("status", "n_events", "first_call", "first_frame", "first_local", "first_remote", "refused", "history",
         "pending")


def prepare(C, total, mp, interval, cache):
    """The oracle's matches of C sessions and the model's outputs for both peers, as arrays."""
    path = os.path.join(cache, f"desync_rate_{C}_{total}_{mp}_{interval}.npz") if cache else None
    if path and os.path.exists(path):
        return dict(np.load(path))
    from tests import desync_compare_model as M
    from tests.test_desync_compare_model import matches, report_rows
    rows, arr, refs = matches(interval, mp, C, total)
    assert all((o["rc"] == 0).all() for o in refs)
    out = dict(rows=rows, arr=arr)
    for k in (0, 1):
        own, peer = report_rows(refs, k), report_rows(refs, 1 - k)
        m = M.Engine(C, interval, total)
        m.add_remote_reports(0, peer["frame"], peer["checksum"], peer["local_last"])
        ev = m.compare_reports(0, own, arr[k])
        want = sorted((c, s, f, l, r) for s, o in enumerate(refs) for (p, c, f, l, r) in o["events"] if p == k)
        assert ev == want, "the model's events are not the oracle's"
        out[f"events{k}"] = np.array(ev, np.int64).reshape(-1, 5)
        for name, a in zip(STATE, m.state()):
            out[f"{name}{k}"] = np.asarray(a)
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez(path, **out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--max-prediction", type=int, default=8)
    ap.add_argument("--launches", type=int, default=6, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--check-sessions", type=int, default=4096, help="sessions of the oracle's matches")
    ap.add_argument("--intervals", default="10,1")
    ap.add_argument("--cache", default=None, help="keep the oracle's and the model's outputs here")
    ap.add_argument("--prepare-only", action="store_true")
    ap.add_argument("--commit", default="", help="provenance: what was built (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()
    S, C, mp = a.sessions, min(a.check_sessions, a.sessions), a.max_prediction
    assert S % C == 0, "--sessions must be a multiple of --check-sessions"
    tile, total = S // C, (a.warmup + a.launches) * N
    intervals = [int(x) for x in a.intervals.split(",")]
    prepared = {i: prepare(C, total, mp, i, a.cache) for i in intervals}
    if a.prepare_only:
        return

    import torch
    from ggrs_amd import P2PEngine, build
    from ggrs_amd.desync import SchedDesyncDetector
    build.build()

    def engine(k, interval, sessions, max_events=0):
        e = P2PEngine(sessions, num_players=2, local_players=(k,), max_prediction=mp, remote_latency=1,
                      input_capacity=2 * N)
        e.set_arrival_schedule(True)
        e.set_desync_detection(interval)
        if max_events:
            e.set_desync_compare(max_events)
        return e

    def stats(v):
        return dict(median=round(1e3 * float(np.median(v)), 3), min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3))

    out = dict(sessions=S, players=2, max_prediction=mp, calls_per_launch=N, timed_launches=a.launches,
               matches=f"oracle pair runs of {C} sessions, repeated {tile}x; synth.jitter_arrivals with stalls; one "
                       "match in three with a corrupted input",
               unit="us per call",
               provenance=dict(commit=a.commit, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                               hip=str(torch.version.hip), tool="tools/desync_compare_rate.py"))
    for interval in intervals:
        d = prepared[interval]
        rows = np.tile(d["rows"], (1, 1, tile, 1))
        arr = np.tile(d["arr"], (1, 1, tile))
        n_model = [len(d[f"events{k}"]) for k in (0, 1)]
        # ---- 1. both kernel forms, alternating
        pairs = {name: [engine(k, interval, S, max(1, tile * n_model[k])) for k in (0, 1)] for name in ("lds", "hbm")}
        ms = dict(tables_in_lds=[], tables_in_hbm=[], advance=[])
        for j in range(a.warmup + a.launches):
            c0 = j * N
            for name in (("lds", "hbm") if j % 2 == 0 else ("hbm", "lds")):
                engs = pairs[name]
                for k, e in enumerate(engs):
                    e.add_inputs(c0, rows[k, c0:c0 + N])
                    e.add_arrivals(c0, arr[k, c0:c0 + N])
                    e.timing_reset()
                    e.advance_frames(N)
                    t, _ = e.timing_read()
                    if k == 0 and j >= a.warmup:
                        ms["advance"].append(t / N)
                for k in (0, 1):
                    engs[k].add_remote_reports_from(engs[1 - k], c0, N)
                for e in engs:
                    e.synchronize()
                os.environ["GGRS_DESYNC_COMPARE_LDS"] = "1" if name == "lds" else "0"
                for k, e in enumerate(engs):
                    e.timing_reset()
                    e.compare_reports(c0, N, wait=False)
                    t, _ = e.timing_read()
                    if k == 0 and j >= a.warmup:
                        ms["tables_in_" + name].append(t / N)
            os.environ.pop("GGRS_DESYNC_COMPARE_LDS")
        for name, engs in pairs.items():
            for k, e in enumerate(engs):
                assert e.compare_reports(total, 0) == tile * n_model[k], f"{name}: the event count differs"
                ev = np.stack([x.astype(np.int64) for x in e.desync_events()], axis=1)
                first = ev[ev[:, 1] < C]
                first = first[np.lexsort(first.T[::-1])]
                assert (first == d[f"events{k}"]).all(), f"{name}: the events differ from the model"
                for nm, got in zip(STATE, e.desync_state()):
                    assert (got == np.tile(d[f"{nm}{k}"], tile)).all(), f"{name}: {nm} differs from the model"
                assert (e.sessions()[2] == 0).all(), "a session stopped"
                e.close()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res = dict({k: stats(v) for k, v in ms.items()}, events_per_peer=[tile * n for n in n_model],
                   sessions_compared_with_the_model=C,
                   lds_over_hbm=round(med["tables_in_lds"] / med["tables_in_hbm"], 3),
                   lds_over_advance=round(med["tables_in_lds"] / med["advance"], 3))
        torch.cuda.empty_cache()
        # ---- 2. the host path at C sessions
        engs = [engine(k, interval, C) for k in (0, 1)]
        dets = [SchedDesyncDetector(e, interval) for e in engs]
        host, events = [], []
        for j in range(a.warmup + a.launches):
            c0 = j * N
            for k, e in enumerate(engs):
                e.add_inputs(c0, d["rows"][k, c0:c0 + N])
                e.add_arrivals(c0, d["arr"][k, c0:c0 + N])
                dets[k].note_arrivals(c0, d["arr"][k, c0:c0 + N])
                e.advance_frames(N)
                e.synchronize()
            sent = dets[1].outgoing()
            t0 = time.perf_counter()
            dets[0].receive(*sent)
            events += dets[0].poll()
            t1 = time.perf_counter()
            if j >= a.warmup:
                host.append(1e3 * (t1 - t0) / N)
        got = sorted((ev.call, ev.session, ev.frame, ev.local_checksum, ev.remote_checksum) for ev in events)
        assert got == [tuple(r) for r in d["events0"].tolist()], "the host detector's events differ from the model"
        for e in engs:
            e.close()
        res["host_path"] = dict(stats(host), sessions=C, what="SchedDesyncDetector.receive + poll of peer A, wall clock")
        res["host_path_over_lds_per_session"] = round(float(np.median(host)) / C / (med["tables_in_lds"] / S), 1)
        out[f"interval_{interval}"] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
