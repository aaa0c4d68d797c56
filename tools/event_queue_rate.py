#!/usr/bin/env python3
"""Device time of the P2P engine's event queue -- collect with K = 0 and K = 4 spectator endpoints, and
the drain -- beside the endpoint poll of the same calls on the same run, and the scheduled launch of
this tree against the parent commit's library.

    python tools/event_queue_rate.py [--sessions 65536] [--launches 6] [--warmup 1] [--check-sessions 1024]
                                     [--parent-lib ggrs_amd/exp/libggrs_amd_parent.so] [--unit-text FILE]
                                     [--commit TEXT] [--out profiles/event_queue_rate.json]

2 players, player 0 local, arrival schedules, 64 calls per launch, every array in device memory.  The
rows a collect takes, and their density (a live server's: events are rare, Inputs are not):
  net_events       the endpoint poll's own output over tools/endpoint_poll_rate.py's clock and links (a
                   260 ms and a 700 ms stall in every launch: the 700 ms one interrupts every quiet link,
                   which resumes at its next message; every 16th link silent for 20 calls, every 64th for
                   good, which times out);
  handled_inputs   1 where the session's arrival row rises (an Input was decoded): most calls;
  events, disc_req every 512th session asks for its disconnect once, at call 200;
  skip_frames      a WaitRecommendation every 240 calls per session (RECOMMENDATION_INTERVAL), phases spread;
  desync records   every third session raises one DesyncDetected every 16 calls (4 per launch), given as
                   a shuffled list;
  spec_net_events  (K = 4) every 16th spectator link interrupted at the 700 ms stall and resumed 3 calls on.
The queues are drained after every launch (into device arrays), so a drain hands over one launch's
events.  Collect and the poll are timed on the device (the engine's event pair), us per call; the
drain waits for its launches and is timed on the host around the call, us per drain.  The queues of the
first --check-sessions sessions are first compared with tests/event_queue_model.py, record by record.
With --parent-lib: the scheduled launch of an engine that configures no unit, on both libraries in one
process, launch by launch in alternating order; the difference of the medians against the pairs' own
spread.  --unit-text: a file whose text says how the other units' device code compares with the
parent's (recorded as given).  Prints one JSON line.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

TIMEOUT, NOTIFY, CAPACITY, K4 = 2000, 500, 128, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--max-prediction", type=int, default=9)
    ap.add_argument("--launches", type=int, default=6, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--check-sessions", type=int, default=1024, help="sessions compared with the model")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library, for the A/B")
    ap.add_argument("--unit-text", default=None, help="a text file: the other units' device code against the parent's")
    ap.add_argument("--commit", default="", help="provenance: what was built (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, _lib, build, synth
    from spectator_emit_rate import RawEngine
    from tests import endpoint_poll_model as P
    from tests import event_queue_model as M
    build.build()
    S, mp, n = a.sessions, a.max_prediction, 64
    total = (a.warmup + a.launches) * n
    arrive = synth.jitter_arrivals(0, S, total, mp)
    arrive[70:90, 3::16] = arrive[69, 3::16]
    arrive[100:, 7::64] = arrive[99, 7::64]
    rng = np.random.default_rng(0xE12)
    step = rng.choice((8, 16, 17, 24), total)
    step[20::n], step[45::n], step[0] = 260, 700, 0
    start = 5 * (1 << 32) - 1000
    now = (np.uint64(start) + np.cumsum(step).astype(np.uint64)).astype(np.uint64)
    rise = np.diff(arrive, axis=0, prepend=-1) > 0
    kinds = np.where(rise, P.K_INPUT, 0).astype(np.uint8)
    kinds[~rise & (rng.random((total, S)) < 0.1)] = P.K_INPUT_ACK | P.K_QUALITY_REPLY
    kinds[70:90, 3::16] = 0
    kinds[100:, 7::64] = 0
    handled = rise.astype(np.uint8)
    events = np.zeros((total, S), np.uint8)
    disc_req = np.zeros((total, S), np.uint8)
    if total > 200:
        events[200, 5::512] = 2
        disc_req[200, 5::512] = 1
    calls = np.arange(total)[:, None]
    skip = np.where((calls + 7 * np.arange(S)[None, :]) % 240 == 0, 3, 0).astype(np.int32)
    spec = np.zeros((total, K4, S), np.uint8)
    spec[45::n, :, 2::16] = M.NET_INTERRUPTED
    spec[48::n, :, 2::16] = M.NET_RESUMED
    ds_sessions = np.arange(0, S, 3, dtype=np.int32)

    def desync_of(c0):
        """The launch's records, shuffled: (call, session, frame, local, remote)."""
        c = np.repeat(np.arange(c0 + 5, c0 + n, 16, dtype=np.int32), len(ds_sessions))
        s = np.tile(ds_sessions, n // 16)
        o = np.random.default_rng(c0).permutation(len(c))
        return (c[o], s[o], (c[o] - 3).astype(np.int32), (s[o] & 0xffff).astype(np.uint16),
                ((s[o] + 1) & 0xffff).astype(np.uint16))

    dev = torch.device("cuda:0")

    def d(x):
        return torch.from_numpy(np.ascontiguousarray(x.view(np.int16) if x.dtype == np.uint16 else x)).to(dev)

    now_d, kinds_d = d(now.view(np.int64)), d(kinds)
    rows_d = dict(events=d(events), disc_req=d(disc_req), handled=d(handled), skip=d(skip), spec=d(spec))

    def engine(K):
        e = P2PEngine(S, num_players=2, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=total)
        e.set_arrival_schedule(True)
        e.set_endpoint_poll(TIMEOUT, NOTIFY, start)
        if K:
            e.set_spectator_emit(K, 16)
            e.set_spectator_poll(TIMEOUT, NOTIFY, start)
        e.set_event_queue(CAPACITY)
        e.add_arrivals(0, arrive)
        return e

    engines = {0: engine(0), K4: engine(K4)}
    C = min(a.check_sessions, S)
    models = {K: M.EventQueueModel(C, CAPACITY, K, 2, TIMEOUT - NOTIFY, TIMEOUT - NOTIFY) for K in engines}
    ms = dict(endpoint_poll=[], collect_k0=[], collect_k4=[])
    drain_us, drained, left_over = [], [], 0
    d_sess = torch.empty(S * CAPACITY, dtype=torch.int32, device=dev)
    d_recs = torch.empty((S * CAPACITY, 16), dtype=torch.uint8, device=dev)
    pushed = {k: 0 for k in ("resumed", "interrupted", "disconnected", "wait", "desync")}
    for j in range(a.warmup + a.launches):
        c0 = j * n
        sl = slice(c0, c0 + n)
        ds = desync_of(c0)
        ds_d = tuple(d(x) for x in ds)
        for K, e in engines.items():
            po = tuple(torch.empty((n, S), dtype=torch.uint8, device=dev) for _ in range(4))
            torch.cuda.synchronize()
            e.timing_reset()
            e.poll_endpoints(c0, n, now_d[sl], kinds_d[sl], out=po)
            t_poll, _ = e.timing_read()
            e.timing_reset()
            e.collect_events(c0, n, rows_d["events"][sl], rows_d["disc_req"][sl], rows_d["handled"][sl], po[3],
                             rows_d["spec"][sl] if K else None, rows_d["skip"][sl], desync=ds_d, on_device=True)
            t_col, _ = e.timing_read()
            e.synchronize()
            net = po[3].cpu().numpy()
            keep = ds[1] < C
            models[K].collect(c0, n, events[sl, :C], disc_req[sl, :C], handled[sl, :C], net[:, :C],
                              spec[sl][:, :, :C] if K else None, skip[sl, :C], tuple(x[keep] for x in ds))
            got = e.event_queue_state()
            for name, g, q in zip(("length", "dropped", "status", "closed_call"), got,
                                  zip(*((len(q.q), q.dropped, q.status, q.closed_call) for q in models[K].sessions))):
                assert (g[:C] == np.array(q)).all(), f"{name} differs from the model (K = {K}, launch {j})"
            for s in range(0, C, 7):
                want = list(models[K].sessions[s].q)
                recs = got[4][:len(want), s]
                assert [(int(r["kind"]), int(r["endpoint"]), int(r["call"]), int(r["payload"])) for r in recs] == want, \
                    f"session {s}'s queue differs from the model (K = {K}, launch {j})"
            if K == 0:
                for k, bit in (("resumed", 2), ("interrupted", 1), ("disconnected", 4)):
                    pushed[k] += int(((net & bit) != 0).sum())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_read, n_left = e.drain_events(S * CAPACITY, out=(d_sess, d_recs))
            t_drain = time.perf_counter() - t0
            models[K].drain(C * CAPACITY)
            left_over += n_left
            if j >= a.warmup:
                ms["collect_k0" if K == 0 else "collect_k4"].append(t_col / n)
                if K == 0:
                    ms["endpoint_poll"].append(t_poll / n)
                    drain_us.append(1e6 * t_drain)
                    drained.append(n_read)
    assert left_over == 0, "a drain left records behind"
    pushed["wait"], pushed["desync"] = int((skip > 0).sum()), int(len(ds_sessions) * (n // 16) * (a.warmup + a.launches))
    for e in engines.values():
        e.close()

    def stats(v, scale=1e3):
        return dict(median=round(scale * float(np.median(v)), 3), min=round(scale * min(v), 3), max=round(scale * max(v), 3))

    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = dict(sessions=S, players=2, calls_per_launch=n, timed_launches=a.launches, capacity=CAPACITY,
               unit="us per call (collect, endpoint_poll); us per drain, host time around the call (drain)",
               density=dict(per_session_and_64_calls=dict(
                   handled_inputs=round(float(handled.mean()) * n, 1),
                   net_event_records=round((pushed["resumed"] + pushed["interrupted"] + pushed["disconnected"]) /
                                           S / (a.warmup + a.launches), 3),
                   wait_recommendations=round(n / 240, 3), desync_records=round(4 / 3, 3)),
                   events_in_all=pushed, text="see the tool's docstring"),
               provenance=dict(commit=a.commit, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                               hip=str(torch.version.hip), tool="tools/event_queue_rate.py"),
               sessions_compared_with_the_model=C,
               **{k: stats(v) for k, v in ms.items()},
               drain=dict(stats(drain_us, 1.0), records_per_drain=int(np.median(drained))),
               collect_k0_over_endpoint_poll=round(med["collect_k0"] / med["endpoint_poll"], 3),
               collect_k4_over_endpoint_poll=round(med["collect_k4"] / med["endpoint_poll"], 3))

    # ---- the scheduled launch: this tree against the parent commit's library
    if a.parent_lib:
        rows = synth.gen_inputs(0, S, total, 2, synth.MODEL_HELD)
        plain = synth.jitter_arrivals(0, S, total, mp)
        pair = dict(this=RawEngine(_lib.LIB_PATH, S, 2, mp, 2 * n), parent=RawEngine(os.path.abspath(a.parent_lib), S, 2, mp, 2 * n))
        ab = {k: [] for k in pair}
        for j in range(a.warmup + a.launches):
            c0 = j * n
            for name in (("this", "parent") if j % 2 == 0 else ("parent", "this")):
                t = pair[name].launch(c0, rows[c0:c0 + n], plain[c0:c0 + n])
                if j >= a.warmup:
                    ab[name].append(t / n)
        assert (pair["this"].states() == pair["parent"].states()).all(), "the parent library's sessions differ"
        spread = max(max(v) - min(v) for v in ab.values())
        diff = abs(float(np.median(ab["this"])) - float(np.median(ab["parent"])))
        out["scheduled_launch_vs_parent"] = dict(this=stats(ab["this"]), parent=stats(ab["parent"]),
                                                 spread_us=round(1e3 * spread, 3), median_difference_us=round(1e3 * diff, 3),
                                                 agree_within_spread=bool(diff <= spread), states_equal=True)
        for e in pair.values():
            e.close()
    else:
        out["scheduled_launch_vs_parent"] = "not measured (no --parent-lib)"
    out["other_units_device_code_vs_parent"] = (open(a.unit_text).read().strip() if a.unit_text
                                                else "not compared (no --unit-text)")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
