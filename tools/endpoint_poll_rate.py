#!/usr/bin/env python3
"""Device time of the P2P engine's endpoint poll beside time sync and packet emit on the same engine
and calls.

    python tools/endpoint_poll_rate.py [--sessions 65536] [--max-prediction 9] [--launches 6] [--warmup 1]
                                       [--check-sessions 4096] [--commit TEXT]
                                       [--out profiles/endpoint_poll_rate.json]

2 players, player 0 local, arrival schedules, the bench's jitter schedule (synth.jitter_arrivals), 64
calls per launch.  The clock steps 8, 16, 17 or 24 ms a call with a stall of 260 ms and one of 700 ms in
every launch, both below the disconnect timeout; a session received an Input at the calls its arrival
row rises, other messages at a tenth of the rest; every 16th session's link is silent for 20 calls and
every 64th for good.  The timeouts are the reference's defaults, 2000 ms and 500 ms notify, so only the
links silent for good time out (their players are disconnected by the calls) and every other endpoint
stays Running: the fraction Running at the start of the first and after the last timed launch is
asserted (>= 97 %) and recorded.  The timers, NetworkInterrupted / NetworkResumed (the 700 ms stalls
interrupt every link that is quiet at that call) and the disconnect timeout all fire.  Every array
stays in device memory; the unit's resend row feeds packet emit.  ggrs_p2p_poll_endpoints,
ggrs_p2p_time_sync (the yardstick: the same launch shape), ggrs_p2p_emit_packets and
ggrs_p2p_advance_frames are timed on the device, us per call.  Every output of the unit is first compared with tests/endpoint_poll_model.py on the first
--check-sessions sessions, and the endpoints' final state too.
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

FPS, W, TIMEOUT, NOTIFY = 60, 16, 2000, 500  # (builder.rs:17-18)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--max-prediction", type=int, default=9)
    ap.add_argument("--launches", type=int, default=6, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--check-sessions", type=int, default=4096, help="sessions compared with the model")
    ap.add_argument("--commit", default="", help="provenance: what was built (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, build, synth
    from tests import endpoint_poll_model as M
    build.build()
    S, P, mp, n = a.sessions, 2, a.max_prediction, 64
    total = (a.warmup + a.launches) * n
    rows = synth.gen_inputs(0, S, total, P, synth.MODEL_HELD)
    arrive = synth.jitter_arrivals(0, S, total, mp)
    # a silent link delivers nothing: the session waits at the prediction threshold until the timeout
    arrive[70:90, 3::16] = arrive[69, 3::16]
    arrive[100:, 7::64] = arrive[99, 7::64]
    rng = np.random.default_rng(0xE9D)
    step = rng.choice((8, 16, 17, 24), total)
    step[20::n], step[45::n], step[0] = 260, 700, 0
    start = 5 * (1 << 32) - 1000
    now = (np.uint64(start) + np.cumsum(step).astype(np.uint64)).astype(np.uint64)
    rise = np.diff(arrive, axis=0, prepend=-1) > 0
    kinds = np.where(rise, M.K_INPUT, 0).astype(np.uint8)
    kinds[~rise & (rng.random((total, S)) < 0.1)] = M.K_INPUT_ACK | M.K_QUALITY_REPLY
    kinds[70:90, 3::16] = 0
    kinds[100:, 7::64] = 0
    dev = torch.device("cuda:0")
    now_d = torch.from_numpy(now.view(np.int64)).to(dev)
    kinds_d, arrive_d = torch.from_numpy(kinds).to(dev), torch.from_numpy(arrive).to(dev)

    C = min(a.check_sessions, S)
    model = M.run(C, TIMEOUT, NOTIFY, start, 0b10, now, kinds[:, :C], np.zeros((total, C), np.uint8))
    names = ("resend", "send_ack", "send_report", "net_events")

    # the row ring holds the whole run: a link silent for good keeps its last delivered frame's row in use
    e = P2PEngine(S, num_players=P, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=total)
    e.set_arrival_schedule(True)
    e.set_packet_emit(W)
    e.set_time_sync(FPS)
    e.set_endpoint_poll(TIMEOUT, NOTIFY, start)
    ms = dict(endpoint_poll=[], time_sync=[], packet_emit=[], advance=[])
    raised = {k: 0 for k in ("resend", "send_report", "interrupted", "resumed", "disconnected")}
    running = []
    for j in range(a.warmup + a.launches):
        c0 = j * n
        if j == a.warmup:  # what the timed launches start from
            running.append(float((e.endpoint_state()[0] == 0).mean()))
        e.add_inputs(c0, rows[c0:c0 + n])
        e.add_arrivals(c0, arrive[c0:c0 + n])
        po = tuple(torch.empty((n, S), dtype=torch.uint8, device=dev) for _ in range(4))
        torch.cuda.synchronize()
        e.timing_reset()
        e.poll_endpoints(c0, n, now_d[c0:c0 + n], kinds_d[c0:c0 + n], out=po)
        t_poll, _ = e.timing_read()
        e.timing_reset()
        e.advance_frames(n)
        t_adv, _ = e.timing_read()
        to = tuple(torch.empty((n, S), dtype=torch.int32, device=dev) for _ in range(3))
        torch.cuda.synchronize()
        e.timing_reset()
        e.time_sync(c0, n, None, None, out=to)
        t_ts, _ = e.timing_read()
        eo = tuple(torch.empty((n, S), dtype=torch.int32, device=dev) for _ in range(3)) + (
            torch.zeros((n, S, e.out_stride), dtype=torch.uint8, device=dev),)
        torch.cuda.synchronize()
        e.timing_reset()
        e.emit_packets(c0, n, arrive_d[c0:c0 + n], po[0], out=eo)
        t_emit, _ = e.timing_read()
        e.synchronize()
        for name, x in zip(names, po):
            assert (x[:, :C].cpu().numpy() == model[name][c0:c0 + n]).all(), f"{name} differs from the model"
        net = po[3]
        raised["resend"] += int(po[0].sum())
        raised["send_report"] += int(po[2].sum())
        for k, bit in (("interrupted", 1), ("resumed", 2), ("disconnected", 4)):
            raised[k] += int(((net & bit) != 0).sum())
        if j >= a.warmup:
            ms["endpoint_poll"].append(t_poll / n)
            ms["time_sync"].append(t_ts / n)
            ms["packet_emit"].append(t_emit / n)
            ms["advance"].append(t_adv / n)
    for got, want in zip(e.endpoint_state(), model["model"].fields()):
        assert (got[:C] == want).all(), "the final state differs from the model"
    state, closed = e.endpoint_state()[0], e.endpoint_state()[6]
    running.append(float((state == 0).mean()))
    # the figures are those of live endpoints: only the links silent for good may have closed
    assert min(running) >= 0.97, running
    assert ((closed >= 0) == (np.arange(S) % 64 == 7)).all(), "an endpoint closed that was not silent for good"
    ts_closed, errors = e.time_sync_state()[4], e.sessions()[2]
    bad = np.nonzero(ts_closed != closed)[0]
    assert len(bad) == 0, ("time sync closed elsewhere than the unit", len(bad),
                           [(int(s), int(ts_closed[s]), int(closed[s]), int(errors[s])) for s in bad[:8]])
    assert (errors == 0).all(), "a session stopped"
    e.close()

    def stats(v):
        return dict(median=round(1e3 * float(np.median(v)), 3), min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3))

    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = dict(sessions=S, players=P, max_prediction=mp, calls_per_launch=n, timed_launches=a.launches,
               disconnect_timeout_ms=TIMEOUT, disconnect_notify_start_ms=NOTIFY, unit="us per call",
               schedule="synth.jitter_arrivals; clock steps of 8/16/17/24 ms with stalls of 260 and 700 ms in every "
                        "launch; every 16th session silent for 20 calls, every 64th for good",
               running_fraction=dict(at_first_timed_launch=round(running[0], 4), after_last_timed_launch=round(running[1], 4)),
               reports_per_session=round(raised["send_report"] / S, 1),
               provenance=dict(commit=a.commit, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                               hip=str(torch.version.hip), tool="tools/endpoint_poll_rate.py"),
               sessions_compared_with_the_model=C, raised=raised, endpoints_closed=int((closed >= 0).sum()),
               sessions_stopped=0, input_capacity=total,
               **{k: stats(v) for k, v in ms.items()},
               endpoint_poll_over_time_sync=round(med["endpoint_poll"] / med["time_sync"], 3),
               endpoint_poll_over_packet_emit=round(med["endpoint_poll"] / med["packet_emit"], 3),
               endpoint_poll_over_advance=round(med["endpoint_poll"] / med["advance"], 4),
               bytes_per_session_and_call=dict(endpoint_poll_in="2 (kinds, events; 6 with the packet feed's status)",
                                               endpoint_poll_out=4, time_sync_in="9 (17 with rtt_ms and remote_advantage)",
                                               time_sync_out=12))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
