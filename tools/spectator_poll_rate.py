#!/usr/bin/env python3
"""Device time of the two spectator poll units, beside the P2P endpoint poll on this tree's library and
on the parent commit's, and of the spectator-emit launch with and without the unit.

    python tools/spectator_poll_rate.py [--sessions 65536] [--launches 6] [--warmup 1] [--repeats 2]
                                        [--check-sessions 2048] [--parent-lib ggrs_amd/exp/libggrs_amd_parent.so]
                                        [--commit TEXT] [--out profiles/spectator_poll_rate.json]

64 calls per launch.  The clock steps 8, 16, 17 or 24 ms a call with a stall of 260 ms and one of 700 ms in
every launch; a link carries a message at nine calls in ten, every 16th link is silent for 20 calls and
every 64th for good; the timeouts are the reference's defaults (2000 ms, 500 ms notify).  Every array
stays in device memory.
  1. ggrs_spectator_poll_endpoints on a spectator engine, us per call; every output is first compared
     with tests/spectator_poll_model.py on the first --check-sessions sessions, and the final state too.
  2. ggrs_p2p_poll_spectator_endpoints at K = 1 and K = 4 on a scheduled P2P engine with spectator emit
     (2 players, player 0 local, synth.jitter_arrivals, 16 pending inputs, acks two calls late), checked
     in the same way; its resend row feeds ggrs_p2p_emit_spectator_packets, which is timed on this
     engine and on one without the unit given the same acks and flags (tools/spectator_emit_rate.py's
     method), launch by launch in alternating order.
  3. ggrs_p2p_poll_endpoints on this library and, with --parent-lib, on the parent commit's library in
     the same process, launch by launch in alternating order: both medians, the spread and whether the
     outputs are equal.
The whole measurement runs --repeats times; every figure is the median over a repeat's timed launches,
and the spread of the repeats' medians is recorded.  Prints one JSON line.  Needs a GPU.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

W, TIMEOUT, NOTIFY, N = 16, 2000, 500, 64
START = 5 * (1 << 32) - 1000


class RawPoll:
    """The P2P endpoint poll over a library given by path (the parent's has not every symbol the
    package binds): a scheduled engine whose calls are polled and never run."""

    def __init__(self, path, S, cap):
        from ggrs_amd.p2p import P2PConfig
        L = ctypes.CDLL(path)
        vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
        L.ggrs_p2p_engine_create.argtypes = [ctypes.POINTER(P2PConfig), ctypes.POINTER(vp)]
        L.ggrs_p2p_engine_destroy.argtypes = [vp]
        L.ggrs_p2p_set_arrival_schedule.argtypes = [vp, i32]
        L.ggrs_p2p_add_arrivals.argtypes = [vp, i32, i32, vp, vp]
        L.ggrs_p2p_set_endpoint_poll.argtypes = [vp, u64, u64, u64]
        L.ggrs_p2p_poll_endpoints.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32]
        L.ggrs_p2p_timing_reset.argtypes = [vp]
        L.ggrs_p2p_timing_read.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(i32)]
        L.ggrs_p2p_synchronize.argtypes = [vp]
        self.L, self.h = L, vp()
        cfg = P2PConfig(S, 2, 1, 0, 9, 1, 0, cap, 0, 0)
        self.ok(L.ggrs_p2p_engine_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        self.ok(L.ggrs_p2p_set_arrival_schedule(self.h, 1))
        self.ok(L.ggrs_p2p_set_endpoint_poll(self.h, TIMEOUT, NOTIFY, START))

    @staticmethod
    def ok(rc):
        if rc:
            raise RuntimeError(f"engine call failed: {rc}")

    def launch(self, c0, arrive, now_d, kinds_d, outs):
        """-> ms of ggrs_p2p_poll_endpoints over the calls (device tensors in place)"""
        n = arrive.shape[0]
        arrive = np.ascontiguousarray(arrive)
        self.ok(self.L.ggrs_p2p_add_arrivals(self.h, c0, n, arrive.ctypes.data_as(ctypes.c_void_p), None))
        self.ok(self.L.ggrs_p2p_timing_reset(self.h))
        self.ok(self.L.ggrs_p2p_poll_endpoints(self.h, c0, n, now_d.data_ptr(), kinds_d.data_ptr(),
                                               *(o.data_ptr() for o in outs), 1))
        ms, cnt = ctypes.c_float(), ctypes.c_int32()
        self.ok(self.L.ggrs_p2p_timing_read(self.h, ctypes.byref(ms), ctypes.byref(cnt)))
        self.ok(self.L.ggrs_p2p_synchronize(self.h))
        return ms.value

    def close(self):
        self.L.ggrs_p2p_engine_destroy(self.h)


def traffic(total, E, seed):
    """kinds [total][E]: an InputAck at nine calls in ten; every 16th link silent for 20 calls, every 64th
    for good."""
    from tests import endpoint_poll_model as P
    rng = np.random.default_rng(seed)
    kinds = np.where(rng.random((total, E)) < 0.9, P.K_INPUT_ACK, 0).astype(np.uint8)
    kinds[70:90, 3::16] = 0
    kinds[100:, 7::64] = 0
    return kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=6, help="timed 64-call launches")
    ap.add_argument("--warmup", type=int, default=1, help="untimed 64-call launches")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--check-sessions", type=int, default=2048, help="sessions compared with the models")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library, for part 3")
    ap.add_argument("--commit", default="", help="provenance: what was built (recorded as given)")
    ap.add_argument("--out", default=None, help="also write the result here")
    a = ap.parse_args()

    import torch
    from ggrs_amd import P2PEngine, SpectatorEngine, _lib, build, synth
    from tests import endpoint_poll_model as P
    from tests import spectator_poll_model as M
    build.build()
    S, n, mp = a.sessions, N, 9
    total = (a.warmup + a.launches) * n
    C = min(a.check_sessions, S)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0x5907)
    step = rng.choice((8, 16, 17, 24), total)
    step[20::n], step[45::n], step[0] = 260, 700, 0
    now = (np.uint64(START) + np.cumsum(step).astype(np.uint64)).astype(np.uint64)
    now_d = torch.from_numpy(now.view(np.int64)).to(dev)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    timed = lambda j: j >= a.warmup  # noqa: E731

    def spectator_unit():
        kinds = traffic(total, S, 1)
        kinds[kinds != 0] = P.K_INPUT
        kinds_d = torch.from_numpy(kinds).to(dev)
        model = M.run_host(C, TIMEOUT, NOTIFY, START, now, kinds[:, :C], np.zeros((total, C), np.uint8))
        e = SpectatorEngine(S, num_players=2)
        e.set_endpoint_poll(TIMEOUT, NOTIFY, START)
        ms = []
        for j in range(a.warmup + a.launches):
            c0 = j * n
            out = (u8(n, S), u8(n, S), u8(n, S))
            torch.cuda.synchronize()
            e.timing_reset()
            e.poll_endpoints(c0, n, now_d[c0:c0 + n], kinds_d[c0:c0 + n], None, out=out)
            t, _ = e.timing_read()
            e.synchronize()
            for name, x in zip(M.HOST_NAMES, out):
                assert (x[:, :C].cpu().numpy() == model[name][c0:c0 + n]).all(), f"{name} differs from the model"
            if timed(j):
                ms.append(t / n)
        for got, want in zip(e.endpoint_state(), model["model"].fields()):
            assert (got[:C] == want).all(), "the final state differs from the model"
        gone = int((e.endpoint_state()[4] >= 0).sum())
        e.close()
        return dict(spectator_engine_poll=ms), dict(hosts_gone=gone)

    def p2p_unit(K):
        rows = synth.gen_inputs(0, S, total, 2, synth.MODEL_HELD)
        arrive = synth.jitter_arrivals(0, S, total, mp)
        ack = np.full_like(arrive, -1)
        ack[2:] = arrive[:-2]
        ack_d = torch.from_numpy(np.ascontiguousarray(np.repeat(ack[:, None, :], K, axis=1))).to(dev)
        kinds = traffic(total, K * S, 2 + K)
        kinds_d = torch.from_numpy(kinds.reshape(total, K, S)).to(dev)
        cols = (np.arange(K)[:, None] * S + np.arange(C)[None, :]).reshape(-1)  # the checked sessions' endpoints
        model = M.run_links(K * C, TIMEOUT, NOTIFY, START, now, kinds[:, cols], np.zeros((total, K * C), np.uint8))

        def engine(poll):
            e = P2PEngine(S, num_players=2, local_players=(0,), max_prediction=mp, remote_latency=1, input_capacity=2 * n)
            e.set_arrival_schedule(True)
            e.set_spectator_emit(K, W)
            if poll:
                e.set_spectator_poll(TIMEOUT, NOTIFY, START)
            return e

        engines = dict(with_unit=engine(True), without=engine(False))
        stride = engines["without"].spectator_stride
        ms = {"p2p_spectator_poll": [], "spectator_emit_with_the_unit": [], "spectator_emit_without": []}
        for j in range(a.warmup + a.launches):
            c0 = j * n
            po = (u8(n, K, S), u8(n, K, S), u8(n, K, S))
            e = engines["with_unit"]
            torch.cuda.synchronize()
            e.timing_reset()
            e.poll_spectator_endpoints(c0, n, now_d[c0:c0 + n], kinds_d[c0:c0 + n], None, out=po)
            t_poll, _ = e.timing_read()
            e.synchronize()
            for name, x in zip(M.LINK_NAMES, po):
                got = x[:, :, :C].reshape(n, K * C).cpu().numpy()
                assert (got == model[name][c0:c0 + n]).all(), f"{name} differs from the model (K = {K})"
            t_emit = {}
            for name in (("with_unit", "without") if j % 2 == 0 else ("without", "with_unit")):
                e = engines[name]
                e.add_inputs(c0, rows[c0:c0 + n])
                e.add_arrivals(c0, arrive[c0:c0 + n])
                e.advance_frames(n)
                so = (torch.empty((n, K, S), dtype=torch.int32, device=dev), torch.empty((n, K, S), dtype=torch.int32, device=dev),
                      torch.empty((n, S), dtype=torch.int32, device=dev), torch.zeros((n, K, S, stride), dtype=torch.uint8, device=dev))
                torch.cuda.synchronize()
                e.timing_reset()
                e.emit_spectator_packets(c0, n, ack_d[c0:c0 + n], po[0], out=so)
                t_emit[name], _ = e.timing_read()
                e.synchronize()
            if timed(j):
                ms["p2p_spectator_poll"].append(t_poll / n)
                ms["spectator_emit_with_the_unit"].append(t_emit["with_unit"] / n)
                ms["spectator_emit_without"].append(t_emit["without"] / n)
        e = engines["with_unit"]
        for got, want in zip(e.spectator_endpoint_state(), model["model"].fields()):
            assert (got[:, :C].reshape(-1) == want).all(), "the final state differs from the model"
        closed = e.spectator_endpoint_state()[6]
        status, emit_closed = e.read_spectator_emit_state()[3:5]
        assert (emit_closed[closed >= 0] == closed[closed >= 0]).all() and (status[closed >= 0] == _lib.GGRS_EMIT_CLOSED).all()
        assert (e.sessions()[2] == 0).all(), "a session stopped"
        info = dict(endpoints=K * S, endpoints_closed=int((closed >= 0).sum()))
        for e in engines.values():
            e.close()
        torch.cuda.empty_cache()
        return ms, info

    def p2p_poll_pair():
        arrive = synth.jitter_arrivals(0, S, total, mp)
        kinds = traffic(total, S, 9)
        kinds_d = torch.from_numpy(kinds).to(dev)
        libs = dict(this=_lib.LIB_PATH)
        if a.parent_lib:
            libs["parent"] = os.path.abspath(a.parent_lib)
        pair = {k: RawPoll(v, S, total) for k, v in libs.items()}
        ms = {"p2p_endpoint_poll_" + k: [] for k in pair}
        equal = True
        for j in range(a.warmup + a.launches):
            c0 = j * n
            outs = {}
            order = list(pair) if j % 2 == 0 else list(pair)[::-1]
            for name in order:
                outs[name] = tuple(u8(n, S) for _ in range(4))
                torch.cuda.synchronize()
                t = pair[name].launch(c0, arrive[c0:c0 + n], now_d[c0:c0 + n], kinds_d[c0:c0 + n], outs[name])
                if timed(j):
                    ms["p2p_endpoint_poll_" + name].append(t / n)
            if "parent" in outs:
                equal = equal and all(bool((x == y).all()) for x, y in zip(outs["this"], outs["parent"]))
        for e in pair.values():
            e.close()
        return ms, dict(outputs_equal=equal if a.parent_lib else "not measured (no --parent-lib)")

    repeats, info = [], {}
    for r in range(a.repeats):
        med = {}
        for key, part in (("spectator_engine", spectator_unit), ("K1", lambda: p2p_unit(1)), ("K4", lambda: p2p_unit(4)),
                          ("p2p_endpoint_poll", p2p_poll_pair)):
            ms, extra = part()
            info[key] = extra
            med[key] = {k: round(1e3 * float(np.median(v)), 3) for k, v in ms.items()}
            med[key].update({k + "_min_max": [round(1e3 * min(v), 3), round(1e3 * max(v), 3)] for k, v in ms.items()})
        repeats.append(med)

    def over_repeats(key, name):
        v = [r[key][name] for r in repeats]
        return dict(median=round(float(np.median(v)), 3), repeats=v, spread=round(max(v) - min(v), 3))

    out = dict(sessions=S, calls_per_launch=n, timed_launches=a.launches, repeats=a.repeats, unit="us per call",
               disconnect_timeout_ms=TIMEOUT, disconnect_notify_start_ms=NOTIFY, sessions_compared_with_the_models=C,
               schedule="clock steps of 8/16/17/24 ms with stalls of 260 and 700 ms in every launch; a message at nine "
                        "calls in ten, every 16th link silent for 20 calls, every 64th for good",
               provenance=dict(commit=a.commit, device=torch.cuda.get_device_name(0), torch=torch.__version__,
                               hip=str(torch.version.hip), tool="tools/spectator_poll_rate.py",
                               parent_lib=a.parent_lib or "none"),
               spectator_engine_poll=dict(over_repeats("spectator_engine", "spectator_engine_poll"), **info["spectator_engine"]),
               p2p_endpoint_poll_this=over_repeats("p2p_endpoint_poll", "p2p_endpoint_poll_this"),
               p2p_endpoint_poll_parent=(over_repeats("p2p_endpoint_poll", "p2p_endpoint_poll_parent") if a.parent_lib
                                         else "not measured (no --parent-lib)"),
               p2p_endpoint_poll_outputs_equal_parent=info["p2p_endpoint_poll"]["outputs_equal"],
               per_repeat=repeats)
    for K in (1, 4):
        key = "K%d" % K
        out[key] = dict(p2p_spectator_poll=over_repeats(key, "p2p_spectator_poll"),
                        spectator_emit_with_the_unit=over_repeats(key, "spectator_emit_with_the_unit"),
                        spectator_emit_without=over_repeats(key, "spectator_emit_without"), **info[key])
    out["K4_over_K1"] = round(out["K4"]["p2p_spectator_poll"]["median"] / out["K1"]["p2p_spectator_poll"]["median"], 3)
    out["bytes_per_endpoint_and_call"] = dict(spectator_engine="2 in (kinds, events), 3 out",
                                              p2p_spectator_poll="2 in (kinds, close_in), 3 out",
                                              p2p_endpoint_poll="2 in (kinds, events), 4 out")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
