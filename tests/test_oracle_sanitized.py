"""Host sanitizers over the oracle: oracle/ggrs_oracle.c built with -fsanitize=address,undefined
(GPU sanitizers are not available on this pool; the C restatement is the host code that matters),
driven by oracle/sanitize_main.c; its digests must equal the normal build's."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_oracle_under_asan_ubsan(oracle, tmp_path):
    exe = str(tmp_path / "oracle_asan")
    subprocess.run(["gcc", "-O1", "-g", "-ffp-contract=off", "-fno-omit-frame-pointer", "-std=c11", "-D_GNU_SOURCE",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "oracle", "ggrs_oracle.c"), os.path.join(ROOT, "oracle", "sanitize_main.c"),
                    "-o", exe, "-lm", "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    lines = dict((" ".join(l.split()[:2]) if l.startswith("synctest") else l.split()[0], l) for l in r.stdout.splitlines())
    # same digests from the normal (ctypes) build
    cases = [(2, 8, 7, 2, 400, 0), (4, 9, 8, 0, 300, 1), (1, 4, 2, 1, 200, 0), (3, 63, 62, 0, 150, 1)]
    for c, (P, mp, cd, d, frames, model) in enumerate(cases):
        inp = oracle.gen_inputs(0x6767525300000000 + c, frames, P, model)
        res = oracle.synctest_run(inp, P, mp, cd, d, corrupt_frame=77 if c == 1 else -1)
        done = res["result"].frames_done
        want = (f"synctest {c} status {res['result'].status} frames {done} last "
                f"{int(res['cksum'][done - 1])} final {oracle.fletcher16(bytes(res['final_state']))}")
        assert lines[f"synctest {c}"] == want
    pr = oracle.particles_synctest_run(oracle.gen_inputs(9, 40, 2, 1), 64, 2, 17, 16, session=3)
    assert lines["particles"] == (f"particles status {pr['result'].status} last {int(pr['ck_trace'][39])} "
                                  f"final {oracle.fletcher16(bytes(pr['final_state']))}")
    _, cks, _ = oracle.p2p_replay(oracle.state_new(2), 0, np.array([(i * 5) % 16 for i in range(16)], np.uint8))
    assert lines["p2p"] == f"p2p last {int(cks[7])}"
    # the single-step batch entries on sanitize_main.c's 64 player states / 16 four-player states
    N, P = 64, 4
    rots = np.array([0.0, 6.2831855, 0.041666668, 3.1415927, -0.0, 100.0, -3.0e9, 1.0e38], np.float32)
    vels = np.array([0.0, -0.0, 7.142857, -7.2, 1.0e-45, -3.0, 5.05, 8.0], np.float32)
    xs = np.array([0.0, 600.0, 300.0, 2.94], np.float32)
    i = np.arange(N)
    pl = np.stack([xs[i & 3], (200.0 * ((i >> 2) & 3) + 100.0).astype(np.float32), vels[i & 7], vels[(i >> 3) & 7],
                   rots[(i * 5) & 7]], axis=1).astype(np.float32)
    inp = (i * 7).astype(np.uint8)
    po = oracle.ship_step_batch(pl.view(np.uint32), inp)
    st = np.zeros((N // P, 36 + 20 * P), np.uint8)
    st[:, 0:4] = (np.arange(N // P, dtype=np.int32) - 3).view(np.uint8).reshape(-1, 4)
    st[:, [4, 12, 20 + 8 * P, 28 + 16 * P]] = P
    plb = pl.reshape(N // P, P, 5)
    st[:, 20:20 + 8 * P] = np.ascontiguousarray(plb[:, :, 0:2]).view(np.uint8).reshape(N // P, -1)
    st[:, 28 + 8 * P:28 + 16 * P] = np.ascontiguousarray(plb[:, :, 2:4]).view(np.uint8).reshape(N // P, -1)
    st[:, 36 + 16 * P:] = np.ascontiguousarray(plb[:, :, 4]).view(np.uint8).reshape(N // P, -1)
    status = ((np.arange(N // P)[:, None] + np.arange(P)[None, :]) % 3).astype(np.uint8)
    so = oracle.state_advance_batch(st, inp.reshape(N // P, P), status)
    assert lines["stepbatch"] == (f"stepbatch rc 0 players {oracle.fletcher16(po.tobytes())} "
                                  f"states {oracle.fletcher16(so.tobytes())} last {int(oracle.fletcher16_batch(so)[-1])}")
