"""bench.py's plain run, --full and --dump-outputs on the default workload (SyncTest config 2) at a
small size: a plain run leaves the parity leg and the CPU baselines out, --full runs them, and two
runs with the same arguments dump identical outputs, which are the engine's own bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--lanes", "192", "--frames-per-step", "24"]


def run_bench(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py", *SMALL, *extra])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_keeps_values_exactly(tmp_path):
    a = {"bytes": np.arange(256, dtype=np.uint8), "cks": np.array([0, 65535], np.uint16),
         "frames": np.array([2 ** 31 - 1, -1], np.int32), "f": np.array([1e-40, np.pi], np.float32),
         "flags": np.array([True, False])}
    bench.dump_outputs(str(tmp_path / "d"), a)
    got = {k: np.load(tmp_path / "d" / (k + ".npy")) for k in a}
    assert {k: v.dtype for k, v in got.items()} == {"bytes": np.float32, "cks": np.float32, "frames": np.float64,
                                                    "f": np.float32, "flags": np.float32}
    for k in a:
        assert (got[k].astype(a[k].dtype) == a[k]).all(), k
    assert got["f"].tobytes() == a["f"].tobytes()


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), {"a": np.zeros(200, np.float32), "b": np.zeros(100, np.float32)})


def test_box_state_arrays_split_frame_and_fields():
    from oracle import pyoracle
    rows = []
    for k in (7, 8, 9):
        s = pyoracle.State(k, [(k + 0.5, -k), (1e-40, 3.0)], [(0.25, k), (-0.0, 2.0)], [k / 3, -1.0])
        rows.append(np.frombuffer(s.bincode(), np.uint8))
    frames, fields = bench.box_state_arrays(np.stack(rows))
    assert frames.tolist() == [7, 8, 9]
    assert fields.dtype == np.float32 and fields.shape == (3, 10)
    want = np.array([[k + 0.5, -k, 1e-40, 3.0, 0.25, k, -0.0, 2.0, k / 3, -1.0] for k in (7, 8, 9)], np.float32)
    assert fields.tobytes() == want.tobytes()


def _held_inputs(device, first_session, sessions, frames, players, chunk):
    import torch
    parts = list(bench.held_inputs_chunks(torch, first_session, sessions, frames, players, torch.device(device), chunk))
    assert [f0 for f0, _ in parts] == list(range(0, frames, chunk or frames))
    return np.concatenate([rows.cpu().numpy() for _, rows in parts])


@pytest.mark.parametrize("first_session,sessions,frames,players,chunk",
                         [(0, 67, 200, 2, 64), (4096, 5, 333, 4, 7), (3, 1, 50, 1, 50)])
def test_held_inputs_chunks_equal_the_host_generator(first_session, sessions, frames, players, chunk):
    """The bench's chunked torch generator against synth.gen_inputs (held-key model): keys held
    across chunk boundaries, from the zero start, other first sessions and player counts."""
    from ggrs_amd import synth
    want = synth.gen_inputs(first_session, sessions, frames, players, synth.MODEL_HELD)
    got = _held_inputs("cpu", first_session, sessions, frames, players, chunk)
    assert got.dtype == np.uint8 and got.shape == want.shape and (got == want).all()


@pytest.mark.gpu
def test_held_inputs_chunks_on_the_device_equal_the_host_generator():
    from ggrs_amd import synth
    want = synth.gen_inputs(192, 300, 130, 2, synth.MODEL_HELD)
    assert (_held_inputs("cuda", 192, 300, 130, 2, 48) == want).all()
    assert (_held_inputs("cuda", 192, 300, 130, 2, None) == want).all()


@pytest.mark.gpu
def test_full_run_past_the_parity_budget_checks_spread_lanes(monkeypatch, capsys):
    """More lanes x frames than the parity leg's budget: it replays evenly spaced lanes, the first
    and the last among them, instead of every lane."""
    monkeypatch.setattr(bench, "PARITY_LANE_FRAMES", 5 * 24 * 10)
    d = run_bench(monkeypatch, capsys, "--full", "--no-cpu-baseline")
    assert d["parity"]["lanes"] == 10 and d["parity"]["lanes_of"] == 192
    assert d["parity"]["every_lane_bit_exact"] is True and d["cpu_baseline"] is None


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeatably(monkeypatch, capsys, tmp_path):
    a = run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "a"))
    b = run_bench(monkeypatch, capsys, "--dump-outputs", str(tmp_path / "b"))
    for d in (a, b):
        assert d["parity"] is None and d["cpu_baseline"] is None
        assert d["steps"] == 3 and d["warmup"] == 2 and d["halted_lanes"] == 0
        assert d["metric"] == "resimulated session-frames/sec (node)" and d["unit"] == "session-frames/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f32"
        # value = lanes x check_distance x frames per step over the step time (ms_per_step is
        # rounded to 1e-4 ms, a step here takes some hundredths of a millisecond)
        assert d["ms_per_step"] > 0
        assert d["value"] == pytest.approx(192 * 8 * 24 / (d["ms_per_step"] * 1e-3), rel=0.02)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["checksum_trace.npy", "final_state_fields.npy", "final_state_frames.npy", "lane_status.npy"]
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), n
        total += x.nbytes
    assert total <= 64 << 20
    fields = np.load(tmp_path / "a" / "final_state_fields.npy")
    assert fields.shape == (192, 10)
    assert (np.load(tmp_path / "a" / "final_state_frames.npy") == 5 * 24).all()
    assert np.load(tmp_path / "a" / "checksum_trace.npy").shape == (5 * 24, 192)
    assert (np.load(tmp_path / "a" / "lane_status.npy") == 0).all()


@pytest.mark.gpu
def test_full_run_carries_parity_and_cpu_baseline_and_the_dump_is_the_oracles(monkeypatch, capsys, tmp_path, oracle):
    from ggrs_amd import synth
    d = run_bench(monkeypatch, capsys, "--full", "--cpu-frames", "20000", "--cpu-threads", "2",
                  "--dump-outputs", str(tmp_path))
    assert d["parity"]["every_lane_bit_exact"] is True and d["parity"]["lanes"] == 192
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["thread0_matches_gpu_lane0"] is True
    # the dumped states and checksums are what the oracle's SyncTestSession computes for these inputs
    inputs = synth.gen_inputs(0, 192, 5 * 24, 2, synth.MODEL_HELD)
    fields = np.load(tmp_path / "final_state_fields.npy")
    trace = np.load(tmp_path / "checksum_trace.npy")
    for lane in (0, 77, 191):
        ref = oracle.synctest_run(inputs[:, lane, :], 2, 9, 8, 0)
        want_frame, want = bench.box_state_arrays(np.frombuffer(bytes(ref["final_state"]), np.uint8)[None])
        assert want_frame[0] == 5 * 24 and fields[lane].tobytes() == want[0].tobytes()
        assert (trace[:, lane] == ref["cksum"]).all()
