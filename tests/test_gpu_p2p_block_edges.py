"""GPU parity of the P2P kernels at the edges of their blocks and stages, EVERY session against the
oracle (oracle_p2p_batch for final states and counts; oracle_p2p_run per session for what the batch
entry does not return: the display-checksum trace and the saved-state ring).

The shapes are the smallest that reach what the kernels' shared plumbing (csrc/p2p_device.h) branches
on: input rows of a whole number of 16-byte pieces (staged piece-wise in the full blocks) and not
(byte-wise everywhere), a partial last block of 16, 8, 2, 1 and 4 sessions, and a launch longer than
one stage of LDS rows (flat_rows_lds: 192, 96, 48 rows for 1, 2, 3-4 players), so the stage loop
crosses a boundary and the ring (9 cells) wraps many times."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

pytestmark = pytest.mark.gpu

MP, D, DELAY = 8, 3, 1
SHAPES = [
    # players, local players, sessions, calls of the last launch (> flat_rows_lds(P))
    (1, (), 144, 200),     # 144-byte rows: 16-byte pieces in the full blocks; last block 16 sessions
    (2, (0,), 136, 100),   # 272-byte rows: 16-byte pieces in the full blocks; last block 8
    (2, (1,), 130, 100),   # 260-byte rows: byte path everywhere; last block 2
    (3, (0,), 129, 60),    # byte path everywhere; last block 1
    (4, (0, 2), 132, 60),  # 528-byte rows: 16-byte pieces in the full blocks; last block 4
]
IDS = ["p1_s144", "p2_s136", "p2_s130", "p3_s129", "p4_s132"]
LAUNCHES = lambda last: (1, 7, last)  # noqa: E731


def mask_of(local):
    return sum(1 << k for k in local)


@functools.lru_cache(maxsize=None)
def inputs_of(k):
    from tests.test_gpu_p2p import stream
    P, _, S, last = SHAPES[k]
    rows = stream(S, sum(LAUNCHES(last)), P, 1, seed_base=0xED6E + k)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def reference(k, sparse):
    """The oracle's every session of shape k, computed once and shared by the forms."""
    from oracle import oracle as o
    P, local, S, _ = SHAPES[k]
    rows = inputs_of(k)
    kw = dict(num_players=P, local_mask=mask_of(local), input_delay=DELAY, max_prediction=MP, latency=D,
              predictor=0, sparse_saving=sparse)
    batch = o.p2p_batch(rows, **kw)
    assert (batch["rc"] == 0).all()
    runs = [o.p2p_run(rows[:, s], **kw) for s in range(S)]
    assert all(r["rc"] == 0 for r in runs)
    return batch, runs


def engine(k, form, sparse=False, trace=False, interval=0):
    from ggrs_amd import P2PEngine
    P, local, S, last = SHAPES[k]
    rows = inputs_of(k)
    frames = rows.shape[0]
    eng = P2PEngine(S, num_players=P, local_players=local, input_delay=DELAY, max_prediction=MP, remote_latency=D,
                    input_capacity=frames + 8, trace_capacity=frames if trace else 0)
    if sparse:
        eng.set_sparse_saving(True)
    if interval:
        eng.set_desync_detection(interval)
    eng.set_kernel_form(form)
    eng.add_inputs(0, rows)
    for n in LAUNCHES(last):
        eng.advance_frames(n)
    assert eng.current_frame() == frames
    return eng


def check_every_session(eng, k, sparse, trace):
    batch, runs = reference(k, sparse)
    S = SHAPES[k][2]
    frames = inputs_of(k).shape[0]
    rb, rs = eng.stats()
    assert (eng.states() == batch["final_states"]).all()
    assert (rb == batch["rollbacks"]).all() and (rs == batch["resim"]).all()
    tr = eng.trace(0, frames) if trace else None
    for s in range(S):
        out = runs[s]
        assert rb[s] == out["result"].rollbacks and rs[s] == out["result"].resim, s
        assert bytes(eng.state(s)) == bytes(out["final_state"]), s
        fr, cks, states = eng.ring(s)
        assert (fr == out["ring_frames"]).all(), (s, fr, out["ring_frames"])
        assert (cks == out["ring_cksums"]).all(), s
        assert (states == out["ring_states"]).all(), s
        if tr is not None:
            assert (tr[:, s] == out["ck_trace"]).all(), s


@functools.lru_cache(maxsize=None)
def stepped_queues(k, sparse):
    """The raw queue words the queue-stepping flat kernel leaves: what every form must leave."""
    return engine(k, "flat_queues", sparse).queues()


PLAIN = [(f, False) for f in ("canonical", "flat", "flat_queues", "unstaged")] + [("canonical", True), ("flat_queues", True)]


@pytest.mark.parametrize("form,sparse", PLAIN, ids=[f + ("_sparse" if sp else "") for f, sp in PLAIN])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_block_edges_plain_launches(oracle, k, form, sparse):
    """Plain launches (no trace, no desync history): state, ring and counts of every session, and the
    device queue words equal to the queue-stepping kernel's, whichever form ran."""
    eng = engine(k, form, sparse)
    check_every_session(eng, k, sparse, trace=False)
    assert (eng.queues() == stepped_queues(k, sparse)).all()


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_block_edges_sparse_saving_with_trace(oracle, k):
    """Sparse saving with the display trace kept (the canonical kernel keeps none, so this is the
    queue-stepping kernel with its ring in LDS): every session's trace as well."""
    eng = engine(k, "flat_queues", sparse=True, trace=True)
    check_every_session(eng, k, True, trace=True)
    assert (eng.queues() == stepped_queues(k, True)).all()


@pytest.mark.parametrize("form", ["canonical", "flat", "flat_queues", "unstaged"])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=IDS)
def test_block_edges_desync_interval(oracle, k, form):
    """DesyncDetection::On{interval: 4}: every call whose report is due reads a saved cell's checksum
    back (the canonical kernel from its LDS ring; the other forms, run with the display trace, from
    theirs), and the reports kept are the oracle's cell checksums: the report of frame F is sent at
    call F + D + 1 before its rollback (p2p_session.rs:939-975), so it is the checksum cell F holds
    after F + D + 1 calls."""
    from oracle import oracle as o
    interval = 4
    trace = form != "canonical"  # (a trace takes the canonical kernel away)
    eng = engine(k, form, trace=trace, interval=interval)
    check_every_session(eng, k, False, trace)
    assert (eng.queues() == stepped_queues(k, False)).all()
    P, local, S, _ = SHAPES[k]
    rows = inputs_of(k)
    newest = ((rows.shape[0] - 2 - D) // interval) * interval
    oldest = newest - 31 * interval  # MAX_CHECKSUM_HISTORY_SIZE reports are kept
    for F in (newest, newest - 13 * interval, max(oldest, interval)):
        got = eng.local_checksums(F)
        for s in range(S):
            out = o.p2p_run(rows[:F + D + 1, s], num_players=P, local_mask=mask_of(local), input_delay=DELAY,
                            max_prediction=MP, latency=D, predictor=0)
            assert out["ring_frames"][F % (MP + 1)] == F
            assert got[s] == out["ring_cksums"][F % (MP + 1)], (F, s)


@pytest.mark.parametrize("S,form", [(136, "flat"), (20, "chains")], ids=["s136_flat", "s20_time_aligned"])
def test_block_edges_scheduled_arrivals(oracle, monkeypatch, S, form):
    """Arrival schedules, two players: two full blocks and a partial one of 8 on the
    one-thread-per-session kernel, and a full block of 16 sessions and a partial one of 4 on the
    time-aligned form; every session as tests/test_gpu_p2p_sched.py checks them."""
    from ggrs_amd import P2PEngine, synth
    from tests.test_gpu_p2p_sched import check_sessions, set_form
    set_form(monkeypatch, form)
    calls, P = 108, 2
    rows = synth.gen_inputs(0, S, calls, P, synth.MODEL_HELD)
    arrive = synth.jitter_arrivals(0, S, calls, MP)
    eng = P2PEngine(S, num_players=P, local_players=(0,), input_delay=DELAY, max_prediction=MP, remote_latency=1,
                    input_capacity=calls)
    eng.set_arrival_schedule(True)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, arrive)
    for n in (1, 7, 100):
        eng.advance_frames(n)
    check_sessions(eng, rows, arrive, np.zeros((calls, S), np.uint8), range(S), calls)
    _, _, errors = eng.sessions()
    assert (errors == 0).all()
