"""Where a remote InputQueue's 128 entries run out: the oracle's stopping call (rc == -4 of
oracle_p2p_sched_run, its `length + 1 > INPUT_QUEUE_LENGTH` before every remote add) against
tests/input_queue_model.py, an independent restatement of the queue's frame bookkeeping.  CPU only.
The model is driven by the arrival column and the oracle's per-call `advanced[]`; the first call at
which its length would pass 128 must be the oracle's stopping call, and there must be none where
the oracle runs through.  Fixed schedules and seeds: the same sessions on every run."""
import numpy as np
import pytest

from tests import input_queue_model as Q
from tests import queue_bound_schedules as B

LAYOUTS = [(2, (0,)), (2, (1,)), (4, (0, 2)), (3, (0,)), (4, (1,)), (2, ())]  # the layouts of test_gpu_p2p_sched.CASES
MAX_PREDICTIONS = (0, 1, 2, 8, 40)
JITTERED = 21


def jittered(mask, P, seed):
    """The jittered / stalled / fixed-lag networks of the lockstep parity tests, without disconnects."""
    from tests.test_gpu_p2p_sched import schedules
    arrive, _ = schedules(JITTERED, B.JITTER_CALLS, 8, seed, mask, P, disconnect_every=0)
    return arrive


def stop_call(out):
    return out["result"].frames_done if out["rc"] == -4 else None


@pytest.mark.parametrize("delay", [0, 1, 3])
@pytest.mark.parametrize("P,local", LAYOUTS)
def test_model_overflows_at_the_oracles_stopping_call(oracle, P, local, delay):
    mask = sum(1 << k for k in local)
    rows = oracle.gen_inputs(oracle.session_seed(P, 0x1B0), B.RATE_CALLS, P, 1)
    ladder, labels = B.rung_table(len(B.RUNGS))
    columns = [(label, ladder[:, i]) for i, label in enumerate(labels)]
    columns += [(("jitter", i), col) for i, col in enumerate(jittered(mask, P, 13 + P + delay).T)]
    stopped = ran = 0
    for mp in MAX_PREDICTIONS:
        for label, arrive in columns:
            calls = len(arrive)
            out = oracle.p2p_sched_run(rows[:calls], arrive, num_players=P, local_mask=mask, input_delay=delay,
                                       max_prediction=mp)
            assert out["rc"] in (0, -4), (mp, label, out["rc"])
            done = out["result"].frames_done
            got = Q.first_overflow_call(arrive, out["advanced"][:done], bool(local), delay, mp)
            assert got == stop_call(out), (mp, label, got, stop_call(out))
            stopped += out["rc"] == -4
            ran += out["rc"] == 0
    assert stopped >= 20 and ran >= 20, (stopped, ran)  # the cases straddle the bound


def test_the_ladders_straddle_the_bound_in_every_mode(oracle):
    """P = 2, local player 0, delay 0: the last rung that survives its burst and the first that stops
    there are both on the stall ladder (the burst of rung L is call 20 + L) and on the catch-up
    ladder (call 141), in lockstep and in rollback mode -- the stall ladder's is the tail at frame 17
    (last_confirmed_frame 18 through the silence) and frames up to 19 + L: 128 entries at L = 125;
    the rate runs stop in lockstep mode at calls 253 .. 257 and run through in rollback mode."""
    rows = oracle.gen_inputs(oracle.session_seed(2, 0x1B0), B.RATE_CALLS, 2, 1)

    def stops_at(build, values, mp, call_of):
        out = []
        for v in values:
            r = oracle.p2p_sched_run(rows[:B.LADDER_CALLS], build(v), num_players=2, max_prediction=mp)
            assert r["rc"] in (0, -4)
            out.append(r["rc"] == -4 and r["result"].frames_done == call_of(v))
        return out

    for mp in (0, 8):
        s = stops_at(B.stall, B.STALLS, mp, lambda L: 20 + L)
        assert s == [L >= 126 for L in B.STALLS], (mp, s)
        s = stops_at(B.catch_up, B.CATCH_UP, mp, lambda u: 141)
        assert not s[0] and s[-1] and s == sorted(s), (mp, s)
    for lag in B.LAGS:
        out = oracle.p2p_sched_run(rows, B.rate(lag), num_players=2, max_prediction=0)
        assert out["rc"] == -4 and out["result"].frames_done == 252 + lag
        assert oracle.p2p_sched_run(rows, B.rate(lag), num_players=2, max_prediction=8)["rc"] == 0
