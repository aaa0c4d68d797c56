"""GPU parity of the spectator engine (ggrs_spectator_*, csrc/spectator.hip) against the Python
restatement of SpectatorSession (tests/spectator_model.py) stepped call by call under the same
per-session networks: jitter with stalls (calls that wait at PredictionThreshold, then a burst and
catch-up), fixed lags, hosts that outrun the spectator until it is lost (SpectatorTooFarBehind),
connect-status notes that wait for an Event::Input.  Every checked session's frames, wait count,
error, final state and per-call (advanced, checksum) trace are bit-exact."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # loads torch's HIP runtime before the engine library

from tests import spectator_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

S, CALLS, ROWS = 200, 240, 720
LAUNCHES = (1, 3, 60, 17, 159)
CASES = [(2, 10, 1), (2, 10, 3), (4, 4, 2), (3, 59, 58), (1, 1, 1)]
CHECKED = [s for s in range(S) if s % 3 == 0 or s % 8 in (3, 7) or s % 24 == 5]


@functools.lru_cache(maxsize=None)
def inputs_of(P, sessions=S, rows=ROWS):
    from oracle import oracle as o
    o.build()
    a = np.stack([o.gen_inputs(o.session_seed(s, 0x57EC + P), rows, P) for s in range(sessions)], axis=1)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(P, mfb, speed):
    """(rows, recv, notes, {session: model output}) of one parity case, computed once."""
    rows = inputs_of(P)
    recv, notes = M.schedules(S, CALLS, P, 11 + P)
    ref = {s: M.run(rows[:, s], recv[:, s], notes[:, s], num_players=P, max_frames_behind=mfb, catchup_speed=speed)
           for s in CHECKED}
    recv.setflags(write=False)
    notes.setflags(write=False)
    return rows, recv, notes, ref


def run_engine(P, mfb, speed, rows, recv, notes, launches, trace=True):
    from ggrs_amd import SpectatorEngine
    n_s = recv.shape[1]
    eng = SpectatorEngine(n_s, num_players=P, max_frames_behind=mfb, catchup_speed=speed, input_capacity=len(rows),
                          trace_capacity=len(recv) if trace else 0)
    eng.add_inputs(0, rows)
    eng.add_arrivals(0, recv, notes)
    for n in launches:
        eng.advance_frames(n)
    assert eng.calls() == sum(launches)
    return eng


def reads(eng, calls):
    cur, last, waited, err = eng.sessions()
    adv, cks = eng.trace(0, calls)
    return dict(cur=cur, last=last, waited=waited, err=err, states=eng.states(), adv=adv, cks=cks)


def check_against_model(got, ref, sessions):
    for s in sessions:
        m = ref[s]
        assert (got["cur"][s], got["last"][s], got["waited"][s], got["err"][s]) == \
            (m["current_frame"], m["last_recv"], m["waited"], m["error"]), s
        assert bytes(got["states"][s]) == bytes(m["state"]), s
        assert (got["adv"][:, s] == m["advanced"]).all(), (s, np.nonzero(got["adv"][:, s] != m["advanced"])[0][:4])
        assert (got["cks"][:, s] == m["checksums"]).all(), (s, np.nonzero(got["cks"][:, s] != m["checksums"])[0][:4])


@pytest.mark.parametrize("P,mfb,speed", CASES)
def test_spectators_match_the_model(oracle, P, mfb, speed):
    rows, recv, notes, ref = case(P, mfb, speed)
    # conditions on the inputs, from the model's outputs: a quiet schedule cannot hide a kernel bug
    waited = sum(m["waited"] for m in ref.values())
    fast_calls = sum(int((m["advanced"] > 1).sum()) for m in ref.values())
    lost = sum(m["error"] == M.E_TOO_FAR_BEHIND for m in ref.values())
    print(f"case ({P},{mfb},{speed}): waited {waited}, calls advancing > 1 frame {fast_calls}, too far behind {lost}")
    assert waited > 0
    if speed > 1:
        assert fast_calls >= S // 4
    if (P, mfb, speed) in ((2, 10, 1), (4, 4, 2)):
        assert 1 <= lost <= S // 4
    if (P, mfb, speed) == (2, 10, 3):
        assert lost == 0
    eng = run_engine(P, mfb, speed, rows, recv, notes, LAUNCHES)
    check_against_model(reads(eng, CALLS), ref, CHECKED)
    # one session through the single-session reads
    assert bytes(eng.state(CHECKED[-1])) == bytes(ref[CHECKED[-1]]["state"])
    eng.close()


def test_launch_split_does_not_matter(oracle):
    """One 240-call launch and 240 one-call launches read the same."""
    P, mfb, speed = 2, 10, 3
    rows, recv, notes, _ = case(P, mfb, speed)
    a = reads(run_engine(P, mfb, speed, rows, recv, notes, (CALLS,)), CALLS)
    b = reads(run_engine(P, mfb, speed, rows, recv, notes, (1,) * CALLS), CALLS)
    for k in a:
        assert (a[k] == b[k]).all(), k


@pytest.mark.parametrize("n_s", [1, 65])
def test_edge_session_counts_and_a_host_that_never_sends(oracle, n_s):
    from oracle import oracle as o
    P, mfb, speed, calls = 2, 10, 3, 64
    rows = inputs_of(P, 65, 128)[:, :n_s]
    recv, notes = M.schedules(n_s, calls, P, 5)
    recv[:, 0] = -1  # session 0 never receives frame 0
    eng = run_engine(P, mfb, speed, rows, recv, notes, (calls,))
    ref = {s: M.run(rows[:, s], recv[:, s], notes[:, s], num_players=P, max_frames_behind=mfb, catchup_speed=speed)
           for s in range(n_s)}
    got = reads(eng, calls)
    check_against_model(got, ref, range(n_s))
    assert (got["cur"][0], got["last"][0], got["waited"][0], got["err"][0]) == (-1, -1, calls, 0)
    assert bytes(got["states"][0]) == bytes(o.state_new(P))
    assert (got["adv"][:, 0] == 0).all() and (got["cks"][:, 0] == o.fletcher16(o.state_new(P))).all()
    eng.close()


def test_row_window_stops_only_the_session_that_fell_out(oracle):
    """input_capacity 64, rows added 32 per launch: session 5 stalls on its network at frame 10 while
    the host's rows run on; when frames up to 60 arrive at call 150 (inside the 60-frame buffer, so
    the session is not lost) the row it needs left the window and it stops with GGRS_E_PRECONDITION
    at that call.  Its neighbours run on."""
    from ggrs_amd import SpectatorEngine
    from ggrs_amd._lib import GGRS_E_PRECONDITION
    P, n_s, per, launches = 2, 66, 32, 6
    calls = per * launches
    rows = inputs_of(P, 66, 192)
    c = np.arange(calls)
    recv = np.repeat(np.maximum(c - 2, -1)[:, None], n_s, axis=1).astype(np.int32)
    recv[:, 5] = np.where(c < 150, np.minimum(c - 2, 10), 60)
    eng = SpectatorEngine(n_s, num_players=P, input_capacity=64, trace_capacity=calls)
    windows = []
    for j in range(launches):
        eng.add_inputs(per * j, rows[per * j:per * (j + 1)])
        eng.add_arrivals(per * j, recv[per * j:per * (j + 1)])
        eng.advance_frames(per)
        hi = per * (j + 1)
        windows.append((per, max(0, hi - 64), hi))
    sessions = [0, 4, 5, 6, 64, 65]
    ref = {s: M.run(rows[:, s], recv[:, s], num_players=P, windows=windows) for s in sessions}
    assert ref[5]["error"] == GGRS_E_PRECONDITION and ref[5]["current_frame"] == 10
    assert ref[5]["advanced"][:150].sum() == 11 and ref[5]["advanced"][150:].sum() == 0
    assert all(ref[s]["error"] == 0 and ref[s]["current_frame"] == calls - 3 for s in sessions if s != 5)
    got = reads(eng, calls)
    check_against_model(got, ref, sessions)
    assert (got["err"][np.arange(n_s) != 5] == 0).all()
    eng.close()


def test_spectators_of_the_device_host(oracle):
    """The P2P engine (fixed latency 3, max_prediction 8) as the host: after 100 calls the oldest cell
    of each session's ring (frame tag g) is confirmed; a spectator fed the same rows with recv_upto
    capped at g - 1 holds exactly that state."""
    from ggrs_amd import P2PEngine, SpectatorEngine
    P, n_s, calls = 2, 64, 100
    rows = inputs_of(P, 65, 128)[:calls, :n_s]
    host = P2PEngine(n_s, num_players=P, local_players=(0,), max_prediction=8, remote_latency=3, input_capacity=calls)
    host.add_inputs(0, rows)
    host.advance_frames(calls)
    checked = list(range(0, n_s, 3)) + [n_s - 1]
    rings = {s: host.ring(s) for s in checked}
    oldest = {s: int(np.argmin(np.where(rings[s][0] >= 0, rings[s][0], 1 << 30))) for s in checked}
    g = {s: int(rings[s][0][oldest[s]]) for s in checked}
    assert all(0 < g[s] < calls for s in checked)
    recv = np.zeros((calls, n_s), np.int32)
    for s in range(n_s):
        recv[:, s] = np.minimum(np.arange(calls), g.get(s, g[0]) - 1)
    spec = SpectatorEngine(n_s, num_players=P, input_capacity=128)
    spec.add_inputs(0, rows)
    spec.add_arrivals(0, recv)
    spec.advance_frames(calls)
    cur, _, _, err = spec.sessions()
    states = spec.states()
    for s in checked:
        assert cur[s] == g[s] - 1 and err[s] == 0, s
        assert bytes(states[s]) == bytes(rings[s][2][oldest[s]]), s
    host.close()
    spec.close()
