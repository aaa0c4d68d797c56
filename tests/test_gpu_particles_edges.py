"""The config-5 particle world SyncTest (ggrs_particle_*, ggrs_amd/csrc/particles.hip) at the edges
tests/test_gpu_particles.py does not reach, bit-exact against the oracle's restatement: the input
ring wrapping (and its queue bound), check distances whose Fletcher slots pass 64 KB of LDS, frame
counters past 65535, first_session_id, the frame-0 state, mismatch reports at every edge of the
compare range and across launches, the smallest and the pass-boundary entity counts, the plain
store path, and the calls the ABI rejects.

check_engine is the one comparison: for EVERY session, state(s), every live ring cell (checksum and
bytes) and the mismatch report against oracle.particles_synctest_run of that session's inputs."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPTS = ["1", "2", "4"]  # entities per thread (GGRS_PW_EPT)
_oracle_runs = {}       # the oracle's run of (shape, session, inputs, corruption): shared by the EPT cases


def inputs_for(O, sessions, frames, P, first=0):
    return np.stack([O.gen_inputs(O.session_seed(first + s), frames, P, 1) for s in range(sessions)], axis=1)


def oracle_run(O, inp, shape, session, corrupt_frame=-1):
    """oracle.particles_synctest_run of one session's inputs [frames][P] (computed once, never changed)"""
    N, P, maxp, cd = shape
    a = np.ascontiguousarray(inp, np.uint8).reshape(-1, P)
    key = (shape, session, corrupt_frame, a.tobytes())
    if key not in _oracle_runs:
        r = O.particles_synctest_run(a, N, P, maxp, cd, session=session, corrupt_frame=corrupt_frame)
        assert r["rc"] == 0 and r["result"].status in (0, 1)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle_runs[key] = r
    return _oracle_runs[key]


def check_engine(O, eng, inp, done, shape, first=0, corrupt=None, what=""):
    """After `done` frames of inp [frames][S][P]: every session's state, live ring cells and
    mismatch report equal the oracle's run of session first + s (corrupt: {session: call whose
    load is corrupted}).  A session the oracle halts stops at its mismatch frame whatever follows."""
    corrupt = corrupt or {}
    S = inp.shape[1]
    st, mf, mm = eng.mismatches()
    runs = []
    for s in range(S):
        r = oracle_run(O, inp[:done, s, :], shape, first + s, corrupt.get(s, -1))
        runs.append(r)
        res = r["result"]
        tag = f"{what} session {s} after {done} frames"
        assert int(st[s]) == res.status, tag
        if res.status == 1:
            assert int(mf[s]) == res.mismatch_frame and int(mm[s]) == int(res.mismatch_mask), tag
        else:
            assert res.frames_done == done, tag
        assert bytes(eng.state(s)) == bytes(r["final_state"]), f"{tag}: state"
        for fr, ck, cell in zip(r["ring_frames"], r["ring_cksums"], r["ring_states"]):
            if fr >= 0:
                gck, gst = eng.saved(s, int(fr))
                assert gck == int(ck), f"{tag}: checksum of saved frame {int(fr)}: {gck:04x}, oracle {int(ck):04x}"
                assert bytes(gst) == bytes(cell), f"{tag}: bytes of saved frame {int(fr)}"
    return runs


def make_engine(monkeypatch, ept, S, shape, capacity, first=0):
    from ggrs_amd import ParticleEngine
    monkeypatch.setenv("GGRS_PW_EPT", ept)
    N, P, maxp, cd = shape
    return ParticleEngine(S, N, P, maxp, cd, input_capacity=capacity, first_session_id=first)


def run_launches(O, monkeypatch, ept, S, shape, launches, first=0, what=""):
    """all inputs up front (a queue as long as the run), the launches, check_engine at the end"""
    frames = sum(launches)
    inp = inputs_for(O, S, frames, shape[1], first)
    eng = make_engine(monkeypatch, ept, S, shape, frames + shape[3] + 2, first)
    eng.add_local_inputs(inp)
    done = 0
    for n in launches:
        eng.synctest_advance_frames(n)
        done += n
    assert eng.current_frame() == done == frames
    check_engine(O, eng, inp, frames, shape, first, what=what)
    eng.close()


# ---------------------------------------------------------------- A1
@pytest.mark.parametrize("ept", EPTS)
def test_input_ring_wraps(oracle, monkeypatch, ept):
    """Inputs fed and consumed in lock step through a queue of cd + 4 frames: every index into it
    (the replay's g % cap, the feed's (q0 + fr) % cap, the materialised state's f % cap) wraps 33
    times, and the frame counter passes 255."""
    from ggrs_amd import InvalidRequest
    S, shape = 3, (260, 3, 6, 5)
    cd = shape[3]
    cap = cd + 4
    frames = 300
    inp = inputs_for(oracle, S, frames + 8, shape[1])
    eng = make_engine(monkeypatch, ept, S, shape, cap)
    checkpoints = {4, 10, 18, 128, 258, 294}  # warm-up; straight after the first wrap (frame 9 -> slot 0); ...; past 256
    done, k, seen = 0, 0, set()
    while done < frames:
        n = (4, 1, 3, 2)[k % 4]  # 4 = cap - cd is the largest chunk the queue admits
        k += 1
        eng.add_local_inputs(inp[done:done + n])
        eng.synctest_advance_frames(n)
        done += n
        if done in checkpoints:
            seen.add(done)
            check_engine(oracle, eng, inp, done, shape, what="cap 9")
            if done == 128:  # read twice in a row: the materialised state and the cells stay
                check_engine(oracle, eng, inp, done, shape, what="cap 9, second read")
        if done == 130:  # one frame more than fits: refused, and nothing is taken
            with pytest.raises(InvalidRequest, match="input queue full"):
                eng.add_local_inputs(inp[done:done + cap - cd + 1])
            assert eng.current_frame() == done
    assert seen == checkpoints and done == frames == eng.current_frame()
    check_engine(oracle, eng, inp, frames, shape, what="cap 9")
    eng.close()


@pytest.mark.parametrize("ept", EPTS)
def test_input_ring_wraps_under_a_mismatch(oracle, monkeypatch, ept):
    """The halted session's state is Advance(cell f-1, input (f-1) % cap): with the same short queue,
    a load corrupted at call 40 is reported at 41, whose previous input sits in a wrapped slot."""
    S, shape, call = 3, (260, 3, 6, 5), 40
    cap = shape[3] + 4
    inp = inputs_for(oracle, S, 60, shape[1])
    eng = make_engine(monkeypatch, ept, S, shape, cap)
    eng.corrupt_on_load(1, call)
    want = oracle_run(oracle, inp[:, 1, :], shape, 1, call)["result"]
    assert want.status == 1 and want.mismatch_frame == call + 1 and (want.mismatch_frame - 1) % cap != want.mismatch_frame - 1
    done, k = 0, 0
    while done < 60:
        n = (4, 1, 3, 2)[k % 4]
        k += 1
        eng.add_local_inputs(inp[done:done + n])
        eng.synctest_advance_frames(n)
        done += n
        if done in (40, 44, 60):  # before the report; its launch (calls 40..43); five launches later
            check_engine(oracle, eng, inp, done, shape, corrupt={1: call}, what="cap 9, corrupted load")
    assert eng.mismatches()[0].tolist() == [0, 1, 0]
    eng.close()


@pytest.mark.parametrize("ept", EPTS)
def test_input_ring_wraps_default_capacity(oracle, monkeypatch, ept):
    """input_capacity = 0 selects 128 frames: its bound (cap - cd = 123 frames at once) and its wrap"""
    from ggrs_amd import InvalidRequest
    S, shape = 3, (260, 3, 6, 5)
    inp = inputs_for(oracle, S, 140, shape[1])
    eng = make_engine(monkeypatch, ept, S, shape, 0)
    with pytest.raises(InvalidRequest, match="input queue full"):
        eng.add_local_inputs(inp[:124])
    done = 0
    for n in (123, 1, 16):
        eng.add_local_inputs(inp[done:done + n])
        eng.synctest_advance_frames(n)
        done += n
        check_engine(oracle, eng, inp, done, shape, what="default capacity")
    assert done == 140
    eng.close()


# ---------------------------------------------------------------- A2
@pytest.mark.parametrize("N,P,maxp,cd", [
    (8, 2, 63, 62),    # the largest check distance: 129,024 B of Fletcher slots, mask bits up to 60
    (260, 1, 40, 32),  # the first past 64 KB (the large-LDS opt-in at creation)
    (64, 2, 33, 31),   # exactly 64 KB, the last without the opt-in
])
@pytest.mark.parametrize("ept", EPTS)
def test_large_check_distance(oracle, monkeypatch, ept, N, P, maxp, cd):
    frames = 2 * cd + 10
    a = cd + 3
    run_launches(oracle, monkeypatch, ept, 3, (N, P, maxp, cd), [a, 1, frames - a - 1], what=f"cd {cd}")


# ---------------------------------------------------------------- A3
@pytest.mark.parametrize("ept", ["1", "4"])
def test_frame_counter_bytes(oracle, monkeypatch, ept):
    """Frames past 65535: bytes 1 and 2 of the frame word are nonzero in every live ring cell, so
    finish_checksum's weights of those bytes count."""
    S, shape = 2, (4, 2, 3, 2)
    launches = [65530, 3, 3, 10]
    frames = sum(launches)
    inp = inputs_for(oracle, S, frames, shape[1])
    eng = make_engine(monkeypatch, ept, S, shape, frames + shape[3] + 2)
    eng.add_local_inputs(inp)
    done = 0
    for i, n in enumerate(launches):
        eng.synctest_advance_frames(n)
        done += n
        if i > 0:
            runs = check_engine(oracle, eng, inp, done, shape, what="frame bytes")
    live = [int(f) for f in runs[0]["ring_frames"] if f >= 0]  # at the end
    assert live and min(live) >= 65536 and all((f >> 16) & 0xFF for f in live)
    eng.close()


# ---------------------------------------------------------------- A4
@pytest.mark.parametrize("ept", EPTS)
def test_first_session_id(oracle, monkeypatch, ept):
    S, shape, launches = 3, (64, 2, 4, 3), [2, 4, 6]
    run_launches(oracle, monkeypatch, ept, S, shape, launches, first=7, what="first_session_id 7")
    # engines A (sessions 0..2) and B (sessions 2..4): A's session 2 and B's session 0 are the same session
    frames = sum(launches)
    ia, ib = inputs_for(oracle, S, frames, shape[1], 0), inputs_for(oracle, S, frames, shape[1], 2)
    assert np.array_equal(ia[:, 2], ib[:, 0]) and not np.array_equal(ia[:, 0], ib[:, 0])
    A = make_engine(monkeypatch, ept, S, shape, frames + 5, first=0)
    B = make_engine(monkeypatch, ept, S, shape, frames + 5, first=2)
    assert bytes(A.state(2)) == bytes(B.state(0)) and bytes(A.state(0)) != bytes(B.state(0))
    for eng, inp in ((A, ia), (B, ib)):
        eng.add_local_inputs(inp)
        for n in launches:
            eng.synctest_advance_frames(n)
    ra = check_engine(oracle, A, ia, frames, shape, first=0, what="engine A")
    check_engine(oracle, B, ib, frames, shape, first=2, what="engine B")
    assert bytes(A.state(2)) == bytes(B.state(0))
    for fr in ra[2]["ring_frames"]:
        if fr >= 0:
            (cka, sta), (ckb, stb) = A.saved(2, int(fr)), B.saved(0, int(fr))
            assert cka == ckb and bytes(sta) == bytes(stb), int(fr)
    A.close()
    B.close()


# ---------------------------------------------------------------- A5
@pytest.mark.parametrize("N", [4, 12, 260, 10000])
@pytest.mark.parametrize("ept", EPTS)
def test_initial_state(oracle, monkeypatch, ept, N):
    """state(s) at frame 0, before any advance: pw_init_kernel against the oracle's run over zero frames"""
    S, shape = 3, (N, 2, 4, 2)
    eng = make_engine(monkeypatch, ept, S, shape, 8)
    assert eng.current_frame() == 0
    runs = check_engine(oracle, eng, np.zeros((0, S, 2), np.uint8), 0, shape, what="frame 0")
    assert all((r["ring_frames"] < 0).all() for r in runs)
    assert len({bytes(eng.state(s)) for s in range(S)}) == S  # the payload is per session
    eng.close()


# ---------------------------------------------------------------- A6
@pytest.mark.parametrize("split", ["corrupt call last of its launch", "corrupt call first of its launch"])
@pytest.mark.parametrize("cd,call", [(1, 3), (2, 3), (2, 7), (3, 4), (62, 63), (62, 67)])
@pytest.mark.parametrize("N", [8, 128])
@pytest.mark.parametrize("ept", EPTS)
def test_mismatch_edges(oracle, monkeypatch, ept, N, cd, call, split):
    """A load corrupted at `call`: the report (status, frame, mask) is the oracle's for the one-bit
    compare range (cd 2), the empty one (cd 1: never reported) and masks past bit 31 (cd 62), with
    the detection in a later launch than the corruption or in the same; the halted session stays
    frozen over further launches while its neighbours go on matching the oracle."""
    S, shape = 3, (N, 2, cd + 1, cd)
    first_launch = call + 1 if split.endswith("last of its launch") else call
    launches = [first_launch, 3, 2, 4]
    frames = sum(launches)
    inp = inputs_for(oracle, S, frames, shape[1])
    for bad in (0, 1, 2):  # the corrupted session first, in the middle, last
        corrupted = oracle_run(oracle, inp[:, bad, :], shape, bad, call)
        want = corrupted["result"]
        if cd == 1:  # the compare range f-cd .. f-2 is empty: the corruption goes on unreported
            assert want.status == 0
            assert bytes(corrupted["final_state"]) != bytes(oracle_run(oracle, inp[:, bad, :], shape, bad)["final_state"])
        else:  # reported by the next call: the first of the second launch, or its second
            assert want.status == 1 and want.mismatch_frame == call + 1 and want.mismatch_mask != 0
            if cd == 62:
                assert int(want.mismatch_mask) >> 32 != 0  # the case is about mask bits past 31
        eng = make_engine(monkeypatch, ept, S, shape, frames + cd + 2)
        eng.corrupt_on_load(bad, call)
        eng.add_local_inputs(inp)
        done = 0
        frozen = None
        for i, n in enumerate(launches):
            eng.synctest_advance_frames(n)
            done += n
            if i == 0:
                assert (eng.mismatches()[0] == 0).all()  # not yet compared: call + 1 is the earliest report
            if i == 1:  # the report's launch
                check_engine(oracle, eng, inp, done, shape, corrupt={bad: call}, what=f"corrupt {bad}, detection launch")
                st, mf, mm = eng.mismatches()
                if cd > 1:
                    assert st.tolist() == [int(s == bad) for s in range(S)]
                    cells = [eng.saved(bad, f) for f in range(want.mismatch_frame - cd, want.mismatch_frame)]
                    frozen = (bytes(eng.state(bad)), int(mf[bad]), int(mm[bad]), [(c, bytes(b)) for c, b in cells])
        check_engine(oracle, eng, inp, frames, shape, corrupt={bad: call}, what=f"corrupt {bad}, two launches later")
        st, mf, mm = eng.mismatches()
        if cd > 1:
            cells = [eng.saved(bad, f) for f in range(want.mismatch_frame - cd, want.mismatch_frame)]
            assert frozen == (bytes(eng.state(bad)), int(mf[bad]), int(mm[bad]), [(c, bytes(b)) for c, b in cells])
            assert int.from_bytes(bytes(eng.state(bad))[:4], "little") == want.mismatch_frame
            assert st.tolist() == [int(s == bad) for s in range(S)]
        else:
            assert (st == 0).all()
        eng.close()


# ---------------------------------------------------------------- A7
def _count_edges(ept):
    return [4, 8, 252, 256, 260, 1024 * int(ept) + 4]  # ... and one unit past a full pass of 256 threads x 4 passes


@pytest.mark.parametrize("ept,N", [(e, n) for e in EPTS for n in _count_edges(e)])
def test_entity_count_edges(oracle, monkeypatch, ept, N):
    run_launches(oracle, monkeypatch, ept, 3, (N, 3, 4, 2), [1, 3, 5], what=f"N {N}")


# ---------------------------------------------------------------- A8
@pytest.mark.parametrize("N,P,maxp,cd,launches", [(260, 3, 4, 2, [1, 3, 5]), (1024, 3, 8, 7, [30])])
@pytest.mark.parametrize("ept", EPTS)
def test_plain_store_path(oracle, monkeypatch, ept, N, P, maxp, cd, launches):
    monkeypatch.setenv("GGRS_PW_STORE", "plain")
    run_launches(oracle, monkeypatch, ept, 3, (N, P, maxp, cd), launches, what="plain stores")


# ---------------------------------------------------------------- A9
def test_rejected_calls(oracle, monkeypatch):
    from ggrs_amd import InvalidRequest, ParticleEngine, PreconditionError
    from ggrs_amd import _lib
    monkeypatch.delenv("GGRS_PW_EPT", raising=False)
    good = dict(num_sessions=3, num_entities=64, num_players=2, max_prediction=4, check_distance=2, input_capacity=16)
    for change in (dict(num_entities=0), dict(num_entities=6), dict(num_entities=160004),
                   dict(num_players=0), dict(num_players=5),
                   dict(check_distance=4), dict(check_distance=63, max_prediction=64), dict(max_prediction=64),
                   dict(input_capacity=3), dict(num_sessions=0)):
        with pytest.raises(InvalidRequest):
            ParticleEngine(**{**good, **change})
    S, shape = 3, (64, 2, 4, 2)
    inp = inputs_for(oracle, S, 12, 2)
    eng = ParticleEngine(**good)
    with pytest.raises(PreconditionError):
        eng.saved(0, 0)  # nothing saved yet
    for wrong in (inp[:2, :2], inp[:2, :, :1], inp[0]):
        with pytest.raises(InvalidRequest):
            eng.add_local_inputs(wrong)
    eng.add_local_inputs(inp[:6])
    a = np.ascontiguousarray(inp[6:7])
    for first_frame in (5, 7, 0):  # the next frame is 6
        rc = eng._L.ggrs_particle_add_local_inputs(eng._h, first_frame, 1, ctypes.c_void_p(a.ctypes.data))
        assert rc == _lib.GGRS_E_INVALID
        with pytest.raises(InvalidRequest, match="sequentially"):
            _lib.check(rc)
    eng.synctest_advance_frames(4)
    before = bytes(eng.state(0))
    eng.timing_reset()
    with pytest.raises(InvalidRequest, match="Missing local input"):
        eng.synctest_advance_frames(3)  # frames 4, 5, 6: 6 was never added
    assert eng.timing_read()[1] == 0  # nothing was launched
    assert eng.current_frame() == 4 and bytes(eng.state(0)) == before
    eng.synctest_advance_frames(2)
    check_engine(oracle, eng, inp, 6, shape, what="after a refused advance")
    eng.add_local_inputs(inp[6:12])
    eng.synctest_advance_frames(6)
    check_engine(oracle, eng, inp, 12, shape, what="after refused calls")
    for s in (-1, S):
        with pytest.raises(InvalidRequest):
            eng.state(s)
        with pytest.raises(InvalidRequest):
            eng.saved(s, 11)
    with pytest.raises(InvalidRequest):
        eng.saved(0, -1)
    r = oracle_run(oracle, inp[:12, 0, :], shape, 0)
    assert sorted(int(f) for f in r["ring_frames"]) == [7, 8, 9, 10, 11]  # R = 5 cells
    assert eng.saved(0, 11)[0] == int(r["ring_cksums"][r["ring_frames"].tolist().index(11)])
    for never_or_overwritten in (12, 40, 6, 0):
        with pytest.raises(PreconditionError):
            eng.saved(0, never_or_overwritten)
    check_engine(oracle, eng, inp, 12, shape, what="after refused reads")
    eng.close()
