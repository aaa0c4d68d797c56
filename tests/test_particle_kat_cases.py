"""CPU side of the particle-world KATs (tests/test_gpu_particles_kat.py): the case sets cover what
they claim to, the Python payload reference equals the oracle's particle world, and the device
harness compiles for gfx950 (so a header change that breaks it shows on a machine without a GPU)."""
import os

import numpy as np

from tests import particle_kat_cases as K
from tests import step_form_cases as C


def test_checksum_cases_cover_the_closed_form(oracle):
    sets = K.checksum_sets()
    assert [s[1] for s in sets] == list(K.CHECKSUM_N) + [8]
    # all 51 residues of c_e = 100 (N - e) mod 255 (the multiples of 5) meet a record
    for N in (52, 256, 260, 10000, K.BIG_N):
        assert set(K.c_e(N).tolist()) == set(range(0, 255, 5))
    assert len(set(K.c_e(8).tolist())) == 8
    # per-entity byte sums: remainder 0 from a zero and from a nonzero sum, and remainder 254
    res = np.concatenate([K.byte_sum_residues(s[3]) for s in sets])
    assert (res == 254).any() and (res == 0).any()
    ff = np.full((1, K.FIELDS), 0xFFFFFFFF, np.uint32)
    assert K.byte_sum_residues(ff)[0] == 0 and any((s[3] == 0xFFFFFFFF).all(axis=(1, 2)).any() for s in sets)
    assert set(res.tolist()) == set(range(255))
    # every byte of the frame counter is nonzero in some case, in the 160000-entity set too
    for frames in (K.FRAMES, K.BIG_FRAMES):
        for b in range(4):
            assert any((f >> (8 * b)) & 0xFF for f in frames)
        assert any(all((f >> (8 * b)) & 0xFF for b in range(4)) for f in frames)
        assert all(0 <= f <= 0x7FFFFFFF for f in frames)
    # the single-byte set: each of the 100 in-record positions of the first and the last entity, both values
    sb = K.single_byte_cases(8)
    by = np.ascontiguousarray(sb, "<u4").view(np.uint8).reshape(sb.shape[0], -1)
    assert ((by != 0).sum(axis=1) == 1).all()
    where = {(int(r.argmax()), int(r.max())) for r in by}
    assert where == {(e * 100 + j, v) for e in (0, 7) for j in range(100) for v in (1, 255)}
    # the byte layout the references hash is the oracle's: its frame-0 state re-serialised from words
    r = oracle.particles_synctest_run(np.zeros((0, 2), np.uint8), 8, 2, 4, 2, session=3)
    st = np.asarray(r["final_state"], np.uint8)
    words = st[4:].view("<u4").reshape(8, K.FIELDS)
    assert np.array_equal(K.stream_bytes(0, words), st)
    assert int(oracle.fletcher16_batch(st[None])[0]) == oracle.fletcher16(st.tobytes())


def test_special_payload_rows_cover_the_shift_and_the_wrap():
    sp = K.special_payload_rows()
    assert (sp == 0).all(axis=1).any() and (sp == 0xFFFFFFFF).all(axis=1).any()
    for v in (0x7F, 0x80, 0xFFFFFF80):
        assert (sp == v).all(axis=1).any()
    assert (sp[:, 19] != sp[:, 0]).any()
    # a wrap that read the NEW p[0] would give another p'[19] on some special row
    differs = 0
    for row in sp:
        new = K.payload_step_int(row, 0)
        differs += ((int(row[19]) * K.PAYLOAD_MUL + (new[0] >> 7)) & K.M32) != new[19]
    assert differs > 0


def test_payload_reference_equals_the_oracle(oracle):
    """payload_step (numpy) and payload_step_int (Python ints) against the payload words of
    oracle.particles_synctest_run over 3 frames at N = 4, and against each other on the KAT's rows."""
    N, P = 4, 2
    inp = oracle.gen_inputs(oracle.session_seed(5), 3, P, 1)
    inp[1] = [0xFF, 0x80]  # whole bytes enter the payload
    states = []
    for f in range(4):
        r = oracle.particles_synctest_run(inp[:f], N, P, 3, 0, session=5, ring_states=False)
        assert r["rc"] == 0 and r["result"].status == 0
        st = np.asarray(r["final_state"], np.uint8)
        assert int(st[:4].view("<u4")[0]) == f
        states.append(st[4:].view("<u4").reshape(N, K.FIELDS).astype(np.uint32))
    for f in range(3):
        per_entity = inp[f][np.arange(N) % P]
        want = states[f + 1]
        assert np.array_equal(K.payload_step(states[f][:, 5:], per_entity), want[:, 5:]), f
        for e in range(N):
            assert K.payload_step_int(states[f][e, 5:], per_entity[e]) == want[e, 5:].tolist()
        assert np.array_equal(K.advance_reference(oracle, states[f], per_entity), want), f
    rng = np.random.default_rng(3)
    rows = np.concatenate([K.special_payload_rows(), rng.integers(0, 1 << 32, (64, K.PAYLOAD), dtype=np.uint64).astype(np.uint32)])
    for b in (0, 1, 0x7F, 0x80, 0xFF):
        got = K.payload_step(rows, np.full(rows.shape[0], b, np.uint8))
        assert got.tolist() == [K.payload_step_int(r, b) for r in rows]


def test_device_harness_compiles(tmp_path):
    so = C.compile_kat("particles_kat_device", tmp_path)
    assert os.path.getsize(so) > 0
