"""CPU side of the step-form KATs (tests/test_gpu_step_forms.py): the oracle's batch single-step
entries equal the one-state-at-a-time entry on the KAT's own cases, the cases cover what they claim
to, and the device harness compiles for gfx950 (so a header change that breaks it shows on a
machine without a GPU)."""
import os
import re

import numpy as np
import pytest

from tests import step_form_cases as C


@pytest.fixture(scope="module")
def prep(oracle):
    return C.prepared(oracle)


def test_cases_cover_their_classes(prep):
    """prepared() asserts every coverage and wave-layout count > 0; the bounds the issue sets on the
    case set itself are checked here."""
    an = prep["an"]
    per_class = {k: int((an["state_cls"] == k).sum()) for k in C.CLASS_NAMES}
    assert all(v > 0 for v in per_class.values()), per_class
    assert per_class[1] + per_class[3] <= 1 << 16           # the random part
    assert an["inputs"].size == 16 * an["states"].shape[0]
    low = (an["inputs"] & 15).reshape(-1, 16)
    assert (low == np.arange(16)).all()                     # every state meets all 16 direction inputs
    m2 = an["mag2"][an["cls"] == 3]
    assert (m2 < 49).any() and (m2 == 49).any() and (m2 > 49).any()
    edges = set(C.rotation_edges().tolist())
    assert {0, 1, C.TWO_PI_BITS} <= edges and C.bits_of(C.ROTATION_SPEED) in edges
    assert edges <= set(an["states"][an["state_cls"] == 5][:, 4].tolist())
    ood = C.u2f(an["states"][an["state_cls"] == 6][:, 4])
    exps = set((np.frexp(np.abs(ood[np.abs(ood) >= 120.0]).astype(np.float64))[1] - 1).tolist())
    assert exps == set(range(6, 127))                       # |rot| in [120, 2^127): every exponent
    assert (an["states"][:, 4] == 0x80000000).any() and ((ood < 0) & (ood > -C.ROTATION_SPEED)).any()


def test_ship_step_batch_equals_state_advance(oracle, prep):
    an = prep["an"]
    sample = np.unique(np.concatenate([np.arange(0, an["inputs"].size, 499), np.flatnonzero(an["cls"] == 6)[::23],
                                       np.flatnonzero(an["mag2"] == np.float32(49.0))[::97]]))
    got = oracle.ship_step_batch(an["players"][sample], an["inputs"][sample])
    assert np.array_equal(got, an["ref"][sample])
    one = np.zeros((1, 6), np.uint32)
    for j, k in enumerate(sample):
        one[0, 1:] = an["players"][k]
        after = oracle.state_advance(C.words_to_bincode(1, one)[0], an["inputs"][k:k + 1])
        assert np.array_equal(C.bincode_to_words(1, after[None])[0, 1:], got[j]), int(k)


@pytest.mark.parametrize("P", [1, 2, 3, 4])
def test_state_advance_batch_equals_state_advance(oracle, prep, P):
    s = C.state_lanes(prep["an"], prep["every"], P, seed=100 + P, with_disconnects=True)
    pick = np.unique(np.concatenate([np.arange(0, s["words"].shape[0], 97), np.flatnonzero(s["disc"])[::13]]))
    before = C.words_to_bincode(P, s["words"][pick])
    assert np.array_equal(C.bincode_to_words(P, before), s["words"][pick])
    after = oracle.state_advance_batch(before, s["inputs"][pick], s["status"][pick])
    cks = oracle.fletcher16_batch(after)
    for j in range(pick.size):
        assert np.array_equal(oracle.state_advance(before[j], s["inputs"][pick[j]], s["status"][pick[j]]), after[j])
        assert oracle.fletcher16(after[j].tobytes()) == int(cks[j])
    # status None is all Confirmed
    assert np.array_equal(oracle.state_advance_batch(before, s["inputs"][pick]),
                          oracle.state_advance_batch(before, s["inputs"][pick], np.zeros((pick.size, P), np.uint8)))
    wrong = before[:1].copy()
    wrong[0, 4] = P % 4 + 1  # num_players that contradicts the row size
    with pytest.raises(ValueError):
        oracle.state_advance_batch(wrong, s["inputs"][pick[:1]])


def test_largest_players_form_is_the_products():
    """advance_players_rec<N>'s largest N: the rounds pipeline's eight stages plus four trunk players"""
    src = open(os.path.join(C.ROOT, "ggrs_amd", "csrc", "branch.hip")).read()
    stages = int(re.search(r"constexpr int kPipeMaxW = (\d+);", src).group(1))
    assert "NS = NK + NT" in src and stages + 4 == C.MAX_PLAYERS_REC


def test_device_harness_compiles(tmp_path):
    so = C.compile_kat("step_forms_kat_device", tmp_path)
    assert os.path.getsize(so) > 0
