"""The device functions of ggrs_amd/csrc/particles.h against the CPU oracle, bit for bit, through
the harness tests/native/particles_kat_device.hip; the cases and their references are
tests/particle_kat_cases.py's.

  test_pw_advance    advance_entity<false> on the step-form classes 1-6, advance_entity<true> on
                     classes 1-5, each with random and special payload rows and every input byte
  test_pw_checksum   fletcher_entity_mod per entity (c_e as the kernel forms it), summed in u32 and
                     finished by finish_checksum, against oracle.fletcher16 of the byte stream
  test_pw_checksum_largest_state   the same at N = 160000 (constant fills, two frame counters)
"""
import ctypes

import numpy as np
import pytest

from tests import particle_kat_cases as K
from tests import step_form_cases as C

pytestmark = pytest.mark.gpu


def _p(a, ct):
    return a.ctypes.data_as(ctypes.POINTER(ct))


class Kat:
    """The harness.  Every entry returns the HIP error code of its copies and launches; the first
    nonzero code fails the test that met it and every later call fails without launching."""

    def __init__(self, so):
        L = ctypes.CDLL(so)
        P = ctypes.POINTER
        u8, u16, u32, i32, i64 = ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int64
        L.kat_pw_advance.argtypes = [ctypes.c_int, i64, P(u32), P(u8), P(u32)]
        L.kat_pw_checksum.argtypes = [i64, i32, i32, P(i32), P(u32), P(u16)]
        self.L = L
        self.failed = None

    def call(self, name, *args):
        if self.failed:
            pytest.fail(f"not launched: {self.failed}")
        rc = getattr(self.L, name)(*args)
        if rc != 0:
            self.failed = f"{name} returned HIP error code {rc}"
            pytest.fail(self.failed)

    def advance(self, lean, words, inputs):
        w, inp = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(inputs, np.uint8)
        assert w.shape == (inp.size, K.FIELDS)
        out = np.zeros_like(w)
        self.call("kat_pw_advance", int(lean), w.shape[0], _p(w, ctypes.c_uint32), _p(inp, ctypes.c_uint8),
                  _p(out, ctypes.c_uint32))
        return out

    def checksum(self, N, frames, words):
        w = np.ascontiguousarray(words, np.uint32)
        assert w.shape[1:] == (N, K.FIELDS)
        fr = np.array(frames, np.int64).astype(np.int32)
        out = np.zeros((w.shape[0], fr.size), np.uint16)
        self.call("kat_pw_checksum", w.shape[0], N, fr.size, _p(fr, ctypes.c_int32), _p(w, ctypes.c_uint32),
                  _p(out, ctypes.c_uint16))
        return out


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    return Kat(C.compile_kat("particles_kat_device", tmp_path_factory.mktemp("particles_kat")))


@pytest.fixture(scope="module")
def prep(oracle):
    return C.prepared(oracle)


def _hex(row):
    return "[" + " ".join(f"{int(v):08x}" for v in row) + "]"


@pytest.mark.parametrize("lean", [False, True])
def test_pw_advance(kat, prep, oracle, lean):
    an = prep["an"]
    order = prep["orders"]["lean" if lean else "all", "interleaved"]
    if not lean:
        assert (an["cls"][order] == 6).any() and (an["players"][order][:, 4] == 0x80000000).any()  # out of domain, -0
    words, inputs = K.advance_cases(an, order, seed=77 + lean)
    assert words.shape[0] % 64 != 0 and np.unique(inputs).size == 256
    assert lean is False or (words[:, 4] <= C.TWO_PI_BITS).all()
    want = K.advance_reference(oracle, words, inputs)
    got = kat.advance(lean, words, inputs)
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        j = int(bad[0])
        cols = np.flatnonzero(got[j] != want[j]).tolist()
        by_word = (got[bad] != want[bad]).sum(axis=0).tolist()
        pytest.fail(f"advance_entity<{str(lean).lower()}>: {bad.size} of {words.shape[0]} lanes differ from the reference.  "
                    f"First: lane {j}, input 0x{int(inputs[j]):02x}, words {cols} (0-4 ship, 5-24 payload), in "
                    f"{_hex(words[j])}, reference {_hex(want[j])}, device {_hex(got[j])}.  Differing lanes by word {by_word}")


def _assert_checksums(name, N, frames, words, got, want):
    bad = np.argwhere(got != want)
    if bad.size:
        c, j = (int(v) for v in bad[0])
        pytest.fail(f"{name}: {bad.shape[0]} of {want.size} checksums differ from fletcher16 of the byte stream.  First: "
                    f"case {c}, frame 0x{int(frames[j]):08x}, N {N}: device {int(got[c, j]):04x}, oracle {int(want[c, j]):04x}; "
                    f"entity 0 {_hex(words[c, 0])}.  Differing by frame {(got != want).sum(axis=0).tolist()}")


@pytest.mark.parametrize("which", range(len(K.CHECKSUM_N) + 1))
def test_pw_checksum(kat, oracle, which):
    name, N, frames, words = K.checksum_sets()[which]
    want = K.checksum_reference(oracle, N, frames, words)
    got = kat.checksum(N, frames, words)
    _assert_checksums(name, N, frames, words, got, want)


def test_pw_checksum_largest_state(kat, oracle):
    words = K.big_cases()
    want = K.checksum_reference(oracle, K.BIG_N, K.BIG_FRAMES, words)
    for c in range(words.shape[0]):  # one 16 MB state per call
        got = kat.checksum(K.BIG_N, K.BIG_FRAMES, words[c:c + 1])
        _assert_checksums(f"fill 0x{K.CONST_FILLS[c]:02x} N={K.BIG_N}", K.BIG_N, K.BIG_FRAMES, words[c:c + 1], got, want[c:c + 1])
