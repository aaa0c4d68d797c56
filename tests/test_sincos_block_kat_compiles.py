"""The device harness of the sin/cos-block KAT (tests/native/sincos_block_kat_device.hip, which
includes ggrs_amd/csrc/synctest_sincos_block.h as it stands) compiles for gfx950 with the product's
flags; tests/test_gpu_sincos_block_kat.py runs it."""
import os

from tests import step_form_cases as C


def test_device_harness_compiles(tmp_path):
    so = C.compile_kat("sincos_block_kat_device", tmp_path)
    assert os.path.getsize(so) > 0
