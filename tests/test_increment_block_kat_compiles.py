"""The device harness of the increment-block KAT (tests/native/increment_block_kat_device.hip, which
includes ggrs_amd/csrc/synctest_sincos_block.h and box_game.h as they stand) compiles for gfx950 with
the product's flags; tests/test_gpu_increment_block_kat.py runs it."""
import os

from tests import step_form_cases as C


def test_device_harness_compiles(tmp_path):
    so = C.compile_kat("increment_block_kat_device", tmp_path)
    assert os.path.getsize(so) > 0
