"""The batches tests/test_gpu_head_dispatch.py runs sit on the code paths it claims: the K-slice count of the head's conv7 product
(wide_splitk in csrc/tron_head.hip) read back from tron_dqn_head_workspace.  No device work: the size query is host arithmetic."""
import ctypes
import os

import pytest

from conftest import PKG
from head_support import BATCHES, NARROW_ROWS, SLICES, head_slices


@pytest.fixture(scope="module")
def L():
    so = os.path.join(PKG, "csrc", "libtron_hip.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.check_call(["bash", os.path.join(PKG, "csrc", "build.sh")])
    lib = ctypes.CDLL(so)                                               # the C ABI of include/tron_hip.h, nothing in between
    lib.tron_dqn_head_workspace.restype = ctypes.c_int64
    lib.tron_dqn_head_workspace.argtypes = [ctypes.c_int64, ctypes.c_int32]
    return lib


def test_head_batches_sit_on_the_paths_they_claim(L):
    """1280 | 1281 .. 3328 | 3329 .. 6784 | 6785: the 128 x 64 tile, four slices, two slices, the 128 x 192 tile alone (no partial
    area, like the first).  If this fails the thresholds were retuned: move BATCHES in tests/head_support.py to the new boundaries,
    or the GPU tests stop covering a path without any of them failing."""
    got = tuple(head_slices(L, B) for B in BATCHES)
    assert got == SLICES, dict(zip(BATCHES, got))
    assert head_slices(L, NARROW_ROWS) == 0 and NARROW_ROWS <= BATCHES[0]
    assert head_slices(L, 4099) == 2 and head_slices(L, 16384) == 0     # what the older head tests and the benchmark batch take
