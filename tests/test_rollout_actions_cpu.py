"""The boundary of tron_rollout_actions without a GPU: the library exports it, the binding lists it, VecTron has the
method, and the ABI number has not moved (the symbol is an addition)."""
import ctypes as C
import os
import subprocess

import pytest


@pytest.fixture(scope="module")
def native():
    import tron.vec as tv
    if not os.path.exists(tv.nat.LIB_PATH):
        subprocess.check_call(["bash", os.path.join(os.path.dirname(tv.nat.LIB_PATH), "build.sh")])
    return tv.nat


def test_library_exports_the_symbol(native):
    assert hasattr(C.CDLL(native.LIB_PATH), "tron_rollout_actions")


def test_binding_lists_the_symbol(native):
    res, args = native.SIGNATURES["tron_rollout_actions"]
    assert res is C.c_int and len(args) == 8                     # h, k_steps, actions, flags, obs_fmt, obs, totals, stream
    assert args[1] is C.c_int32 and args[3] is C.c_uint32 and args[4] is C.c_int32
    assert native.lib().tron_rollout_actions.argtypes == args


def test_vectron_has_the_method():
    import tron.vec as tv
    assert callable(getattr(tv.VecTron, "rollout_actions", None))


def test_abi_version_unchanged(native):
    assert native.lib().tron_abi_version() == native.ABI_VERSION == 13
