"""The boundary of tron_rollout_actions_records without a GPU: the library exports it, the binding lists it with its eleven
arguments, VecTron.rollout_actions takes `records`, and the ABI number has not moved (the symbol is an addition)."""
import ctypes as C
import inspect
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
    assert hasattr(C.CDLL(native.LIB_PATH), "tron_rollout_actions_records")


def test_binding_lists_the_symbol(native):
    res, args = native.SIGNATURES["tron_rollout_actions_records"]
    # h, k_steps, actions, flags, obs_fmt, obs, out_done, out_winner, out_reward, totals, stream
    assert res is C.c_int and len(args) == 11
    assert args[1] is C.c_int32 and args[3] is C.c_uint32 and args[4] is C.c_int32
    assert all(args[i] is C.c_void_p for i in (0, 2, 5, 6, 7, 8, 9, 10))
    assert native.lib().tron_rollout_actions_records.argtypes == args
    assert len(native.SIGNATURES["tron_rollout_actions"][1]) == 8     # the call without records keeps its arguments


def test_rollout_actions_takes_records():
    import tron.vec as tv
    p = inspect.signature(tv.VecTron.rollout_actions).parameters
    assert list(p) == ["self", "actions", "totals", "per_step_launches", "records"]
    assert p["records"].default is None


def test_abi_version_unchanged(native):
    assert native.lib().tron_abi_version() == native.ABI_VERSION == 13
