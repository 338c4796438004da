"""The host model of the learner's work split (tests/px_items_support.py) against the source it restates, and the batches it
chooses for tests/test_gpu_px_items.py: a changed geometry fails here instead of silently un-covering the GPU tests."""
import ctypes
import os
import re

import pytest

from conftest import PKG
import px_items_support as P

TRAIN_HIP = os.path.join(PKG, "csrc", "tron_conv_ws_train.hip")
KERNEL_HPP = os.path.join(PKG, "csrc", "tron_conv_ws_kernel.hpp")
CUS = (64, 104, 256, 304)
CAP = 150e6                                                          # bytes of the largest f32 tensor of a GPU test


@pytest.fixture(scope="module")
def source():
    with open(TRAIN_HIP) as f:
        return f.read()


def _ints(s):
    return tuple(int(v) for v in s.split(","))


def test_wgrad_table_is_the_source_s(source):
    body = source[source.index("int dispatch_wgrad_px("):]
    body = body[:body.index("return TRON_ERR_UNSUPPORTED")]
    found = {}
    for cin, cout, args in re.findall(r"if \(cin == (\d+) && cout == (\d+)\) return f\(WCfg<([\d, ]+)>\{\}\);", body):
        S, NI, R, CO, CI, COT, CIT, KG = _ints(args)
        assert (CO, CI) == (int(cout), int(cin)), args
        side = re.findall(r"side == (\d+)", body[:body.index(f"WCfg<{args}>")])[-1]        # the branch the line stands in
        assert int(side) == S, args
        assert (S, CI, CO) not in found
        found[(S, CI, CO)] = dict(NI=NI, R=R, COT=COT, CIT=CIT, KG=KG)
    assert len(found) == 9 and found == P.WGRAD_CFG
    assert set(found) == set(P.SHAPES)


def test_backward_table_is_the_source_s(source):
    cases = re.findall(r"^\s*TRON_WSB_CASE\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", source, flags=re.M)
    assert len(cases) == 9
    # TRON_WSB_CASE(S, R, CI, CO, IPI, WAVES) is taken when cout == CI and cin == CO
    assert re.search(r"#define TRON_WSB_CASE\(S_, R_, CI_, CO_, IPI_, WAVES_\)\s*\\\n\s*if \(side == S_ && cout == CI_ && cin == CO_\)", source)
    found = {(int(S), int(CO), int(CI)): dict(R=int(R), IPI=int(IPI)) for S, R, CI, CO, IPI, _ in cases}
    assert len(found) == 9 and found == P.WSB_CFG


def test_forward_table_is_the_source_s(source):
    cases = re.findall(r"TRON_WST_CASE\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+), MODE_, ARGS_\)", source)
    assert len(cases) == 9
    assert "if (side == S_ && cin == CI_ && cout == CO_) return launch_ws<Geo<S_, R_, CI_, CO_, IPI_, WAVES_, 1>, MODE_> ARGS_;" in source
    found = {(int(S), int(CI), int(CO)): dict(R=int(R), IPI=int(IPI)) for S, R, CI, CO, IPI, _ in cases}
    assert len(found) == 9 and found == P.WST_CFG


def test_launchers_are_what_the_model_restates(source):
    """The lines of the two launchers the plans copy (a rewrite of either must revisit the model)."""
    for line in ("int per_kind = cus / kinds;", "if (per_kind < C::NB) per_kind = C::NB;", "slabs[b] = (nr * C::S + 31) / 32;",
                 "int n = per_kind * slabs[b] / tot;", "n = n < 1 ? 1 : n;", "if (n > nstack) n = (int)nstack;",
                 "const int64_t parts = (int64_t)used * C::KG;", "*ws_need = parts * 9 * CO * CI * (int64_t)sizeof(float);",
                 "for (int cur = 0; stack < nstack; stack += nwb, cur ^= 1) {", "int groups = (int)(batch < 1024 ? batch : 1024);"):
        assert line in source, line
    with open(KERNEL_HPP) as f:
        hpp = f.read()
    for line in ("const int64_t nitems = (B + G::IPI - 1) / G::IPI * G::NB;", "int grid = device_cus(dev) / G::NB * G::NB;",
                 "if (nitems < grid) grid = (int)nitems;", "for (; item < nitems; item += (int)gridDim.x, cur ^= 1) {",
                 "const int band = blockIdx.x % G::NB;", "const int ip = item / G::NB;"):
        assert line in hpp, line


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("plan_fn", [P.wgrad_px_plan, P.ws_bwd_plan, P.ws_fwd_plan], ids=["wgrad", "bwd", "fwd"])
def test_steady_batch_meets_its_conditions(plan_fn, cus):
    for side, cin, cout in P.SHAPES:
        B = P.steady_batch(plan_fn, side, cin, cout, cus)
        plan = plan_fn(side, cin, cout, B, cus)
        cond = plan.conditions()
        assert len(cond) == 4 and all(cond.values()), (side, cin, cout, B, cond)
        assert P.tensor_bytes(side, cin, cout, B) < CAP, (side, cin, cout, B)
        if B > 1:                                                    # the smallest: one image fewer fails a condition
            assert not all(plan_fn(side, cin, cout, B - 1, cus).conditions().values())
        # the conditions say what they mean: walk every workgroup's items
        if plan_fn is P.wgrad_px_plan:
            counts = [[len(range(wb, plan.nstack, n)) for wb in range(n)] for n in plan.nwg]
            assert [(max(c), min(c)) for c in counts] == [plan.items(b) for b in range(plan.NB)]
            assert all(sum(c) == plan.nstack for c in counts)
            assert plan.NI == 1 or plan.B == 2 * plan.nstack - 1
        else:
            counts = [[len(range(w, plan.nitems, plan.grid)) for w in range(plan.grid)]]
            assert (max(counts[0]), min(counts[0])) == plan.items() and sum(counts[0]) == plan.nitems
            assert plan.grid % plan.NB == 0 and plan.nitems % plan.NB == 0          # a workgroup keeps its band
        assert min(min(c) for c in counts) >= 2 and max(max(c) for c in counts) >= 3
        assert any(len(set(c)) == 2 for c in counts)                 # a ragged round: not every workgroup of a band gets the same number


def test_expected_batches_on_256_cus():
    """What the split gives on the MI355X's 256 CUs (documentation of the sizes the GPU tests run at; the tests compute their own)."""
    w = {s: P.steady_batch(P.wgrad_px_plan, *s, 256) for s in P.SHAPES}
    assert w[(12, 64, 64)] == w[(12, 32, 32)] == 341 and w[(26, 32, 32)] == 116 and w[(26, 64, 64)] == 58
    assert all(18 <= w[(34, ci, co)] <= 74 for ci, co in P.CHANNELS)
    d = {s: P.steady_batch(P.ws_bwd_plan, *s, 256) for s in P.SHAPES}
    assert d[(12, 32, 32)] == 1025 and d[(12, 64, 64)] == 513
    assert all(129 <= d[(26, ci, co)] <= 257 and 73 <= d[(34, ci, co)] <= 171 for ci, co in P.CHANNELS)


@pytest.mark.parametrize("cus", CUS)
def test_planted_cases_sit_where_they_claim(cus):
    for side, cin, cout in P.SHAPES:
        plan = P.wgrad_px_plan(side, cin, cout, P.steady_batch(P.wgrad_px_plan, side, cin, cout, cus), cus)
        cases = P.wgrad_one_hot_cases(plan)                          # (asserts image, band, workgroup and item of every case)
        assert {c.item for c in cases} >= {0, 1, 2} and len(cases) == (6 if side == 12 else 4)
        assert any(c.image // plan.NI == plan.nstack - 1 for c in cases)
        if side == 12:
            assert any(c.image == plan.B - 1 and c.y == 11 for c in cases) and any(c.image % 2 == 1 and c.y == 0 for c in cases)
        bwd = P.ws_bwd_plan(side, cin, cout, P.steady_batch(P.ws_bwd_plan, side, cin, cout, cus), cus)
        imgs = P.ws_planted_images(bwd)
        assert imgs["first"] != imgs["last"] and imgs["first"] not in imgs["sums"] and 2 <= len(imgs["sums"]) <= 2 * bwd.IPI


def test_workspace_query_is_the_plan_s():
    """tron_conv3x3_wgrad_px16_workspace answers without a device too (it then assumes 256 CUs): bytes = plan + 256."""
    so = os.path.join(PKG, "csrc", "libtron_hip.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.check_call(["bash", os.path.join(PKG, "csrc", "build.sh")])
    import torch
    L = ctypes.CDLL(so)                                              # the C ABI of include/tron_hip.h, nothing in between
    L.tron_conv3x3_wgrad_px16_workspace.restype = ctypes.c_int64
    L.tron_conv3x3_wgrad_px16_workspace.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    for side, cin, cout in P.SHAPES:
        for B in (1, 2, 3, 37, P.steady_batch(P.wgrad_px_plan, side, cin, cout, cus), 4096):
            assert int(L.tron_conv3x3_wgrad_px16_workspace(B, cin, cout, side)) == P.wgrad_px_plan(side, cin, cout, B, cus).bytes + 256
