"""kfac_gram_support, what the GPU tests of csrc/tron_kfac.hip's Gram kernels stand on, checked without a GPU: the Python copy
of the host plan against the library's two size queries (host arithmetic, read through ctypes), the split model and the
references against their definitions, the exactness condition on every input the GPU tests use, and that the multi-pass
cases still sit on the edges they were chosen for.  A retuned ksplit rule, pass size or tile fails here first."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import PKG
from kfac_gram_support import (CASES, CONV1_12, CONV1_34, CONV7_15, CONV7_17, EXACT_LIMIT, MAX_D, NCHW_B, NCHW_C, NCHW_GEOMETRY,
                               NCHW_SIDES, ODD_9x11, PATCH_BATCHES, PATCH_GEOMETRIES, SIDE_13, build_input, cases, exact_condition,
                               gram_plan, in_scale_of, k_ranges, linear_spill, linear_workspace, lo_input, lo_parts, operand,
                               out_size, passes, patch_workspace, pow2_scale_model, px_supported, ref_gram, ref_gram_three_term,
                               spill_batch, split_model, uneven_split_rows, which_patch_kernel)


@pytest.fixture(scope="module")
def L():
    so = os.path.join(PKG, "csrc", "libtron_hip.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.check_call(["bash", os.path.join(PKG, "csrc", "build.sh")])
    lib = ctypes.CDLL(so)                                               # the C ABI of include/tron_hip.h, nothing in between
    lib.tron_kfac_gram_workspace.restype = ctypes.c_int64
    lib.tron_kfac_gram_workspace.argtypes = [ctypes.c_int64, ctypes.c_int32]
    lib.tron_kfac_patch_gram_workspace.restype = ctypes.c_int64
    lib.tron_kfac_patch_gram_workspace.argtypes = [ctypes.c_int64] + [ctypes.c_int32] * 7
    return lib


# ---- the plan --------------------------------------------------------------------------------------------------------------
def test_linear_workspace_is_the_plan(L):
    """d on both sides of every multiple of 64 (and with it of 128) up to 8192, rows from 1 to past one pass."""
    widths = sorted({1, 2, 3} | {64 * m + e for m in range(1, 129) for e in (-1, 0, 1) if 64 * m + e <= MAX_D})
    for d in widths:
        chunk = gram_plan(1 << 40, 64, d)["rows_chunk"]
        for rows in (1, 63, 64, 65, 1000, 1023, 1024, 1025, 3071, 3072, 100000, chunk - 1, chunk, chunk + 1, 3 * chunk + 5):
            assert linear_workspace(rows, d) == L.tron_kfac_gram_workspace(rows, d), (rows, d, gram_plan(rows, 64, d))
    for rows, d in ((100, MAX_D + 1), (100, 9000), (0, 64), (-1, 64), (100, 0)):
        assert L.tron_kfac_gram_workspace(rows, d) == 0 == linear_workspace(rows, d)


def test_plan_values_by_hand():
    """The constants a retune would move, pinned: 512 MB per pass, 768 / upper-triangle tiles of 128, at least 16 K chunks
    of 64 per split, at most 256 splits."""
    p = gram_plan(1 << 40, 64, 1)
    assert (p["dpad"], p["rows_chunk"], p["ksplit"]) == (64, (512 << 20) // 256, 256)
    assert gram_plan(3008, 64, 64)["ksplit"] == 2 and gram_plan(3009, 64, 64)["ksplit"] == 3       # rows_chunk / 64 = 47 | 48 -> / 16
    assert gram_plan(1 << 40, 81, 3136)["ksplit"] == 768 // (25 * 26 // 2) == 2
    assert gram_plan(1 << 40, 64, 129)["ksplit"] == 256 and gram_plan(1 << 40, 64, 257)["ksplit"] == 768 // 6
    assert gram_plan(1 << 40, 64, 2048)["ksplit"] == 768 // 136 == 5
    p = gram_plan(1, 64, 1)
    assert (p["rows_chunk"], p["ksplit"], p["total"]) == (64, 1, 2 * 64 * 64 * 2 + 64 * 4 + 512)


def test_patch_workspace_is_the_plan(L):
    for (C, H, W), geo in PATCH_GEOMETRIES:
        assert not px_supported(7, C, H, W, *geo)
        spill = spill_batch(C, H, W, *geo)
        for B in PATCH_BATCHES + (spill - 1, spill, spill + 1, 16384):
            assert patch_workspace(B, C, H, W, *geo) == L.tron_kfac_patch_gram_workspace(B, C, H, W, *geo), (B, C, H, W, geo)
    for C in NCHW_C:
        for H, W in NCHW_SIDES.values():
            for B in NCHW_B + (160, 16384):
                want = patch_workspace(B, C, H, W, *NCHW_GEOMETRY)
                assert want == L.tron_kfac_patch_gram_workspace(B, C, H, W, *NCHW_GEOMETRY), (B, C, H, W)
                assert want >= min(B, 2048) * C * C * 4
    assert patch_workspace(160, 64, 4, 4, *NCHW_GEOMETRY) == 160 * 64 * 64 * 4 + 512 > gram_plan(160 * 16, 16, 64)["total"]
    for C in (32, 64):                                                   # the PX kernel may ask for more, never for less
        for S in (12, 26, 34):
            for B in (1, 7, 500):
                assert px_supported(B, C, S, S, 3, 3, 1, 1)
                assert L.tron_kfac_patch_gram_workspace(B, C, S, S, 3, 3, 1, 1) >= patch_workspace(B, C, S, S, 3, 3, 1, 1) > 0
    for args in ((0, 3, 12, 12, 3, 3, 1, 1), (4, 3, 12, 12, 3, 3, 1, 0), (4, 1024, 12, 12, 3, 3, 1, 1), (4, 3, 2, 12, 3, 3, 0, 1),
                 (4, 0, 12, 12, 3, 3, 1, 1), (4, 3, 12, 12, 3, 3, -1, 1)):
        assert L.tron_kfac_patch_gram_workspace(*args) == 0 == patch_workspace(*args), args


def test_geometries_run_the_kernels_they_were_chosen_for():
    want = {CONV1_12: "k_patches_t_plane", CONV1_34: "k_patches_t_plane", CONV7_17: "k_patches_t", CONV7_15: "k_patches_t_plane",
            ODD_9x11: "k_patches_t", SIDE_13: "k_patches_t"}
    for (chw, geo), kernel in want.items():
        assert which_patch_kernel(*chw, *geo) == kernel, (chw, geo)
    assert [out_size(H, W, *geo) for (C, H, W), geo in (CONV7_17, CONV7_15, ODD_9x11)] == [(9, 9), (8, 8), (7, 9)]
    for c in CASES:
        if c.kind == "patch":
            assert c.in_scale is not None or not px_supported(*c.shape, *c.geometry), c.name
            assert patch_workspace(*c.shape, *c.geometry) > 0, c.name


def test_multipass_cases_sit_on_their_edges():
    """What each multi-pass case is there for, from passes() and k_ranges().  If the plan changes, the batches move with it
    (they are spill_batch() / linear_spill()), but the edges below may not: the message names what the last pass looks like now;
    pick tails (images or rows behind the first pass) that restore an empty split, a range of one chunk, and ranges of 2 and 3."""
    seen = {}
    for c in cases("multipass"):
        if c.kind == "patch":
            B, (C, H, W) = c.shape[0], c.shape[1:]
            oh, ow = out_size(H, W, *c.geometry[0:4])
            per, d = oh * ow, C * c.geometry[0] * c.geometry[1]
            ps, ks = passes(B, per, d), gram_plan(B * per, per, d)["ksplit"]
            assert B == spill_batch(C, H, W, *c.geometry) and ps[-1][0] == 1, (c.name, ps)
        else:
            rows, d = c.shape
            ps, ks = passes(rows, 1, d, rows_unit=64), gram_plan(rows, 64, d)["ksplit"]
        lengths = sorted({hi - lo for lo, hi in k_ranges(ps[-1][1], ks)})
        seen[c.name] = (len(ps), ps[-1][1] // 32, ks, lengths)
        assert len(ps) >= 2, (c.name, ps)
        assert 4 * c.shape[0] * (per if c.kind == "patch" else 1) < EXACT_LIMIT, c.name
    assert seen == {"64x17x17": (2, 4, 2, [2]),                          # k_patches_t: 528 + 1 images, the last pass 81 rows in 128
                    "64x15x15": (2, 2, 2, [1]),                          # plane kernel: 668 + 1 images, ranges of ONE chunk
                    "3x12x12": (2, 6, 256, [0, 1]),                      # plane kernel behind 256 splits: nk < ksplit, 250 empty splits
                    "5x9x11": (2, 2, 256, [0, 1]),                       # k_patches_t behind 256 splits
                    "linear-tail1": (2, 2, 256, [0, 1]),                 # one row behind a full pass
                    "linear-d3-tail20000": (2, 626, 256, [2, 3])}, seen
    assert spill_batch(*CONV7_17[0], *CONV7_17[1]) == 529 and spill_batch(*CONV7_15[0], *CONV7_15[1]) == 669
    assert linear_spill(1) == ((512 << 20) // 256 + 1, 1)
    rows = uneven_split_rows(64)
    p = gram_plan(rows, 64, 64)
    assert p["ksplit"] >= 3 and len(passes(rows, 1, 64, rows_unit=64)) == 1
    assert len({hi - lo for lo, hi in k_ranges(passes(rows, 1, 64, rows_unit=64)[0][1], p["ksplit"])}) == 2      # uneven ranges


# ---- the split and the references ------------------------------------------------------------------------------------------
def test_split_model_is_the_definition():
    """hi = the nearest f16 (ties to even), lo = the nearest f16 of (v - hi) 2^11: against numpy's conversions on a sweep with
    f16 subnormals, values at and next to rounding ties, and against values written down by hand."""
    ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 - 2.0 ** -12, 2 + 2.0 ** -10, 3 * 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -25, 1023.5 * 2.0 ** -24]
    near = [float(np.nextafter(np.float32(t), np.float32(s))) for t in ties for s in (0.0, 4.0)]
    sub = [k * 2.0 ** -24 for k in (1, 2, 3, 1023, 1024, 1025)] + [2.0 ** -26, 2.0 ** -30]
    g = torch.Generator().manual_seed(0)
    rand = (torch.randn(4096, generator=g) * torch.tensor(2.0) ** torch.randint(-20, 12, (4096,), generator=g)).tolist()
    v = torch.tensor(ties + near + sub + rand + [0.0, -0.0, 1.0, -3.0], dtype=torch.float32)
    v = torch.cat([v, -v])
    hi, lo = split_model(v)
    n = v.numpy()
    nh = n.astype(np.float16)
    nl = ((n - nh.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    assert np.array_equal(hi.numpy(), nh) and np.array_equal(lo.numpy(), nl)
    assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all()
    back = hi.double() + lo.double() * 2.0 ** -11
    assert ((back - v.double()).abs() <= v.double().abs() * 2.0 ** -22 + 2.0 ** -36).all()
    by_hand = {1 + 2.0 ** -11: (1.0, 1.0),                               # midway between 1 and 1 + 2^-10: to the even 1
               1 + 3 * 2.0 ** -11: (1 + 2.0 ** -9, -1.0),                # midway between 1 + 2^-10 (odd) and 1 + 2^-9
               1 - 2.0 ** -12: (1.0, -0.5),                              # midway between 1 - 2^-11 (odd) and 1
               3 * 2.0 ** -25: (2.0 ** -23, -2.0 ** -14),                # midway between the subnormals 1 and 2 (x 2^-24)
               2.0 ** -25: (0.0, 2.0 ** -14),                            # half the smallest subnormal: to zero, lo keeps it
               2.0 ** -30: (0.0, 2.0 ** -19)}
    for val, (h, l) in by_hand.items():
        gh, gl = split_model(torch.tensor([val, -val], dtype=torch.float32))
        assert gh.tolist() == [h, -h] and gl.tolist() == [l, -l], val


def test_lo_family_splits_into_h_and_half_m():
    x = lo_input((500, 40), seed=1)
    h, m = lo_parts(x)
    assert sorted(h.unique().tolist()) == [-2, -1, 0, 1, 2] and sorted(m.unique().tolist()) == [-1, 0, 1]
    assert ((h == 0) == (m == 0)).all() and 0.4 < (h != 0).float().mean() < 0.6
    hi, lo = operand(x)
    assert torch.equal(hi.float(), h) and torch.equal(lo.float(), m / 2)
    for both in ((1, 1), (1, -1), (-1, 1), (-1, -1), (2, -1), (-2, 1)):   # every sign pairing, the ties 1 - 2^-12 among them
        hi, lo = operand(torch.tensor([64.0 * both[0] + both[1] * 2.0 ** -6]))
        assert (hi.item(), lo.item()) == (both[0], both[1] / 2)


def loop_gram(rows):
    d = len(rows[0])
    return [[sum(r[i] * r[j] for r in rows) for j in range(d)] for i in range(d)]


def test_ref_gram_is_the_definition():
    """Against a Gram written as three Python loops, on the rows spelt out by hand for each kind of input."""
    from kfac_gram_support import ints
    a = ints((9, 5), False, 1)
    assert ref_gram(a, 0.5).tolist() == (torch.tensor(loop_gram(a.tolist()), dtype=torch.float64) * 0.5).tolist()
    g = ints((3, 4, 2, 2), False, 2)                                     # NCHW: a row per (image, position), a column per channel
    rows = [[g[b, c, y, x].item() for c in range(4)] for b in range(3) for y in range(2) for x in range(2)]
    want = torch.tensor(loop_gram(rows), dtype=torch.float64)
    assert torch.equal(ref_gram(g, 1.0, NCHW_GEOMETRY), want)
    gd = g.double().permute(1, 0, 2, 3).reshape(4, -1)
    assert torch.equal(gd @ gd.t(), want)
    for (B, C, H, W), (kh, kw, pad, stride) in (((2, 2, 4, 5), (3, 3, 1, 1)), ((2, 1, 7, 7), (3, 2, 1, 2)), ((1, 2, 4, 4), (2, 2, 0, 1))):
        x = ints((B, C, H, W), False, H)
        oh, ow = out_size(H, W, kh, kw, pad, stride)
        get = lambda b, c, y, xx: x[b, c, y, xx].item() if 0 <= y < H and 0 <= xx < W else 0.0
        rows = [[get(b, c, oy * stride - pad + ky, ox * stride - pad + kx) for c in range(C) for ky in range(kh) for kx in range(kw)]
                for b in range(B) for oy in range(oh) for ox in range(ow)]
        want = torch.tensor(loop_gram(rows), dtype=torch.float64)
        assert want.abs().max() > 0 and torch.equal(ref_gram(x, 1.0, (kh, kw, pad, stride)), want)
        assert torch.equal(ref_gram(x, 2.0 ** -10, (kh, kw, pad, stride)), want * 2.0 ** -10)


def test_three_term_reference():
    """== ref_gram wherever every lo is zero (integers, with and without in_scale); on the lo family it is the hand-written
    sum of h h' + (h m' + m h') 2^-12 — the true product without its m m' 2^-24 — and differs from the hi-only product."""
    from kfac_gram_support import ints
    for k, in_scale in ((0, None), (17, 2.0 ** 17), (-20, 2.0 ** -20), (17, 2.0 ** 25)):
        x = ints((50, 7), False, 3) * 2.0 ** -k
        assert not operand(x, in_scale)[1].any()
        assert torch.equal(ref_gram_three_term(x, 0.25, in_scale), ref_gram(x, 0.25))
    g = ints((2, 3, 4, 4), True, 4)
    assert torch.equal(ref_gram_three_term(g, 1.0, None, (3, 3, 1, 1)), ref_gram(g, 1.0, (3, 3, 1, 1)))
    x = lo_input((60, 6), seed=2)
    h, m = (t.double() for t in lo_parts(x))
    want = 4096.0 * (h.t() @ h + (h.t() @ m + m.t() @ h) * 2.0 ** -12)
    assert torch.equal(ref_gram_three_term(x, 1.0), want)
    assert torch.equal(ref_gram_three_term(x, 1.0, terms=1), 4096.0 * (h.t() @ h))
    assert not torch.equal(want, ref_gram_three_term(x, 1.0, terms=1))
    assert torch.equal(ref_gram(x, 1.0), want + (m.t() @ m) * 2.0 ** -12)


def test_exact_condition_counts_what_it_says():
    """Ones: the numerator is the row count.  Twos: still the row count (the unit grows with the data's smallest bit).  The lo
    family: sum |h h'| in units of 2^-12, plus the mixed terms.  pow2_scale_model puts the maximum in [2^15, 2^16)."""
    assert exact_condition(torch.ones(1000, 3)) == 1000 and exact_condition(torch.full((1000, 3), 2.0)) == 1000
    assert exact_condition(torch.tensor([[1.0, 2.0]] * 10)) == 40 and exact_condition(torch.zeros(4, 4)) == 0
    assert exact_condition(torch.ones(2, 1, 3, 3), None, (3, 3, 1, 1)) == 18          # the centre tap sees every pixel
    x = torch.tensor([[64.0 + 2.0 ** -6, 128.0 - 2.0 ** -6]] * 3)                     # h = (1, 2), m = (1, -1)
    assert exact_condition(x) == 3 * (4 * 4096 + 2 * 2)                               # the (1, 1) entry: 4 + 2 * 2 * 0.5 * 2^-11
    assert exact_condition(torch.ones(1 << 22, 1) * 2.0) < EXACT_LIMIT <= exact_condition(torch.ones(1 << 24, 1))
    assert pow2_scale_model(torch.tensor([0.0, -2.0 * 2.0 ** -17])) == 2.0 ** 31 and pow2_scale_model(torch.zeros(3)) == 1.0
    from Net import kfac
    for v in (3.0, 2.0 ** -17, 1e-9, 70000.0):
        t = torch.tensor([v, -v / 3])
        assert kfac._pow2_scale(t).item() == pow2_scale_model(t)


@pytest.mark.parametrize("group", sorted({c.group for c in CASES}))
def test_every_gpu_input_meets_the_exact_condition(group):
    """The inputs of tests/test_gpu_kfac_gram.py, built here from the same table and seeds: the reference alone decides that
    they are exact — use smaller or sparser data if this fails."""
    for c in cases(group):
        x = build_input(c)
        top = exact_condition(x, in_scale_of(c, x), c.geometry)
        assert 0 < top < EXACT_LIMIT, f"{c.group}/{c.name}: numerator {top}: use smaller or sparser data"
        if x.numel() <= 1 << 22:
            assert bool(operand(x, in_scale_of(c, x))[1].any()) == (c.family == "lo"), c.name
