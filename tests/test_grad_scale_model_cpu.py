"""The host model of the gradient scales (tests/grad_scale_support.py) against what csrc/tron_f16x3.hpp and k_absmax_pow2
document: over every f32 exponent, both mantissa ends and the denormals the scaled maximum lies in the half-open interval, and
outside the scaled range the model answers the fallback.  tests/test_gpu_grad_scale.py holds the kernels to this model."""
import numpy as np
import pytest

import grad_scale_support as G

F32 = np.float32


def test_sweep_covers_every_exponent_and_both_mantissa_ends():
    vals = G.sweep()
    assert all(v.dtype == F32 and np.isfinite(v) and v > 0 for v in vals)
    exps = {int(np.frexp(np.float64(v))[1]) for v in vals}
    assert exps == set(range(-148, 129))                               # 2^-149 = 0.5 2^-148 ... the largest float = f 2^128
    fields = {(int(v.view(np.uint32)) >> 23) & 255 for v in vals}
    assert fields == set(range(0, 255))                                # every exponent field but inf / NaN's
    for k in range(-125, 128):
        p = F32(np.ldexp(1.0, k))
        assert any(v == p for v in vals) and any(v == np.nextafter(p, F32(0), dtype=F32) for v in vals)
    assert len(set(float(v) for v in vals)) == len(vals)


@pytest.mark.parametrize("fallback", [1.0, 1.0 / 64.0])
def test_absmax_scale_puts_the_maximum_in_its_interval_or_falls_back(fallback):
    """m s in [2^13, 2^14) for every finite m = f 2^e with e >= -100, the largest float included; the fallback for everything
    else: smaller maxima, zero, negatives, inf, NaN.  The products are exact (s is a power of two, the result a normal float)
    and so is the scale's inverse, which k_conv3x3_f16 needs."""
    scaled = 0
    for m in G.sweep():
        s = G.absmax_scale(m, fallback)
        assert s.dtype == F32 and s == G.absmax_scale_bits(m, fallback), m
        _, e = np.frexp(np.float64(m))
        if G.SCALE_E_MIN <= e <= G.SCALE_E_MAX:
            prod = np.float64(m) * np.float64(s)
            assert 2.0 ** 13 <= prod < 2.0 ** 14, (m, s)
            assert F32(prod) == prod and s == F32(np.ldexp(1.0, 14 - int(e)))
            inv = F32(1.0) / s
            assert np.isfinite(inv) and inv >= np.finfo(F32).tiny and np.float64(inv) * np.float64(s) == 1.0
            scaled += 1
        else:
            assert e < G.SCALE_E_MIN and s == F32(fallback), (m, s)
    assert scaled == 2 * 229                                           # e = -100 .. 128, two mantissa ends each
    for m in (0.0, -0.0, -1.0, -np.inf, np.inf, np.nan):
        assert G.absmax_scale(F32(m), fallback) == F32(fallback)
    # the edges by name: no finite maximum is too large (2^100 unscaled would be inf in f16); 2^-101 = 0.5 2^-100 is the smallest
    assert G.absmax_scale(F32(2.0 ** 99), 7.0) == F32(2.0 ** -86) and G.absmax_scale(F32(2.0 ** 100), 7.0) == F32(2.0 ** -87)
    assert G.absmax_scale(np.nextafter(F32(2.0 ** 100), F32(0)), 7.0) == F32(2.0 ** -86)
    assert G.absmax_scale(np.finfo(F32).max, 7.0) == F32(2.0 ** -114) == G.absmax_scale(F32(2.0 ** 127), 7.0)
    assert G.absmax_scale(F32(2.0 ** -101), 7.0) == F32(2.0 ** 114) and G.absmax_scale(F32(2.0 ** -99), 7.0) == F32(2.0 ** 112)
    assert G.absmax_scale(np.nextafter(F32(2.0 ** -101), F32(0)), 7.0) == 7.0 and G.absmax_scale(F32(2.0 ** -102), 7.0) == 7.0


@pytest.mark.parametrize("target", [-60, -1, 0, 14, 15, 16, 60])
def test_absmax_pow2_puts_the_maximum_below_its_target_or_clamps(target):
    """m s in [2^(t - 1), 2^t) wherever |t - e| <= 60; beyond, the scale is 2^60 or 2^-60; 1 for an all-zero tensor."""
    inside = 0
    for m in G.sweep():
        s = G.absmax_pow2(m, target)
        assert s.dtype == F32 and s == G.absmax_pow2_bits(m, target), (m, target)
        _, e = np.frexp(np.float64(m))
        k = target - int(e)
        if -G.POW2_CLAMP <= k <= G.POW2_CLAMP:
            prod = np.float64(m) * np.float64(s)
            assert 2.0 ** (target - 1) <= prod < 2.0 ** target, (m, s)
            inside += 1
        else:
            assert s == F32(2.0 ** (G.POW2_CLAMP if k > 0 else -G.POW2_CLAMP)), (m, s)
        assert np.isfinite(np.float32(s) * np.float32(s))              # what the clamp is for
    assert inside == sum(1 for m in G.sweep() if abs(target - int(np.frexp(np.float64(m))[1])) <= G.POW2_CLAMP) > 200
    assert G.absmax_pow2(F32(0.0), target) == 1.0 and G.absmax_pow2(F32(-0.0), target) == 1.0
    for m in G.denormal_sweep():
        assert G.absmax_pow2(m, target) == F32(2.0 ** 60)              # denormals: always the upper clamp


def test_planted_tensors_and_positions():
    for n in (1, 2, 3, 5, 7, 1023, 1024, 1025, 4099):
        pos = G.pow2_positions(n)
        assert 0 in pos and n - 1 in pos and all(0 <= p < n for p in pos)
        for v in (F32(1.0), F32(-2.0 ** -140), F32(2.0 ** 127), F32(2.0 ** -149)):
            x = G.planted(n, pos[-1], v, 3)
            assert x.dtype == F32 and np.abs(x).max() == abs(v) and int(np.abs(x).argmax()) == pos[-1] or n == 1
    n = 1_000_003
    grid = G.pow2_grid(n)
    assert grid == 62 and 4 * grid * 1024 + 5 < n                      # a second grid-stride trip exists
    assert {4 * grid * 1024 - 1, 4 * grid * 1024, 4 * grid * 1024 + 5} <= set(G.pow2_positions(n, grid * 1024))
    assert G.pow2_grid(1) == 1 and G.pow2_grid(4 * 4096 * 256 * 3) == 256
    names = dict(G.spike_positions(37, 64, 12))
    assert names["last"] == (36, 63, 11, 11) and names["ragged group"][0] == 36 and names["octet end"][1] == 7
    for N in (1, 3, 63, 64, 65, 130):
        owned = [G.segment_bounds(N, s) for s in range(G.BIAS_SEGS)]
        assert owned[0][0] == 0 and owned[-1][1] == N and all(a[1] == b[0] for a, b in zip(owned, owned[1:]))
    assert G.absmax_indices(1) == [0] and G.absmax_indices(4096) == [0, 255, 256, 511, 512, 4095]
