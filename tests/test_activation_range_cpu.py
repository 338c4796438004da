"""The activation-range tests' own tools (tests/activation_range_support.py), checked without a GPU: the placement of the sweep,
the host PX16 pack / unpack, the float64 references, and that the fast formula of the fused epilogues — emulated in float32 with a
correctly rounded exp2 and reciprocal — stays inside the bounds tests/test_gpu_activation_range.py holds the kernels to."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

from activation_range_support import (band_rows, check_placement, dmish64, fast_formula, fill, mish64, out_floor, pack_px,
                                       placement, special_points, sweep, unpack_px)


def test_sweep_holds_the_grid_and_every_special_point():
    sw = sweep()
    assert sw.dtype == torch.float32 and sw.numel() == 4001 + special_points().numel()
    assert sw.min().item() == -1e6 and sw.max().item() == 1e6 and torch.isfinite(sw).all()
    vals = set(sw.tolist())
    for v in (-110.0, 110.0, 20.0, 41.4465, 44.3614, -87.3365, -87.4, -103.9, 88.8, 1e3, -3e4, 1e-9, -1e-6):
        assert float(np.float32(v)) in vals, v
    bits = sw.view(torch.int32)
    assert (bits == 0).any() and (bits == -2 ** 31).any()                    # +0 and -0
    twenty = np.float32(20.0)
    assert float(np.nextafter(twenty, np.float32(0))) in vals and float(np.nextafter(twenty, np.float32(100))) in vals
    zero = sorted(v for v in vals if abs(v + 1.1924) < 1e-5)
    assert len(zero) == 5 and zero[0] < np.float32(-1.1924) < zero[-1]


@pytest.mark.parametrize("S", [12, 26, 34])
@pytest.mark.parametrize("B,C", [(3, 32), (3, 64), (2, 32)])
def test_fill_places_every_special_point_three_times(S, B, C):
    t = fill(B, C, S, seed=S + C)
    assert t.shape == (B, C, S, S) and t.dtype == torch.float32
    check_placement(t, B, C, S, S + C)
    corner, row_end, band = placement(B, C, S, S + C)
    assert len({tuple(r) for r in np.concatenate([corner, row_end, band]).tolist()}) == 3 * len(corner)
    assert set(band[:, 2].tolist()) <= set(band_rows(S))
    assert band_rows(26) == (12, 13) and band_rows(34) == (8, 9, 16, 17, 24, 25)
    if t.numel() >= 4 * sweep().numel():                                   # every grid point is there as well
        assert torch.isin(torch.linspace(-110.0, 110.0, 4001, dtype=torch.float64).float(), t).all()
    assert torch.equal(t, fill(B, C, S, seed=S + C))


def test_px16_round_trip_over_the_sweep():
    sw = sweep()
    side = 2
    while side * side * 8 < sw.numel():
        side += 1
    x = torch.zeros(1, 8, side, side)
    x.view(-1)[:sw.numel()] = sw
    back = unpack_px(pack_px(x), 1, 8, side)
    err = (back - x.double()).abs()
    bound = 2.0 ** -21 * x.double().abs() + 2 * (64 * 2.0 ** -24 / 2048)
    assert (err <= bound).all(), (err - bound).max().item()
    assert torch.equal(out_floor(x), err)
    # a PX16 value packs to itself: the floor of an exactly representable reference is 0
    assert torch.equal(unpack_px(pack_px(back), 1, 8, side), back)
    # the layout: channel c of pixel p sits at [hi | lo][c / 8][p][c % 8]
    y = torch.arange(2 * 16 * 4, dtype=torch.float32).reshape(2, 16, 2, 2)
    img = pack_px(y).view(torch.float16).reshape(2, 2, 2, 4, 8)
    assert img[1, 0, 1, 3, 5].item() * 64 == y[1, 13, 1, 1].item() and (img[:, 1] == 0).all()


def test_float64_references_agree_with_torch():
    x = sweep().double()
    xr = x.clone().requires_grad_(True)
    want = F.mish(xr)
    want.sum().backward()
    assert (mish64(x) - want.detach()).abs().max().item() <= 1e-12 * 1e6
    assert ((mish64(x) - want.detach()).abs() <= 1e-14 * want.detach().abs() + 1e-300).all()
    assert ((dmish64(x) - xr.grad).abs() <= 1e-13).all()
    assert dmish64(torch.tensor([0.0])).item() == pytest.approx(0.6, abs=1e-15)
    assert abs(dmish64(torch.tensor([-1.1924])).item()) < 1e-4


def test_fast_formula_alone_stays_inside_the_bounds():
    """The sweep is one the formula passes with exact transcendentals: what a kernel adds is its hardware exp2 / rcp and its bugs."""
    sw = sweep()
    y, m = fast_formula(sw.numpy())
    assert np.isfinite(y).all() and np.isfinite(m).all()
    ref, dref = mish64(sw).numpy(), dmish64(sw).numpy()
    fwd = np.abs(y.astype(np.float64) - ref) / (1e-6 * np.abs(ref) + 2e-9)
    der = np.abs(m.astype(np.float64) - dref) / (np.abs(dref) + 0.1)
    print(f"forward: {fwd.max():.3f} of its bound at x = {sw[fwd.argmax()].item()!r}; "
          f"derivative: {der.max():.3g} against 2e-6 at x = {sw[der.argmax()].item()!r}")
    assert fwd.max() <= 1.0
    assert der.max() <= 2e-6
