"""Every fused mish / mish' epilogue swept over the activation's whole range (tests/activation_range_support.py::sweep: -110 .. 110
on a grid, the cut-over at 20, the derivative's zero, the cap ln 1e18, e * e's overflow, exp2's flush boundary, +-1e-9 .. +-1e6).

Degenerate weights turn each fused kernel into an elementwise probe of its own activation code: the pre-activation of every output
element is a planted, exactly known value — (1) one-tap identity weights W[co][co % cin][1][1] = 1, (2) zero weights and a planted
residual / `extra`, (3) zero weights and a planted bias, (4) for the derivative kernels a planted z and a gradient plane of signed
powers of two.  The inputs are read back from the very bytes handed to the kernel (unpack of the PX16 image), so input quantisation
is not in the error; the reference is float64 x tanh(softplus x) and its autograd derivative at those values.

Which test reaches which copy of the formula:

  copy                                                        reached by
  tron_conv.hip:75            mish1 (Newton step, x > 20 select)   test_conv3x3_f32_in[f32-*], test_conv3x3_from_codes[f32-*]
  tron_conv_f16.hip:103       mish4 (cap, one rcp)                 test_conv3x3_f32_in[f16x3-*], test_conv3x3_from_codes[f16x3-*]
  tron_conv_f16.hip:120       mish_grad4                           test_conv3x3_dgrad_mish
  tron_conv_f16.hip:88        mish1: no kernel calls it            -
  tron_conv_ws_kernel.hpp:78  mish4 (conv1 from codes, :801)       test_conv1_px16
  tron_conv_ws_kernel.hpp:389 staged copy, forward (:405)          test_conv_ws, test_conv_ws_train, test_conv_ws_pool12
  tron_conv_ws_kernel.hpp:389 staged copy, mish' (:398-403)        test_conv_ws_dgrad
  tron_conv_ws_train.hip:146  inline mish' of k_gout_px            test_grad_px_from_f32, test_grad_px_from_pooled
  tron_head.hip:40            mish1 (k_mish_cl_to_nchw, :1019)     test_pool_conv7
  tron_head.hip:1030          mish_grad1 (k_mish_bwd_to_cl, :1062) test_pool_conv7

Bounds (none comes from a run of a kernel under test):
  forward     |got - mish64(x)| <= 1e-6 |ref| + 2e-9 + out_floor(ref)
  derivative  |got - g dmish64(z)| <= 2e-6 |g| (|dmish64(z)| + 0.1) + out_floor
  z           the returned pre-activation equals the planted value to out_floor
  bias sums   1e-5 max |sum| + 1e-6 scale;  channel maxima 2e-6 scale
No copy needed a wider relative term.  Measured on an MI355X against float64, as the largest fraction of the bound over the sweep:
forward 0.38 (every copy; the formula alone with exact exp2 / rcp gives 0.35, tests/test_activation_range_cpu.py), derivative 0.20.
tron_conv7_fwd / _bwd apply no activation (Net/activations.py::_Conv7HIP) and are not probed here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from activation_range_support import (dmish64, fill, mish64, out_floor, pack_px, px_value, sweep, to_px, unpack_px)

PAIRS = [(32, 32), (32, 64), (64, 64)]
B3 = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fused():
    from Net import fused
    return fused


@pytest.fixture(scope="module")
def nat(fused):
    fused.nat.lib()
    return fused.nat                                                     # (the C ABI's loader, as Net/fused.py holds it)


def _one_tap(cin, cout):
    w = torch.zeros(cout, cin, 3, 3, device="cuda")
    w[torch.arange(cout), torch.arange(cout) % cin, 1, 1] = 1.0
    return w


@pytest.fixture(scope="module")
def weights(fused):
    """Per channel pair: the one-tap and the all-zero weights, their weight-stationary fragment images and the rotated ones of the
    input gradient — built once."""
    out = {}
    for cin, cout in PAIRS:
        tap, zero = _one_tap(cin, cout), torch.zeros(cout, cin, 3, 3, device="cuda")
        frag = fused._split_jobs([tap, zero], "tron_conv3x3_ws_split_weights", False)
        rot, wn = fused._split_jobs([tap, zero], "tron_conv3x3_ws_split_weights_bwd", True)
        out[cin, cout] = dict(tap=tap, zero=zero, frag_tap=frag[0], frag_zero=frag[1], rot_tap=rot[0], rot_zero=rot[1], wn=wn)
    return out


_FILLS = {}


def _fill(B, C, S, seed=0):
    """fill() on the device, computed once per shape and never written to."""
    key = (B, C, S, seed)
    if key not in _FILLS:
        _FILLS[key] = fill(B, C, S, 1000 * S + C + seed).cuda()
    return _FILLS[key]


def _worst(name, err, bound, x):
    ratio = torch.where(err > 0, err / bound, torch.zeros_like(err)).flatten()          # (0 of a 0 bound is inside it)
    i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
    return f"{name}: worst {ratio[i].item():.3g} of the bound at x = {x.flatten()[i].item()!r} (error {err.flatten()[i].item():.3g})"


def check_forward(name, got, x, floor=None):
    """got = mish(x) for every element: finite, and inside the forward bound."""
    got, x = got.double(), x.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite output at x = {x[~torch.isfinite(got)][:8].tolist()}"
    ref = mish64(x)
    bound = 1e-6 * ref.abs() + 2e-9 + (out_floor(ref) if floor else 0.0)
    err = (got - ref).abs()
    msg = _worst(name, err, bound, x)
    print(msg)
    assert (err <= bound).all(), msg


def check_pre(name, z, x, floor=None):
    """The returned pre-activation is the planted value."""
    z, x = z.double(), x.double()
    assert torch.isfinite(z).all(), name
    bound = out_floor(x) if floor else torch.zeros_like(x)
    err = (z - x).abs()
    assert (err <= bound).all(), f"{name}: pre-activation off by {err.max().item():.3g} at x = {x.flatten()[int(err.argmax())].item()!r}"


def check_derivative(name, got, g, z, floor=None):
    """got = g mish'(z) for every element."""
    got, g, z = got.double(), g.double(), z.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite output at z = {z[~torch.isfinite(got)][:8].tolist()}"
    d = dmish64(z)
    bound = 2e-6 * g.abs() * (d.abs() + 0.1) + (floor if floor is not None else 0.0)
    err = (got - g * d).abs()
    msg = _worst(name, err, bound, z)
    print(msg)
    assert (err <= bound).all(), msg
    return g * d


def check_sums(name, gb, ref, info=None):
    """The bias gradient (column sums of ref) and, with `info`, the gradient image's record of channel maxima."""
    scale = ref.abs().max().item()
    sums = ref.sum((0, 2, 3))
    err = (gb.double() - sums).abs().max().item()
    print(f"{name}: bias sums off by {err:.3g}, bound {1e-5 * sums.abs().max().item() + 1e-6 * scale:.3g}")
    assert torch.isfinite(gb).all() and err <= 1e-5 * sums.abs().max().item() + 1e-6 * scale, name
    if info is not None:
        top = info[4:4 + ref.shape[1]].max().item()
        assert abs(top - scale) <= 2e-6 * scale, (name, top, scale)


def _signed_pow2(shape, seed, lo=-2, hi=2):
    """A gradient plane of signed powers of two 2^lo .. 2^hi: exact in every format on the way."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(lo, hi + 1, shape, generator=g).double()
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (s * 2.0 ** e).float().cuda()


def _grad_px(fused, g):
    """A gradient image of g at the scale tron_absmax_pow2(14) would give."""
    B, C, S, _ = g.shape
    m = g.abs().max().item()
    s = 2.0 ** (13 - int(np.floor(np.log2(m))))
    px = to_px(fused, g, s)
    out = fused.GradPX(B, C, S, g.device)
    out.buf = px.buf
    out.info = torch.zeros(68, dtype=torch.float32, device=g.device)
    out.info[0], out.info[1] = s, 1.0 / s
    out.info[4:4 + C] = g.abs().amax((0, 2, 3))
    return out, px_value(px) / s


def _module(w, bias=None):
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.zero_() if bias is None else conv.bias.copy_(bias)
    return conv


def _spread(x, cout):
    """What the one-tap weights make of x [B, cin, S, S]: output channel co carries input channel co % cin."""
    return x[:, torch.arange(cout, device=x.device) % x.shape[1]]


# ---- the f32-in kernels: tron_conv3x3_fwd in both arithmetics -------------------------------------------------------------------

MATH_SIDES = [("f32", 12), ("f32", 26), ("f16x3", 12), ("f16x3", 26), ("f16x3", 34)]      # (the f32 arithmetic has no 34x34 kernel)


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("math,S", MATH_SIDES)
def test_conv3x3_f32_in(fused, weights, math, cin, cout, S):
    w = weights[cin, cout]
    nobias = torch.zeros(cout, device="cuda")
    x, r = _fill(B3, cin, S), _fill(B3, cout, S, seed=1)
    # what the split-f16 arithmetic sees of an f32 input is its PX16-style split hi + lo / 2048; the f32 arithmetic sees x itself
    seen = unpack_px(pack_px(x), B3, cin, S) if math == "f16x3" else x.double()
    zero_in = torch.zeros_like(x)
    for plant, (xin, wt, res, want) in {"one tap": (x, w["tap"], None, _spread(seen, cout)), "residual": (zero_in, w["zero"], r, r.double())}.items():
        name = f"conv3x3 {math} {cin}->{cout} S={S} {plant}"
        out, pre = fused.conv3x3_raw(xin, wt, nobias, res, want_pre=True, math=math)
        check_pre(name, pre, want)
        check_forward(name, out, want)
        if math == "f16x3":
            out2, split = fused.conv3x3_raw(xin, wt, nobias, res, math=math, want_split=True)
            assert torch.equal(out, out2)
            # the Split16 image of the output: per image [16-channel chunk][hi | lo][pixel][16 channels], value / 64 = hi + lo / 2048
            img = split.buf.view(torch.float16).reshape(B3, cout // 16, 2, S * S, 16).double()
            val = (64.0 * (img[:, :, 0] + img[:, :, 1] / 2048.0)).permute(0, 1, 3, 2).reshape(B3, cout, S, S)
            check_forward(name + " split out", val, want, floor=True)
            out3, split3 = fused.conv3x3_raw(xin, wt, nobias, res, math=math, want_split=True)
            assert torch.equal(split.buf, split3.buf)
        assert torch.equal(out, fused.conv3x3_raw(xin, wt, nobias, res, math=math))


def _bias_chunks(C):
    """The sweep as bias vectors of C values (padded with its own first values), dealt out so that every vector spans the whole range:
    a sum or a maximum over one call is then of the activation's own size, as the bias-sum bound assumes."""
    sw = sweep()
    n = (sw.numel() + C - 1) // C * C
    return torch.cat([sw, sw[:n - sw.numel()]]).reshape(C, -1).t().contiguous().cuda()


@pytest.mark.parametrize("math,S", MATH_SIDES)
def test_conv3x3_from_codes(fused, math, S):
    """conv1 from the int8 codes: all-EMPTY boards (no plane set) and zero weights leave pre = bias[c]."""
    B = 2
    codes = torch.ones(B, S, S, dtype=torch.int8, device="cuda")
    w = torch.zeros(32, 3, 3, 3, device="cuda")
    chunks = _bias_chunks(32)
    outs, pres = [], []
    for bias in chunks:
        out, pre = fused.conv3x3_raw(codes, w, bias, codes=True, want_pre=True, math=math)
        outs.append(out)
        pres.append(pre)
    assert torch.equal(outs[-1], fused.conv3x3_raw(codes, w, chunks[-1], codes=True, math=math))
    x = chunks[:, None, :, None, None].expand(-1, B, 32, S, S)
    check_pre(f"conv3x3 codes {math} S={S}", torch.stack(pres), x)
    check_forward(f"conv3x3 codes {math} S={S}", torch.stack(outs), x)


@pytest.mark.parametrize("S", [12, 26, 34])
def test_conv1_px16(fused, S):
    """tron_conv1_px16 and (12x12 / 26x26: its sides) tron_conv1_px16_train the same way: a and z as PX16 images."""
    B = 2
    codes = torch.ones(B, S, S, dtype=torch.int8, device="cuda")
    conv = _module(torch.zeros(32, 3, 3, 3, device="cuda"))
    chunks = _bias_chunks(32)
    for i, bias in enumerate(chunks):
        with torch.no_grad():
            conv.bias.copy_(bias)
        x = bias[None, :, None, None].expand(B, 32, S, S)
        a = fused.conv1_px16(codes, conv, 0.0)
        va = px_value(a)
        assert torch.isfinite(va).all(), bias
        if S != 34:
            at, zt = fused.conv1_px16_train(codes, conv.weight, conv.bias, 0.0)
            vz = px_value(zt)
            assert torch.equal(a.buf, at.buf) and torch.isfinite(vz).all()
            assert ((vz - x.double()).abs() <= out_floor(x)).all(), (i, "z")
        ref = mish64(x)
        err, bound = (va - ref).abs(), 1e-6 * ref.abs() + 2e-9 + out_floor(ref)
        assert (err <= bound).all(), _worst(f"conv1_px16 S={S}", err, bound, x)
    assert torch.equal(a.buf, fused.conv1_px16(codes, conv, 0.0).buf)


# ---- the weight-stationary kernels on PX16 images --------------------------------------------------------------------------------

def _ws_plants(fused, weights, cin, cout, S):
    w = weights[cin, cout]
    xp = to_px(fused, _fill(B3, cin, S))
    rp = to_px(fused, _fill(B3, cout, S, seed=1))
    zp = to_px(fused, torch.zeros(B3, cin, S, S, device="cuda"))
    return {"one tap": (xp, w["frag_tap"], None, _spread(px_value(xp), cout)), "residual": (zp, w["frag_zero"], rp, px_value(rp))}


@pytest.mark.parametrize("S", [12, 26])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_conv_ws(fused, weights, cin, cout, S):
    conv = _module(weights[cin, cout]["zero"])                          # (only its zero bias and its channel counts are read)
    for plant, (xin, frag, res, want) in _ws_plants(fused, weights, cin, cout, S).items():
        name = f"conv_ws {cin}->{cout} S={S} {plant}"
        px = fused.conv_ws(xin, conv, frag, residual=res)
        check_forward(name + " PX16 out", px_value(px), want, floor=True)
        px2, o32, pre = fused.conv_ws(xin, conv, frag, residual=res, want_f32=True, want_pre=True)
        check_pre(name, pre, want)
        check_forward(name + " f32 out", o32, want)
        check_forward(name + " PX16 beside f32", px_value(px2), want, floor=True)
        assert torch.equal(px.buf, fused.conv_ws(xin, conv, frag, residual=res).buf)


@pytest.mark.parametrize("S", [12, 26, 34])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_conv_ws_train(fused, weights, cin, cout, S):
    bias = torch.zeros(cout, device="cuda")
    for plant, (xin, frag, res, want) in _ws_plants(fused, weights, cin, cout, S).items():
        name = f"conv_ws_train {cin}->{cout} S={S} {plant}"
        a, z = fused.conv_ws_train(xin, cout, frag, bias, residual=res)
        check_pre(name, px_value(z), want, floor=True)
        check_forward(name + " PX16 out", px_value(a), want, floor=True)
        a32, z2 = fused.conv_ws_train(xin, cout, frag, bias, residual=res, want_f32=True)
        check_forward(name + " f32 out", a32, want)
        a3, z3 = fused.conv_ws_train(xin, cout, frag, bias, residual=res)
        assert torch.equal(z.buf, z2.buf) and torch.equal(a.buf, a3.buf) and torch.equal(z.buf, z3.buf)


def _planes12(values, B):
    """[B, 64, 12, 12] with one value per (image, channel): the 3x3 / stride-2 average of an interior window is the value itself."""
    return values.reshape(B, 64, 1, 1).expand(B, 64, 12, 12).contiguous()


def test_conv_ws_pool12(fused, nat, weights):
    """conv6 + AvgPool2d(3, 2, 1) in one launch, gradient-free and training, and tron_pool12_px16 behind the layer kernel: constant
    planes, interior pooled cells (rows / columns 1 .. 5: the whole window lies inside the image)."""
    B = 5
    w = weights[64, 64]
    conv = _module(w["zero"])
    bias = torch.zeros(64, device="cuda")
    zero_in = to_px(fused, torch.zeros(B, 64, 12, 12, device="cuda"))
    chunks = _bias_chunks(B * 64)
    for vals in chunks:
        rp = to_px(fused, _planes12(vals, B))
        want = px_value(rp)
        pooled, z = fused.conv_ws_train_pool12(zero_in, w["frag_zero"], bias, rp)
        assert ((px_value(z) - want).abs() <= out_floor(want)).all()
        a = fused.conv_ws(zero_in, conv, w["frag_zero"], residual=rp)
        two = torch.empty(B, 64 * 36, dtype=torch.float32, device="cuda")
        nat.check(nat.lib().tron_pool12_px16(nat.ptr(a.buf), nat.ptr(two), B, nat.stream_ptr()), "tron_pool12_px16")
        p12 = fused.conv_ws_pool12(zero_in, conv, w["frag_zero"], rp)
        half = (B * 2304 * 2 + 255) // 256 * 256                        # (bytes of the hi rows; the lo rows follow)
        raw = p12.buf.view(torch.float16)
        rows = 64.0 * (raw[:B * 2304].double() + raw[half // 2:half // 2 + B * 2304].double() / 2048.0)
        rows = rows.reshape(B, 8, 6, 6, 8).permute(0, 1, 4, 2, 3).reshape(B, 64, 6, 6)       # [b][octet][y][x][8 channels] -> NCHW
        inner = want[:, :, :5, :5]
        ref = mish64(inner)
        for name, got in (("train_pool12", pooled.reshape(B, 64, 6, 6)), ("pool12_px16", two.reshape(B, 64, 6, 6)), ("ws_pool12", rows)):
            g = got[:, :, 1:, 1:].double()
            assert torch.isfinite(got).all(), name
            bound = 1e-6 * ref.abs() + 2e-9 + out_floor(ref)
            err = (g - ref).abs()
            assert (err <= bound).all(), _worst(name, err, bound, inner)
    assert torch.equal(pooled, fused.conv_ws_train_pool12(zero_in, w["frag_zero"], bias, rp)[0])
    assert torch.equal(p12.buf, fused.conv_ws_pool12(zero_in, conv, w["frag_zero"], rp).buf)


# ---- the derivative kernels ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,C", [(12, 64), (12, 32), (26, 64), (26, 32), (34, 64)])
def test_grad_px_from_f32(fused, S, C):
    zp = to_px(fused, _fill(B3, C, S))
    z = px_value(zp)
    g = _signed_pow2((B3, C, S, S), S + C)
    gp, gb = fused.grad_px_from_f32(g, zp)
    info = gp.info.double()
    got = px_value(gp) * info[1]
    # the image stores g m s: its quantisation is out_floor of the scaled reference, brought back to g's units
    ref = g.double() * dmish64(z)
    floor = out_floor(ref * info[0]) * info[1]
    want = check_derivative(f"grad_px_from_f32 S={S} C={C}", got, g, z, floor)
    check_sums(f"grad_px_from_f32 S={S} C={C}", gb, want, info)
    gp2, gb2 = fused.grad_px_from_f32(g, zp)
    assert torch.equal(gp.buf, gp2.buf) and torch.equal(gb, gb2)


@pytest.mark.parametrize("S,C", [(12, 64), (12, 32), (26, 64), (26, 32)])
def test_grad_px_from_pooled(fused, nat, S, C):
    """The entry from the pooled gradient, both layouts: a constant pooled plane 9 c per (image, channel) makes the pooling's
    backward c times the number of windows over the pixel (1, 2 or 4): known exactly."""
    L = nat.lib()
    PS = S // 2
    zp = to_px(fused, _fill(B3, C, S))
    z = px_value(zp)
    c = _signed_pow2((B3, C, 1, 1), S * C)
    gpool = (9.0 * c).expand(B3, C, PS, PS).contiguous()
    odd = (torch.arange(S, device="cuda") % 2 == 1) & (torch.arange(S, device="cuda") // 2 + 1 < PS)
    count = (1 + odd.double())[:, None] * (1 + odd.double())[None, :]
    for layout in (0, 1):
        src = gpool.permute(0, 2, 3, 1).contiguous() if layout else gpool
        sc4 = torch.zeros(4, device="cuda")
        outs = []
        for _ in range(2):
            out = fused.GradPX(B3, C, S, "cuda")
            gb = torch.empty(C, device="cuda")
            ws = torch.empty(int(L.tron_px16_grad_workspace(B3, C)), dtype=torch.uint8, device="cuda")
            nat.check(L.tron_absmax_pow2(nat.ptr(src), src.numel(), 15, nat.ptr(sc4), nat.stream_ptr()))
            nat.check(L.tron_px16_grad_from_pooled(nat.ptr(src), layout, nat.ptr(zp.buf), nat.ptr(sc4), B3, C, S, nat.ptr(out.buf),
                                                   nat.ptr(out.info), nat.ptr(gb), nat.ptr(ws), nat.stream_ptr()))
            outs.append((out, gb))
        out, gb = outs[0]
        assert torch.equal(out.buf, outs[1][0].buf) and torch.equal(gb, outs[1][1])
        info = out.info.double()
        # (9 c k) (1 / 9) in f32: the kernel's product with its rounded 1 / 9 is within an ulp of c k — part of g, not of mish'
        g = ((9.0 * c).float() * count.float() * torch.tensor(1.0 / 9.0, device="cuda")).double().expand(B3, C, S, S)
        got = px_value(out) * info[1]
        ref = g * dmish64(z)
        floor = out_floor(ref * info[0]) * info[1]
        want = check_derivative(f"grad_px_from_pooled S={S} C={C} layout={layout}", got, g, z, floor)
        check_sums(f"grad_px_from_pooled S={S} C={C} layout={layout}", gb, want, info)


@pytest.mark.parametrize("S", [12, 26, 34])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_conv_ws_dgrad(fused, weights, cin, cout, S):
    """(conv^T(g, W) + extra) mish'(z below): the gradient through the one-tap weights (input channel ci collects the output
    channels co = ci mod cin: magnitudes 1 and 1/4 apart, so the sum is exact and never 0), or through `extra` with zero weights."""
    w = weights[cin, cout]
    zp = to_px(fused, _fill(B3, cin, S))
    z = px_value(zp)
    g = _signed_pow2((B3, cout, S, S), S + cout, lo=0, hi=0)
    g[:, cin:] *= 0.25
    gpx, gval = _grad_px(fused, g)
    epx, eval_ = _grad_px(fused, _signed_pow2((B3, cin, S, S), S + cin + 7, lo=3, hi=5))      # (8 .. 32: never cancels the tap's +-1, +-1.25)
    zero_g, _ = _grad_px(fused, torch.zeros(B3, cout, S, S, device="cuda") + 1.0)
    zero_g.buf.zero_()
    zero_g.info[4:] = 0.0
    gin = gval.reshape(B3, cout // cin, cin, S, S).sum(1)
    for plant, (gp, rot, ex, gwant) in {"one tap": (gpx, w["rot_tap"], None, gin), "extra": (zero_g, w["rot_zero"], epx, eval_),
                                        "one tap + extra": (gpx, w["rot_tap"], epx, gin + eval_)}.items():
        name = f"conv_ws_dgrad {cin}->{cout} S={S} {plant}"
        wn = w["wn"][0:1] if rot is w["rot_tap"] else w["wn"][1:2]
        out, o32, gb = fused.conv_ws_dgrad(gp, cin, rot, wn, zp, extra=ex, want_f32=True)
        info = out.info.double()
        want = check_derivative(name + " f32 out", o32, gwant, z)
        floor = out_floor(want * info[0]) * info[1]
        check_derivative(name + " PX16 out", px_value(out) * info[1], gwant, z, floor)
        check_sums(name, gb, want, info)
        out2, _, gb2 = fused.conv_ws_dgrad(gp, cin, rot, wn, zp, extra=ex)
        assert torch.equal(out.buf, out2.buf) and torch.equal(gb, gb2)


@pytest.mark.parametrize("S", [12, 26])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_conv3x3_dgrad_mish(fused, cin, cout, S):
    """tron_conv3x3_dgrad_mish (f32 tensors, split-f16 arithmetic): the same plants on f32 planes."""
    tap = _one_tap(cin, cout)
    assert fused.dgrad_mish_supported(tap, S)
    z = _fill(B3, cin, S)
    g = _signed_pow2((B3, cout, S, S), S + cout, lo=0, hi=0)
    g[:, cin:] *= 0.25
    ex = _signed_pow2((B3, cin, S, S), S + cin + 7, lo=3, hi=5)          # (8 .. 32: never cancels the tap's +-1, +-1.25)
    gin = torch.einsum("oi,bohw->bihw", tap[:, :, 1, 1].double(), g.double())
    absmax = g.abs().reshape(B3, -1).amax(1).contiguous()
    for plant, (gp, wt, e, gwant) in {"one tap": (g, tap, None, gin), "extra": (torch.zeros_like(g), torch.zeros_like(tap), ex, ex.double()),
                                      "one tap + extra": (g, tap, ex, gin + ex.double())}.items():
        name = f"conv3x3_dgrad_mish {cin}->{cout} S={S} {plant}"
        am_in = absmax if gp is g else torch.zeros_like(absmax)
        got, gb, am = fused.conv3x3_dgrad_mish(gp, wt, am_in, z, e)
        want = check_derivative(name, got, gwant, z)
        check_sums(name, gb, want)
        top = want.abs().amax((0, 2, 3))
        assert ((am.double() - top).abs() <= 2e-6 * top.max()).all(), name
        got2, gb2, am2 = fused.conv3x3_dgrad_mish(gp, wt, am_in, z, e)
        assert torch.equal(got, got2) and torch.equal(gb, gb2) and torch.equal(am, am2)


# ---- the head's pool + conv7 + mish (tron_head.hip) --------------------------------------------------------------------------------

@pytest.mark.parametrize("side", [26, 34])
def test_pool_conv7(nat, fused, side):
    """tron_pool_conv7_fwd / _bwd (and, at 26, the PX16 / pooled forms): zero weights, pre = bias[c]; the backward's bias
    gradient is the sum of g mish'(pre) over images and pixels, g signed powers of two."""
    L = nat.lib()
    B, o = 2, (side // 2 + 1) // 2
    x = torch.randn(B, 64, side, side, generator=torch.Generator().manual_seed(side)).cuda()
    xp = fused.PX16.from_f32(x) if side == 26 else None
    w = torch.zeros(64, 64, 7, 7, device="cuda")
    gy = _signed_pow2((B, 64, o, o), side)
    saved = torch.empty(int(L.tron_pool_conv7_saved_bytes(B, side)), dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(L.tron_pool_conv7_workspace(B, side)), dtype=torch.uint8, device="cuda")
    st = nat.stream_ptr()
    forms = [("f32", L.tron_pool_conv7_fwd, x, L.tron_pool_conv7_bwd)]
    if side == 26:
        forms.append(("px16", L.tron_pool_conv7_fwd_px16, xp.buf, L.tron_pool_conv7_bwd_pooled))
    for form, fwd, xin, bwd in forms:
        ys, pres, gbs = [], [], []
        chunks = _bias_chunks(64)
        for bias in chunks:
            pre = torch.empty(B, o * o, 64, device="cuda")
            y = torch.empty(B, 64 * o * o, device="cuda")
            nat.check(fwd(nat.ptr(xin), B, side, nat.ptr(w), nat.ptr(bias), nat.ptr(saved), nat.ptr(pre), nat.ptr(y), nat.ptr(ws), st), form)
            gb = torch.empty(64, device="cuda")
            gx = torch.empty(B, (side // 2) ** 2, 64, device="cuda") if form == "px16" else torch.empty_like(x)
            nat.check(bwd(nat.ptr(gy.reshape(B, -1)), nat.ptr(pre), nat.ptr(saved), nat.ptr(w), B, side, nat.ptr(gx), None, nat.ptr(gb),
                          nat.ptr(ws), st), form)
            assert torch.count_nonzero(gx) == 0                          # zero weights: nothing reaches the input
            ys.append(y.reshape(B, 64, o, o))
            pres.append(pre.reshape(B, o, o, 64).permute(0, 3, 1, 2))
            gbs.append(gb)
        gb_again = torch.empty(64, device="cuda")
        nat.check(bwd(nat.ptr(gy.reshape(B, -1)), nat.ptr(pre), nat.ptr(saved), nat.ptr(w), B, side, nat.ptr(gx), None, nat.ptr(gb_again), nat.ptr(ws), st), form)
        assert torch.equal(gb_again, gbs[-1])
        planted = chunks[:, None, :, None, None].expand(-1, B, 64, o, o)
        name = f"pool_conv7 {form} side={side}"
        check_pre(name, torch.stack(pres), planted)
        check_forward(name, torch.stack(ys), planted)
        d = dmish64(planted)                                          # [chunk, B, 64, o, o]
        ref = gy.double()[None] * d
        sums, scale = ref.sum((1, 3, 4)), ref.abs().amax((1, 2, 3, 4))
        got = torch.stack(gbs).double()
        assert torch.isfinite(got).all(), name
        bound = 1e-5 * sums.abs().amax(1) + 1e-6 * scale
        err = (got - sums).abs().amax(1)
        print(f"{name}: bias sums worst {(err / bound).max().item():.3g} of the bound")
        assert (err <= bound).all(), (name, chunks[int((err / bound).argmax())].tolist())
