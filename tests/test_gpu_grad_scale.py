"""The gradient scales of the matrix-core backward kernels (csrc/tron_f16x3.hpp: every gradient operand travels as split f16
under one power of two found from maxima of |g|), producer by producer and consumer by consumer:

  * tron_absmax_pow2 against the host model of tests/grad_scale_support.py, with the maximum planted at every seam of its loops
    and over every f32 exponent;
  * the records tron_bias_mish_bwd and tron_conv3x3_dgrad_mish leave for the next kernel, bit for bit against the gradient
    they wrote;
  * one spike of +-1024 in a uniform(-1, 1) gradient — a maximum that a skipped tail, image, channel or border pixel would miss,
    after which the spike is scaled to 2^23 and overflows f16 — through every entry point that scales, with the records of the
    REAL producers (the pre-pass of tron_conv3x3_wgrad, tron_bias_mish_bwd's scratch, tron_absmax_pow2's record through
    tron_px16_grad_from_f32 / _from_pooled), against float64 at the tolerance of the entry point's own test;
  * an absmax array whose only large record sits at either end or at a seam of the consumers' strided loops;
  * one workspace used for a large gradient, then a small one, then zeros; maxima on the half-open edge of [2^13, 2^14) and at
    the ends of the scaled range.

tron_linear_wgrad is not here: k_lin_wgrad multiplies in plain f32 and takes no scale."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional

import grad_scale_support as G
from activation_range_support import px_value, to_px as _to_px

SPIKE_SHAPES = [(12, 1, 32, 32), (12, 3, 32, 64), (12, 37, 64, 64), (12, 37, 64, 32), (26, 3, 32, 64), (26, 3, 64, 64)]
PX_SHAPES = [(12, 3, 32, 32), (12, 37, 32, 64), (12, 37, 64, 64), (26, 3, 64, 64)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fused():
    import config  # noqa: F401
    from Net import fused
    return fused


@pytest.fixture(scope="module")
def nat(fused):
    return fused.nat


# ---- helpers -----------------------------------------------------------------------------------------------------------------

def _uniform(shape, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(shape, device="cuda", generator=gen) * 2.0 - 1.0


def _randn(shape, seed, scale=1.0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=gen) * scale


def _spiked(shape, pos, n, seed):
    """uniform(-1, 1) with the entry at pos set to +-1024 (the sign alternates with n)."""
    g = _uniform(shape, seed)
    g[pos] = G.SPIKE if n % 2 == 0 else -G.SPIKE
    return g


def _held(got, ref, tol, what, rest=None):
    """finite; |got - ref| < tol max |ref|; and, rest = a mask or slice of the entries the spike cannot reach, the same relative
    to the largest entry among those."""
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got.double() - ref).abs()
    top = ref.abs().max().item()
    assert err.max().item() < tol * top, f"{what}: {err.max().item() / top:.3g} of the largest entry, bound {tol}"
    if rest is not None and rest.any():
        top_r = ref[rest].abs().max().item()
        assert top_r > 0.0
        e_r = err[rest].max().item()
        assert e_r < tol * top_r, f"{what}: {e_r / top_r:.3g} of the largest entry the spike cannot reach, bound {tol}"


def _others(shape, dim, index):
    """A mask over `shape` that leaves out slice `index` of dimension `dim` (other images, other output channels)."""
    m = torch.ones(shape, dtype=torch.bool, device="cuda")
    m.select(dim, index).fill_(False)
    return m


def _wgrad64(x, gp):
    wd = torch.zeros(gp.shape[1], x.shape[1], 3, 3, dtype=torch.float64, device="cuda", requires_grad=True)
    F.conv2d(x.double(), wd, padding=1).backward(gp.double())
    return wd.grad


def _dgrad64(gp, w, cin):
    B, _, S, _ = gp.shape
    xd = torch.zeros(B, cin, S, S, dtype=torch.float64, device="cuda", requires_grad=True)
    F.conv2d(xd, w.double(), padding=1).backward(gp.double())
    return xd.grad


def _mish_bwd64(z, g):
    zd = z.double().detach().clone().requires_grad_(True)
    F.mish(zd).backward(g.double())
    return zd.grad


def _produced(g, pos, seed):
    """The gradient tron_bias_mish_bwd writes for grad_out = g and its scratch maxima [C * 64] — the real producer's records.
    The pre-activation is N(0, 2) with 3.0 under the spike (mish' = 1.02: the spike stays the maximum by three orders)."""
    from Net import activations
    pre = _randn(g.shape, seed + 1000, 2.0)
    pre[pos] = 3.0
    gp, _, rec = activations.bias_mish_bwd(pre, g, want_absmax=True)
    assert gp[pos].abs().item() > 1000.0 and rec.numel() == g.shape[1] * G.BIAS_SEGS
    rest = gp.abs().clone()
    rest[pos] = 0.0
    assert rest.max().item() < 1.2                                    # |mish'| <= 1.09
    return gp, rec


# ---- 2. tron_absmax_pow2 against the model ------------------------------------------------------------------------------------

def _pow2(nat, x, target, out):
    nat.check(nat.lib().tron_absmax_pow2(nat.ptr(x), x.numel(), target, nat.ptr(out), nat.stream_ptr()), "tron_absmax_pow2")


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 1023, 1024, 1025, 4099, 1_000_003])
def test_absmax_pow2_finds_a_maximum_planted_anywhere(nat, n):
    """uniform(-1, 1) 2^-4 with +-v planted at both ends, in the n % 4 tail, in the middle, at the ends of a 1 024- and a 4 096-float
    block and (n = 1 000 003: 62 workgroups) in the float4s a workgroup reads on its second grid-stride trip: out[1] == v and
    out[0] == the model, exactly.  v = 1, 1.5 (2^0 is the half-open interval's closed end) and 3 2^-3."""
    grid = G.pow2_grid(n)
    stride = grid * 1024 if n // 4 > grid * 1024 else None
    assert (stride is not None) == (n == 1_000_003)
    pos = G.pow2_positions(n, stride)
    base = torch.from_numpy(G.background(n, n)).cuda()
    cases = [(p, v * (1 if (k + j) % 2 == 0 else -1), t) for k, p in enumerate(pos)
             for j, (v, t) in enumerate(((1.0, 14), (1.5, 15), (0.375, 16)))]
    outs = torch.zeros(len(cases), 4, device="cuda")
    for k, (p, v, t) in enumerate(cases):
        x = base.clone()
        x[p] = v
        _pow2(nat, x, t, outs[k])
    got = outs.cpu().numpy()
    for k, (p, v, t) in enumerate(cases):
        assert got[k, 1] == abs(np.float32(v)), (n, p, v, got[k])
        assert got[k, 0] == G.absmax_pow2(abs(v), t), (n, p, v, t, got[k])


def test_absmax_pow2_over_every_exponent(nat):
    """Every f32 exponent at both mantissa ends and the denormals as the planted maximum of 1 025 floats (position 1 024 is the
    n % 4 tail), targets 14 / 15 / 16 and the +-60 the entry accepts: out[1] == v, out[0] == the model (the clamp to 2^+-60
    included), exactly.  And an all-zero tensor: {1, 0}."""
    n, pos = 1025, (0, 1024, 512, 1023, 1021)
    vals = G.sweep()
    cases = [(pos[k % 5], v if k % 2 == 0 else -v, (14, 15, 16, -60, 60, 0)[k % 6]) for k, v in enumerate(vals)]
    outs = torch.zeros(len(cases) + 1, 4, device="cuda")
    for k, (p, v, t) in enumerate(cases):
        _pow2(nat, torch.from_numpy(G.planted(n, p, v, k)).cuda(), t, outs[k])
    _pow2(nat, torch.zeros(n, device="cuda"), 14, outs[-1])
    got = outs.cpu().numpy()
    for k, (p, v, t) in enumerate(cases):
        assert got[k, 1] == abs(v), (p, v, t, got[k])
        assert got[k, 0] == G.absmax_pow2(abs(v), t), (p, v, t, got[k])
    assert got[-1, 0] == 1.0 and got[-1, 1] == 0.0


# ---- 3. the producers' records are exact --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("C", [32, 64])
def test_bias_mish_bwd_leaves_every_segment_s_maximum(fused, C, N):
    """scratch[C 64 + c 64 + seg] == max |grad_pre[n0:n1, c]| bit for bit, n0, n1 = N seg / 64, N (seg + 1) / 64, 0 for an empty
    segment (N < 64: most of them; 65, 130: ragged) — from the grad_pre the kernel itself wrote; grad_pre and the bias gradient
    against float64 with test_training_conv_gradients_match_float64's 2e-5 max(1, largest entry)."""
    from Net import activations
    pre = _randn((N, C, 12, 12), 7 * N + C, 2.0)
    pre[0, 0, 0, :4] = torch.tensor([30.0, -30.0, 21.0, -90.0], device="cuda")
    g = _randn((N, C, 12, 12), 7 * N + C + 1)
    gp, gb, rec = activations.bias_mish_bwd(pre, g, want_absmax=True)
    want = torch.zeros(C, G.BIAS_SEGS, device="cuda")
    for seg in range(G.BIAS_SEGS):
        n0, n1 = G.segment_bounds(N, seg)
        if n1 > n0:
            want[:, seg] = gp[n0:n1].abs().amax((0, 2, 3))
    assert torch.equal(rec.reshape(C, G.BIAS_SEGS), want)
    assert rec.max().item() == gp.abs().max().item()
    ref = _mish_bwd64(pre, g)
    for a, b in ((gp, ref), (gb, ref.sum((0, 2, 3)))):
        assert (a.double() - b).abs().max().item() < 2e-5 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("S,B", [(12, 1), (12, 37), (12, 131), (26, 3)])
@pytest.mark.parametrize("cin,cout", [(32, 64), (64, 64)])
def test_dgrad_mish_channel_maxima_are_those_of_what_it_wrote(fused, S, B, cin, cout):
    """absmax_below == max |grad_pre_below| over (image, pixel), bit for bit, with a spike in the last image's last pixel."""
    w = _randn((cout, cin, 3, 3), S + B, 0.1)
    gp = _spiked((B, cout, S, S), (B - 1, cout - 1, S - 1, S - 1), B, S + B + 1)
    z = _randn((B, cin, S, S), S + B + 2, 2.0)
    got, _, am = fused.conv3x3_dgrad_mish(gp, w, gp.abs().reshape(B, -1).amax(1).contiguous(), z, None)
    assert torch.equal(am, got.abs().amax((0, 2, 3)))


# ---- 4. a spike through every consumer ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,B,cin,cout", SPIKE_SHAPES)
def test_wgrad_with_a_spike_and_the_producers_records(fused, S, B, cin, cout):
    """tron_conv3x3_wgrad on the gradient tron_bias_mish_bwd wrote, scaled by its own pre-pass (absmax=None) and by that kernel's
    scratch maxima: finite and within test_conv3x3_wgrad_matches_float64's 2e-6 of the largest entry; the other output channels
    — the spike does not reach them — within 2e-6 of THEIR largest entry (they are scaled to 2^3 instead of 2^13: hi + lo 2^-11
    keeps 2^-22 either way, lo's subnormal floor 2^-35 of the scaled maximum is 2^-38 of them)."""
    x = _randn((B, cin, S, S), S + B + cin)
    for n, (name, pos) in enumerate(G.spike_positions(B, cout, S, octet=False)):
        gp, rec = _produced(_spiked((B, cout, S, S), pos, n, S + B + cout + n), pos, n)
        ref = _wgrad64(x, gp)
        rest = _others(ref.shape, 0, pos[1])
        for absmax in (None, rec):
            _held(fused.conv3x3_wgrad(x, gp, absmax), ref, 2e-6, f"wgrad {name} {'pre-pass' if absmax is None else 'records'}", rest)


@pytest.mark.parametrize("S,B,cin,cout", SPIKE_SHAPES)
def test_dgrad_with_a_spike_and_the_producers_records(fused, S, B, cin, cout):
    """tron_conv3x3_dgrad with tron_bias_mish_bwd's records and with per-image maxima (n_absmax = B): 2e-6 as in
    test_conv3x3_dgrad_matches_float64_at_gradient_magnitudes, over everything and over the other images."""
    w = _randn((cout, cin, 3, 3), S + B + cin, 0.1)
    for n, (name, pos) in enumerate(G.spike_positions(B, cout, S, octet=False)):
        gp, rec = _produced(_spiked((B, cout, S, S), pos, n, S + B + cout + n), pos, n)
        ref = _dgrad64(gp, w, cin)
        rest = _others(ref.shape, 0, pos[0])
        for what, absmax in (("records", rec), ("per image", gp.abs().reshape(B, -1).amax(1).contiguous())):
            _held(fused.conv3x3_dgrad(gp, w, absmax), ref, 2e-6, f"dgrad {name} {what}", rest)


@pytest.mark.parametrize("S,B,cin,cout", [s for s in SPIKE_SHAPES if s[2:] != (64, 32) or s[0] == 12])
def test_dgrad_mish_with_a_spike_and_the_producers_records(fused, S, B, cin, cout):
    """tron_conv3x3_dgrad_mish likewise, test_dgrad_mish_matches_float64's bounds (3e-6; sums 1e-5), maxima exact."""
    w = _randn((cout, cin, 3, 3), S + B + cin, 0.1)
    z = _randn((B, cin, S, S), S + B + cin + 1, 2.0)
    for n, (name, pos) in enumerate(G.spike_positions(B, cout, S, octet=False)):
        gp, rec = _produced(_spiked((B, cout, S, S), pos, n, S + B + cout + n), pos, n)
        ref = _mish_bwd64(z, _dgrad64(gp, w, cin))
        got, gb, am = fused.conv3x3_dgrad_mish(gp, w, rec, z, None)
        _held(got, ref, 3e-6, f"dgrad_mish {name}", _others(ref.shape, 0, pos[0]))
        sums = ref.sum((0, 2, 3))
        assert (gb.double() - sums).abs().max().item() / max(sums.abs().max().item(), ref.abs().max().item()) < 1e-5, name
        assert torch.equal(am, got.abs().amax((0, 2, 3))), name


def _large_record_cases(gp, C):
    """absmax arrays of 1, B and C 64 records whose only large one — the true maximum; the others bound the rest of the
    gradient — sits at either end or at a seam of the consumers' loops (threads 255 | 256, 511 | 512)."""
    B = gp.shape[0]
    top = gp.abs().max()
    for n in sorted({1, B, C * G.BIAS_SEGS}):
        for i in G.absmax_indices(n):
            a = torch.full((n,), 2.0, device="cuda")
            a[i] = top
            yield n, i, a


@pytest.mark.parametrize("S,B,cin,cout", [(12, 37, 32, 32), (12, 37, 64, 64), (26, 3, 32, 64), (26, 3, 64, 64)])
def test_consumers_read_every_absmax_record(fused, S, B, cin, cout):
    """wave_absmax (k_wgrad: 256 threads, k_wgrad_rows: 256 / 512) and k_conv3x3_f16's own loop (512) over n_absmax = 1, B and
    C 64 records of which one holds the spike: every placement gives what the first gives, bit for bit (the scale is the same
    power of two), and that is within the entry points' float64 bounds."""
    pos = (B - 1, cout - 1, S - 1, S - 1)
    gp = _spiked((B, cout, S, S), pos, 0, S + B)
    x = _randn((B, cin, S, S), S + B + 1)
    w = _randn((cout, cin, 3, 3), S + B + 2, 0.1)
    z = _randn((B, cin, S, S), S + B + 3, 2.0)
    first = None
    for n, i, a in _large_record_cases(gp, cout):
        got = (fused.conv3x3_wgrad(x, gp, a), fused.conv3x3_dgrad(gp, w, a), fused.conv3x3_dgrad_mish(gp, w, a, z, None)[0])
        assert all(bool(torch.isfinite(t).all()) for t in got), (n, i)
        if first is None:
            first = got
            dg = _dgrad64(gp, w, cin)
            _held(got[0], _wgrad64(x, gp), 2e-6, "wgrad", _others(got[0].shape, 0, pos[1]))
            _held(got[1], dg, 2e-6, "dgrad", _others(dg.shape, 0, pos[0]))
            _held(got[2], _mish_bwd64(z, dg), 3e-6, "dgrad_mish", _others(dg.shape, 0, pos[0]))
        else:
            assert all(torch.equal(a_, b_) for a_, b_ in zip(got, first)), (n, i)


def _entry_checks(gp, gb, ref, C, tol, what, pos):
    """test_gradient_image_entry's bounds on a gradient image, its sums and its record."""
    scale = ref.abs().max().item()
    val = px_value(gp) * float(gp.info[1].item())
    _held(val, ref, tol, what, _others(ref.shape, 0, pos[0]))
    sums = ref.sum((0, 2, 3))
    assert (gb.double() - sums).abs().max().item() < 1e-5 * sums.abs().max().item() + 1e-6 * scale, what
    info = gp.info.cpu().numpy()
    top = info[4:4 + C].max()
    assert info[0] * info[1] == 1.0 and abs(top - scale) <= 2e-6 * scale, what
    assert (info[4:4 + C] >= ref.abs().amax((0, 2, 3)).cpu().numpy() * (1 - 1e-5)).all(), what
    assert top * info[0] < 2.0 ** 15, what
    return val


@pytest.mark.parametrize("S,B,cin,cout", PX_SHAPES)
def test_px16_chain_with_a_spike(fused, S, B, cin, cout):
    """tron_absmax_pow2 -> tron_px16_grad_from_f32 (2e-6, test_gradient_image_entry) and, on that image and its record,
    tron_conv3x3_wgrad_px16 (3e-6, test_weight_gradient_from_px16_images) and tron_conv3x3_ws_dgrad (4e-6, sums 2e-5 + 2e-6:
    test_input_gradient_with_fused_activation_backward), both against float64 of what the image holds.  Spikes also in the last
    channel of the first and of the last octet."""
    z = _randn((B, cout, S, S), S + B + cout, 3.0)
    zb = _randn((B, cin, S, S), S + B + cin + 1, 2.0)
    x = _randn((B, cin, S, S), S + B + cin + 2, 1.5)
    W = _randn((cout, cin, 3, 3), S + B + 3, 0.08)
    rot, wn = fused._split_jobs([W], "tron_conv3x3_ws_split_weights_bwd", True)
    xpx, zbpx = _to_px(fused, x), _to_px(fused, zb)
    for n, (name, pos) in enumerate(G.spike_positions(B, cout, S)):
        g = _spiked((B, cout, S, S), pos, n, S + B + n)
        zz = z.clone()
        zz[pos] = 3.0
        zpx = _to_px(fused, zz)
        gp, gb = fused.grad_px_from_f32(g, zpx)
        val = _entry_checks(gp, gb, _mish_bwd64(px_value(zpx), g), cout, 2e-6, f"grad entry {name}", pos)
        assert val[pos].abs().item() > 1000.0
        gw = fused.conv3x3_wgrad_px(xpx, gp)
        _held(gw, _wgrad64(px_value(xpx), val), 3e-6, f"wgrad_px {name}", _others(gw.shape, 0, pos[1]))
        out, o32, gbb = fused.conv_ws_dgrad(gp, cin, rot[0], wn[0:1], zbpx, want_f32=True)
        ref = _mish_bwd64(px_value(zbpx), _dgrad64(val, W, cin))
        rest = _others(ref.shape, 0, pos[0])
        _held(px_value(out) * float(out.info[1].item()), ref, 4e-6, f"ws_dgrad image {name}", rest)
        _held(o32, ref, 4e-6, f"ws_dgrad f32 {name}", rest)
        sums = ref.sum((0, 2, 3))
        assert (gbb.double() - sums).abs().max().item() < 2e-5 * sums.abs().max().item() + 2e-6 * ref.abs().max().item(), name


@pytest.mark.parametrize("S,B", [(12, 3), (12, 37), (26, 3)])
def test_px16_entry_from_the_pooled_gradient_with_a_spike(fused, nat, S, B):
    """tron_absmax_pow2(15) -> tron_px16_grad_from_pooled, pooled planes (12x12) and channels-last (26x26), the spike in the
    pooled gradient: test_gradient_image_entry_from_the_pooled_gradient's 2e-6 and sums, other images relative to their own."""
    L = nat.lib()
    C, PS = 64, S // 2
    z = _randn((B, C, S, S), S + B, 2.5)
    for n, (name, pos) in enumerate(G.spike_positions(B, C, PS)):
        gpool = _spiked((B, C, PS, PS), pos, n, S + B + n)
        zz = z.clone()
        zz[pos[0], pos[1]] = 3.0                                     # mish' = 1.02 under every window the spike feeds
        zpx = _to_px(fused, zz)
        zd = px_value(zpx).requires_grad_(True)
        F.avg_pool2d(F.mish(zd), 3, stride=2, padding=1).backward(gpool.double())
        src = gpool.permute(0, 2, 3, 1).contiguous() if S == 26 else gpool.contiguous()
        sc4 = torch.zeros(4, device="cuda")
        out = fused.GradPX(B, C, S, "cuda")
        gb = torch.empty(C, device="cuda")
        ws = torch.empty(int(L.tron_px16_grad_workspace(B, C)), dtype=torch.uint8, device="cuda")
        nat.check(L.tron_absmax_pow2(nat.ptr(src), src.numel(), 15, nat.ptr(sc4), nat.stream_ptr()))
        nat.check(L.tron_px16_grad_from_pooled(nat.ptr(src), int(S == 26), nat.ptr(zpx.buf), nat.ptr(sc4), B, C, S, nat.ptr(out.buf),
                                               nat.ptr(out.info), nat.ptr(gb), nat.ptr(ws), nat.stream_ptr()))
        assert sc4[1].item() == G.SPIKE and sc4[0].item() == G.absmax_pow2(G.SPIKE, 15)
        _entry_checks(out, gb, zd.grad, C, 2e-6, f"pooled entry {name}", pos)


def test_pool_conv7_bwd_with_a_spike(nat):
    """tron_pool_conv7_bwd at 26x26, B = 3 (its own tron_absmax_pow2 over the output gradient): all three gradients within
    test_pool_conv7_matches_float64's 5e-6; the input gradient of the other images within 5e-6 of their largest entry."""
    import test_gpu_conv7 as conv7
    B, side, o = 3, 26, 7
    x = _randn((B, 64, side, side), 1, 1.5)
    w = _randn((64, 64, 7, 7), 2, 0.02)
    b = _randn((64,), 3, 0.1)
    for n, (name, pos) in enumerate(G.spike_positions(B, 64, o)):
        gy = _spiked((B, 64, o, o), pos, n, 10 + n).reshape(B, -1)
        _, _, gx_w, gw_w, gb_w = conv7._reference(x, w, b, gy)
        _, _, gx, gw, gb = conv7._run(nat, x, w, b, gy)
        _held(gx, gx_w, 5e-6, f"conv7 gx {name}", _others(gx.shape, 0, pos[0]))
        _held(gw, gw_w, 5e-6, f"conv7 gw {name}")
        _held(gb, gb_w, 5e-6, f"conv7 gb {name}")


@pytest.mark.parametrize("C", [32, 64])
def test_kfac_gradient_factor_with_a_spike(C):
    """tron_kfac_patch_gram's gradient factor (k_gram_nchw) with in_scale from Net/kfac.py::_pow2_scale — tron_absmax_pow2(16) —
    on integers {-2 .. 2} (uniform(-1, 1) would not let the neighbours' bound, bit equality with float64, hold) with one +-1024:
    a missed spike is scaled to 2^18 and overflows.  The scale is the model's; the factor is float64's bit for bit."""
    from Net import kfac
    import kfac_gram_support as K
    import test_gpu_kfac_gram as kg
    B, S = 3, 12
    for n, (name, pos) in enumerate(G.spike_positions(B, C, S)):
        g = K.ints((B, C, S, S), False, 50 + n, "cuda")
        g[pos] = G.SPIKE if n % 2 == 0 else -G.SPIKE
        s = kfac._pow2_scale(g)
        assert s.item() == G.absmax_pow2(G.SPIKE, 16) == K.pow2_scale_model(g), name
        assert K.exact_condition(g, s.item(), K.NCHW_GEOMETRY) < K.EXACT_LIMIT
        got = kg.call_patch(g, K.NCHW_GEOMETRY, 0.25, s.item())           # (a power-of-two factor scale: the last product is exact)
        assert bool(torch.isfinite(got).all()), name
        assert torch.equal(got.double(), K.ref_gram(g, 0.25, K.NCHW_GEOMETRY)), name


# ---- 5. reuse, interval edges, range limits -----------------------------------------------------------------------------------

def _abi_runs(fused, nat, S, B, cin, cout):
    """Every entry point of part 4 that owns scratch, through the C ABI with caller-held buffers: name -> (bytes of each buffer,
    run(g, buffers) -> tuple of outputs), g f32 [B, cout, S, S]."""
    L = nat.lib()
    st = nat.stream_ptr
    x = _randn((B, cin, S, S), 1)
    w = _randn((cout, cin, 3, 3), 2, 0.1)
    z = _randn((B, cin, S, S), 3, 2.0)
    zo = _randn((B, cout, S, S), 4, 2.0)
    xpx, zpx, zopx = _to_px(fused, x), _to_px(fused, z), _to_px(fused, zo)
    rot, wn = fused._split_jobs([w], "tron_conv3x3_ws_split_weights_bwd", True)
    new = lambda *shape: torch.empty(*shape, device="cuda")

    def bias_mish(g, bufs):
        gp, gb = torch.empty_like(g), new(cout)
        nat.check(L.tron_bias_mish_bwd(nat.ptr(zo), nat.ptr(g), nat.ptr(gp), nat.ptr(gb), nat.ptr(bufs[0]), B, cout, S * S, st()))
        return gp, gb, bufs[0].view(torch.float32)[cout * 64:cout * 128].clone()

    def wgrad(g, bufs):
        gw = new(cout, cin, 3, 3)
        nat.check(L.tron_conv3x3_wgrad(nat.ptr(x), nat.ptr(g), None, 0, nat.ptr(gw), B, cin, cout, S, nat.ptr(bufs[0]), st()))
        return (gw,)

    def dgrad(g, bufs):
        gx = new(B, cin, S, S)
        am = g.abs().reshape(B, -1).amax(1).contiguous()
        nat.check(L.tron_conv3x3_dgrad(nat.ptr(g), nat.ptr(w), nat.ptr(am), B, nat.ptr(gx), B, cin, cout, S, nat.ptr(bufs[0]), st()))
        return (gx,)

    def dgrad_mish(g, bufs):
        out, gb, amb = new(B, cin, S, S), new(cin), new(cin)
        am = g.abs().reshape(B, -1).amax(1).contiguous()
        nat.check(L.tron_conv3x3_dgrad_mish(nat.ptr(g), nat.ptr(w), nat.ptr(am), B, None, nat.ptr(z), nat.ptr(out), nat.ptr(gb), nat.ptr(amb),
                                            B, cin, cout, S, nat.ptr(bufs[0]), st()))
        return out, gb, amb

    def px_chain(g, bufs):
        """tron_absmax_pow2 (its record zeroed by the caller, as the entry asks) -> grad_from_f32 -> wgrad_px16 and ws_dgrad."""
        sc = torch.zeros(4, device="cuda")
        gp, gb = fused.GradPX(B, cout, S, "cuda"), new(cout)
        nat.check(L.tron_absmax_pow2(nat.ptr(g), g.numel(), 14, nat.ptr(sc), st()))
        nat.check(L.tron_px16_grad_from_f32(nat.ptr(g), nat.ptr(zopx.buf), nat.ptr(sc), B, cout, S, nat.ptr(gp.buf), nat.ptr(gp.info), nat.ptr(gb),
                                            nat.ptr(bufs[0]), st()))
        gw = new(cout, cin, 3, 3)
        nat.check(L.tron_conv3x3_wgrad_px16(nat.ptr(xpx.buf), nat.ptr(gp.buf), nat.ptr(gp.info), nat.ptr(gw), B, cin, cout, S, nat.ptr(bufs[1]), st()))
        out, o32, gbb = fused.GradPX(B, cin, S, "cuda"), new(B, cin, S, S), new(cin)
        nat.check(L.tron_conv3x3_ws_dgrad(nat.ptr(gp.buf), nat.ptr(gp.info), nat.ptr(rot[0]), nat.ptr(wn[0:1]), None, None, nat.ptr(zpx.buf),
                                          nat.ptr(out.buf), nat.ptr(o32), nat.ptr(out.info), nat.ptr(gbb), B, cin, cout, S, nat.ptr(bufs[2]), st()))
        return px_value(gp) * float(gp.info[1].item()), gb, gw, px_value(out) * float(out.info[1].item()), o32, gbb

    runs = {
        "bias_mish_bwd": ([cout * 128 * 4], bias_mish),
        "wgrad": ([int(L.tron_conv3x3_wgrad_workspace(cin, cout))], wgrad),
        "dgrad": ([max(16, int(L.tron_conv3x3_workspace(cout, cin)))], dgrad),
        "dgrad_mish": ([int(L.tron_conv3x3_dgrad_mish_workspace(B, cin, cout, S))], dgrad_mish),
        "px chain": ([int(L.tron_px16_grad_workspace(B, cout)), int(L.tron_conv3x3_wgrad_px16_workspace(B, cin, cout, S)),
                      int(L.tron_conv3x3_ws_dgrad_workspace(cin, cout))], px_chain),
    }
    assert all(n > 0 for sizes, _ in runs.values() for n in sizes)
    return runs


def _zeroed(sizes):
    return [torch.zeros(n, dtype=torch.uint8, device="cuda") for n in sizes]


@pytest.mark.parametrize("S,B,cin,cout", [(12, 37, 32, 64), (12, 37, 64, 64), (26, 3, 64, 64)])
def test_one_workspace_for_a_large_then_a_small_gradient_then_zeros(fused, nat, S, B, cin, cout):
    """A gradient of size 1, the same data 2^-20, zeros, all through ONE scratch / workspace allocation per entry point: the small
    gradient's result equals the result on a freshly zeroed allocation bit for bit (a maximum left over from the large one would
    cost 20 bits), and zeros give zeros."""
    g = _uniform((B, cout, S, S), S + B)
    small = g * 2.0 ** -20
    for name, (sizes, run) in _abi_runs(fused, nat, S, B, cin, cout).items():
        bufs = _zeroed(sizes)
        big = run(g, bufs)
        again = run(small, bufs)
        fresh = run(small, _zeroed(sizes))
        assert all(torch.equal(a, b) for a, b in zip(again, fresh)), name
        assert all(t.abs().max().item() > 0.0 for t in big + fresh), name
        assert all(torch.count_nonzero(t).item() == 0 for t in run(torch.zeros_like(g), bufs)), name


def _pool_conv7(nat, x, w, b, gy, saved, ws):
    L = nat.lib()
    B, side = x.shape[0], x.shape[-1]
    o = (side // 2 + 1) // 2
    pre, y = torch.empty(B, o * o, 64, device="cuda"), torch.empty(B, 64 * o * o, device="cuda")
    st = nat.stream_ptr()
    nat.check(L.tron_pool_conv7_fwd(nat.ptr(x), B, side, nat.ptr(w), nat.ptr(b), nat.ptr(saved), nat.ptr(pre), nat.ptr(y), nat.ptr(ws), st))
    gx, gw, gb = torch.empty_like(x), torch.empty_like(w), torch.empty(64, device="cuda")
    nat.check(L.tron_pool_conv7_bwd(nat.ptr(gy), nat.ptr(pre), nat.ptr(saved), nat.ptr(w), B, side, nat.ptr(gx), nat.ptr(gw), nat.ptr(gb),
                                    nat.ptr(ws), st))
    return gx, gw, gb


def test_pool_conv7_one_workspace_for_a_large_then_a_small_gradient_then_zeros(nat):
    L = nat.lib()
    B, side, o = 3, 26, 7
    x, w, b = _randn((B, 64, side, side), 1, 1.5), _randn((64, 64, 7, 7), 2, 0.02), _randn((64,), 3, 0.1)
    gy = _uniform((B, 64 * o * o), 4)
    sizes = [int(L.tron_pool_conv7_saved_bytes(B, side)), int(L.tron_pool_conv7_workspace(B, side))]
    bufs = _zeroed(sizes)
    big = _pool_conv7(nat, x, w, b, gy, *bufs)
    again = _pool_conv7(nat, x, w, b, gy * 2.0 ** -20, *bufs)
    fresh = _pool_conv7(nat, x, w, b, gy * 2.0 ** -20, *_zeroed(sizes))
    assert all(torch.equal(a, c) for a, c in zip(again, fresh))
    assert all(t.abs().max().item() > 0.0 for t in big + fresh)
    assert all(torch.count_nonzero(t).item() == 0 for t in _pool_conv7(nat, x, w, b, torch.zeros_like(gy), *bufs))


def _with_maximum(shape, m, seed):
    """uniform(-1, 1) m with the last entry exactly m: max |g| == m (|u m| <= m after rounding)."""
    g = _uniform(shape, seed) * m
    g.view(-1)[-1] = -m
    assert g.abs().max().item() == float(np.float32(m))
    return g


def _f32_entries(fused, S, B, cin, cout, g, seed):
    """(name, output, float64 reference, tolerance) of the f32-gradient entry points on g, scaled by the pre-pass and by
    per-image maxima."""
    x = _randn((B, cin, S, S), seed)
    w = _randn((cout, cin, 3, 3), seed + 1, 0.1)
    z = _randn((B, cin, S, S), seed + 2, 2.0)
    am = g.abs().reshape(B, -1).amax(1).contiguous()
    dg = _dgrad64(g, w, cin)
    return [("wgrad pre-pass", lambda: fused.conv3x3_wgrad(x, g, None), _wgrad64(x, g), 2e-6),
            ("wgrad records", lambda: fused.conv3x3_wgrad(x, g, am), _wgrad64(x, g), 2e-6),
            ("dgrad", lambda: fused.conv3x3_dgrad(g, w, am), dg, 2e-6),
            ("dgrad_mish", lambda: fused.conv3x3_dgrad_mish(g, w, am, z, None)[0], _mish_bwd64(z, dg), 3e-6)]


EDGES = [(k, below) for k in (0, -20, 7) for below in (False, True)]


@pytest.mark.parametrize("k,below", EDGES)
@pytest.mark.parametrize("S,B,cin,cout", [(12, 37, 32, 64), (26, 3, 64, 64)])
def test_maximum_on_the_edge_of_the_interval(fused, S, B, cin, cout, k, below):
    """max |g| = 2^k exactly (scaled to 2^13, the closed end) and the float below it (the largest value under 2^14): float64
    agreement at the neighbours' tolerances through the f32 entry points and through the PX16 chain."""
    m = np.float32(2.0 ** k)
    m = np.nextafter(m, np.float32(0), dtype=np.float32) if below else m
    g = _with_maximum((B, cout, S, S), float(m), S + B + k)
    for name, run, ref, tol in _f32_entries(fused, S, B, cin, cout, g, S + k):
        _held(run(), ref, tol, f"{name} max {m!r}")
    z = _randn((B, cout, S, S), S + k + 5, 3.0)
    z.view(-1)[-1] = 3.0
    zpx, xpx = _to_px(fused, z), _to_px(fused, _randn((B, cin, S, S), S + k + 6, 1.5))
    gp, gb = fused.grad_px_from_f32(g, zpx)
    assert gp.info[0].item() == G.absmax_pow2(m, 14)
    val = _entry_checks(gp, gb, _mish_bwd64(px_value(zpx), g), cout, 2e-6, f"grad entry max {m!r}", (B - 1,))
    _held(fused.conv3x3_wgrad_px(xpx, gp), _wgrad64(px_value(xpx), val), 3e-6, f"wgrad_px max {m!r}")


@pytest.mark.parametrize("m", [2.0 ** -99, 2.0 ** 99, 2.0 ** -101, float(np.nextafter(np.float32(2.0 ** 100), np.float32(0))),
                               2.0 ** 100, 2.0 ** 115])
@pytest.mark.parametrize("S,B,cin,cout", [(12, 37, 32, 64), (26, 3, 64, 64)])
def test_maxima_at_the_ends_of_the_scaled_range(fused, S, B, cin, cout, m):
    """2^-99 and 2^99, 2^-101 = 0.5 2^-100 (the smallest maximum absmax_scale scales), both sides of 2^100 (where the scaled
    range once ended) and 2^115 (as large as the sums over a batch stay finite in f32) are held to float64 like any other gradient."""
    g = _with_maximum((B, cout, S, S), m, S + B)
    for name, run, ref, tol in _f32_entries(fused, S, B, cin, cout, g, S + 1):
        _held(run(), ref, tol, f"{name} max {m!r}")


@pytest.mark.parametrize("m", [2.0 ** -102, 2.0 ** 100])
@pytest.mark.parametrize("S,B,cin,cout", [(12, 37, 32, 64), (26, 3, 64, 64)])
def test_maxima_beyond_the_scaled_range_fall_back(fused, S, B, cin, cout, m):
    """One exponent beyond 2^-101 and 2^99: finite and the same bits twice.  At 2^-102 each kernel takes its own fallback
    (tron_f16x3.hpp) and the gradient flushes to zero in f16.  At 2^100 the fallback used to apply as well: the gradient went
    into split() unscaled, f16(2^100 u) was inf, lo = (v - inf) 2^11 was -inf, and every entry point returned NaN throughout
    (inf - inf in the MFMA sums) — this test found it; absmax_scale and k_conv3x3_f16's copy now scale every finite maximum, so
    this case is finite because it is right (test_maxima_at_the_ends_of_the_scaled_range holds it to float64)."""
    g = _with_maximum((B, cout, S, S), m, S + B)
    for name, run, _, _ in _f32_entries(fused, S, B, cin, cout, g, S + 1):
        a, b = run(), run()
        assert bool(torch.isfinite(a).all()), f"{name} max {m!r}: not finite"
        assert torch.equal(a, b), f"{name} max {m!r}"
