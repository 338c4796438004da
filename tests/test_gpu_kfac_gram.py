"""GPU tests of the Gram kernels of csrc/tron_kfac.hip that the PX16 kernel does not take — k_patches_t, k_patches_t_plane,
k_transpose_split, k_gram2_f16x3, k_gram_nchw, k_gram_finish — through the C ABI (tron_kfac_gram, tron_kfac_patch_gram) with a
workspace of exactly the queried size.

Every comparison is bit equality against a float64 reference (kfac_gram_support: why the inputs make the kernels' f32 sums
exact, and the condition each case asserts first).  Inputs, seeds and shapes come from kfac_gram_support.CASES, the table
tests/test_kfac_gram_model_cpu.py checks without a GPU.  Every call runs with the workspace full of f16 NaN bit patterns and
0xA5 guard bytes behind the workspace and behind the factor; every case is also symmetric bit for bit and gives the same bits
when run again."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from kfac_gram_support import (CONV1_12, CONV1_34, CONV7_15, CONV7_17, EXACT_LIMIT, LINEAR_D, NCHW_C, NCHW_GEOMETRY, NCHW_PER,
                               NCHW_SIDES, ODD_9x11, PATCH_GEOMETRIES, SIDE_13, build_input, cases, describe_gram_diff,
                               exact_condition, gram_plan, in_scale_of, linear_workspace, out_size, passes, patch_workspace,
                               pow2_scale_model, ref_gram, ref_gram_three_term)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


TAIL, GUARD = 1 << 20, 0xA5
NAN_FILL, INF_FILL = 0xFF, 0x7C00                                # bytes 0xFF: f16 / f32 NaN; the f16 pattern of +Inf


def native():
    from Net import fused
    nat = fused.nat                                              # the library binding Net/ calls through
    return nat, nat.lib()


def workspace(need, fill):
    """`need` bytes holding `fill` (a byte, or the 16-bit pattern INF_FILL) and TAIL guard bytes behind them."""
    buf = torch.empty(need + TAIL, dtype=torch.uint8, device="cuda")
    if fill == INF_FILL:
        buf[:need].view(torch.int16).fill_(INF_FILL)
    else:
        buf[:need].fill_(fill)
    buf[need:].fill_(GUARD)
    return buf


def factor_buffer(d, value=None):
    """(the bytes, their first d x d floats as the factor): TAIL guard bytes behind the factor."""
    buf = torch.full((d * d * 4 + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
    gram = buf[:d * d * 4].view(torch.float32).view(d, d)
    if value is not None:
        gram.fill_(value)
    return buf, gram


def guards_intact(ws, need, gbuf, d, what):
    assert bool((ws[need:] == GUARD).all()), f"{what}: wrote past the {need} bytes the size query reserved"
    assert bool((gbuf[d * d * 4:] == GUARD).all()), f"{what}: wrote past the factor"


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device="cuda")


def call_linear(a, scale, in_scale=None, fill=NAN_FILL):
    nat, L = native()
    rows, d = a.shape
    need = int(L.tron_kfac_gram_workspace(rows, d))
    assert need == linear_workspace(rows, d) > 0
    ws, (gbuf, gram), sc = workspace(need, fill), factor_buffer(d), scalar(in_scale)
    rc = L.tron_kfac_gram(nat.ptr(a), rows, d, scale, nat.ptr(sc), nat.ptr(gram), nat.ptr(ws), nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == nat.OK, rc
    guards_intact(ws, need, gbuf, d, f"tron_kfac_gram rows={rows} d={d}")
    return gram


def call_patch(x, geometry, scale, in_scale=None, fill=NAN_FILL, x_ptr=None):
    nat, L = native()
    B, C, H, W = x.shape
    d = C * geometry[0] * geometry[1]
    need = int(L.tron_kfac_patch_gram_workspace(B, C, H, W, *geometry))
    assert need == patch_workspace(B, C, H, W, *geometry) > 0
    ws, (gbuf, gram), sc = workspace(need, fill), factor_buffer(d), scalar(in_scale)
    rc = L.tron_kfac_patch_gram(nat.ptr(x) if x_ptr is None else x_ptr, B, C, H, W, *geometry, scale, nat.ptr(sc), nat.ptr(gram),
                                nat.ptr(ws), nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == nat.OK, rc
    guards_intact(ws, need, gbuf, d, f"tron_kfac_patch_gram {tuple(x.shape)} {geometry}")
    return gram


def call(case, x, in_scale, fill=NAN_FILL):
    if case.kind == "linear":
        return call_linear(x, case.scale, in_scale, fill)
    return call_patch(x, case.geometry, case.scale, in_scale, fill)


def assert_exact(case, x=None, want=None):
    """The entry == the float64 reference bit for bit, symmetric, and the same bits when run again; returns the factor."""
    x = build_input(case, "cuda") if x is None else x
    in_scale = in_scale_of(case, x)
    top = exact_condition(x, in_scale, case.geometry)
    assert top < EXACT_LIMIT, f"{case.group}/{case.name}: numerator {top}: use smaller or sparser data"
    if want is None:
        want = (ref_gram_three_term(x, case.scale, in_scale, case.geometry) if case.family == "lo" else ref_gram(x, case.scale, case.geometry))
    got = call(case, x, in_scale)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.double(), want), f"{case.group}/{case.name}: {describe_gram_diff(got.double(), want, case.geometry)}"
    assert torch.equal(got, got.t()), f"{case.group}/{case.name}: not symmetric"
    assert torch.equal(got, call(case, x, in_scale)), f"{case.group}/{case.name}: a second run gave other bits"
    return got


# ---- the Linear entry: k_transpose_split + k_gram2_f16x3 + k_gram_finish ---------------------------------------------------
@pytest.mark.parametrize("d", LINEAR_D)
def test_linear_entry_is_exact_on_integers(d):
    """rows 1 .. 1000 at this width, {-2 .. 2} with scale 1 and {0, 1, 2} with scale 2^-10: a ragged 64 (d = 1, 27, 63), both
    halves of a 128 tile (64, 65, 127, 128), a clamped second tile row with the diagonal and an off-diagonal tile (129, 192,
    257: nb = 2, 2, 3), K padding of 63 .. 0 rows."""
    mine = [c for c in cases("linear") if c.shape[1] == d]
    assert len(mine) == 16
    for c in mine:
        assert_exact(c)


def test_linear_entry_with_uneven_k_splits():
    """d = 64 at the fewest rows with three splits whose ranges differ in length (kfac_gram_support.uneven_split_rows)."""
    (c,) = cases("linear_split")
    p = gram_plan(*c.shape[:1], 64, c.shape[1])
    assert p["ksplit"] >= 3 and ((c.shape[0] + 63) // 64 * 2) % p["ksplit"]
    assert_exact(c)


@pytest.mark.parametrize("case", cases("linear_in_scale"), ids=lambda c: c.name)
def test_linear_entry_with_a_power_of_two_in_scale(case):
    """integers * 2^-k with in_scale = 2^k: the operand is the integers' again, and k_gram_finish's scale / in_scale^2 only moves
    the exponent — the factor is that of the scaled input, exactly."""
    got = assert_exact(case)
    assert got.abs().max().item() > 0


# ---- the patch entry off the PX path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw,geometry", PATCH_GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_patch_entry_is_exact_on_integers(chw, geometry):
    """B = 1, 2, 7 of {-2 .. 2} (scale 1) and {0, 1, 2} (scale 2^-10): conv1's 3 and 4 channels (plane kernel, d = 27 and 36),
    conv7 at 17x17 (k_patches_t, d = 3136) and at 15x15 (plane kernel with a stride), 5 x 9 x 11 without padding and a
    32-channel 13x13 board (k_patches_t)."""
    mine = [c for c in cases("patch") if c.shape[1:] == chw and c.geometry == geometry]
    assert len(mine) == 6
    for c in mine:
        assert_exact(c)


def impulse_factor(C, H, W, geometry, c, y, x):
    """The factor of a single 1 at pixel (y, x) of channel c: output position (oy, ox) sees it through tap (ky, kx) where
    oy stride - pad + ky = y and ox stride - pad + kx = x; a tap belongs to at most one position and a position to one tap, so
    the factor is ones on the diagonal at c kh kw + ky kw + kx for the taps whose position exists."""
    kh, kw, pad, stride = geometry
    oh, ow = out_size(H, W, *geometry)
    want = torch.zeros(C * kh * kw, C * kh * kw, dtype=torch.float64, device="cuda")
    for ky in range(kh):
        for kx in range(kw):
            ty, tx = y + pad - ky, x + pad - kx
            if ty % stride == 0 and tx % stride == 0 and 0 <= ty // stride < oh and 0 <= tx // stride < ow:
                want[c * kh * kw + ky * kw + kx, c * kh * kw + ky * kw + kx] = 1.0
    return want


@pytest.mark.parametrize("chw,geometry", PATCH_GEOMETRIES, ids=lambda v: "x".join(map(str, v)))
def test_patch_impulses_name_the_tap(chw, geometry):
    """Three images, a single 1: at the corner pixel of the first image's first channel, at an edge pixel of it, and at the
    last pixel of the last channel of the last image.  The expected factor is written down without unfold (and unfold agrees);
    a wrong halo, stride or K padding shows as the (channel, ky, kx) entries that differ."""
    from kfac_gram_support import Case
    C, H, W = chw
    for img, c, y, x in ((0, 0, 0, 0), (0, 0, H // 2, W - 1), (2, C - 1, H - 1, W - 1)):
        inp = torch.zeros(3, C, H, W, device="cuda")
        inp[img, c, y, x] = 1.0
        want = impulse_factor(C, H, W, geometry, c, y, x)
        assert want.sum().item() >= 1 and torch.equal(ref_gram(inp, 1.0, geometry), want)
        assert_exact(Case("impulse", f"{chw} at {(img, c, y, x)}", "patch", (3,) + chw, geometry, "int", 0, 0, None, 1.0), inp, want)
    assert impulse_factor(64, 17, 17, (7, 7, 3, 2), 0, 0, 0).sum().item() == 4      # taps (3, 3), (3, 1), (1, 3), (1, 1): even offsets
    assert impulse_factor(3, 12, 12, (3, 3, 1, 1), 0, 0, 0).sum().item() == 4


# ---- more than one pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases("multipass"), ids=lambda c: c.name)
def test_second_pass_adds_to_the_first(case):
    """One image (or one row, or 20 000) more than a pass takes: the loop over passes, the `+=` into the partial sums of the
    first pass, a short last pass whose K chunks leave splits empty or with one, two or three chunks
    (test_kfac_gram_model_cpu.py::test_multipass_cases_sit_on_their_edges says which case has which).  Exact against float64,
    and the whole == the first pass alone + the tail alone, bit for bit: every sum is an integer below 2^24."""
    x = build_input(case, "cuda")
    if case.kind == "linear":
        first = passes(case.shape[0], 1, case.shape[1], rows_unit=64)[0][0]
    else:
        oh, ow = out_size(*case.shape[2:], *case.geometry)
        first = passes(case.shape[0], oh * ow, case.shape[1] * case.geometry[0] * case.geometry[1])[0][0]
    assert 0 < first < case.shape[0]
    whole = assert_exact(case, x)
    head, tail = call(case, x[:first], None), call(case, x[first:], None)
    assert tail.abs().max().item() > 0, "the tail is all zeros: it proves nothing"
    assert torch.equal(whole, head + tail), describe_gram_diff(whole, head + tail, case.geometry)


# ---- k_gram_nchw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", NCHW_PER)
@pytest.mark.parametrize("C", NCHW_C)
def test_gradient_factor_is_exact_on_integers(C, per):
    """integers * 2^-17 in an NCHW tensor of `per` positions an image — a slab shorter than 32, one slab, two with a ragged
    tail, many — at B = 1, 2, 3 and on both sides of the 2048-split cap (2047, 2048, 2049, 4099: uneven B s / nsplit), with the
    in_scale Net/kfac.py::_pow2_scale finds on the device ({0, 1, 2}) and with the hand-made 2^17 ({-2 .. 2})."""
    from Net import kfac
    mine = [c for c in cases("nchw") if c.shape[1] == C and c.shape[2:] == NCHW_SIDES[per]]
    assert len(mine) == 14
    for c in mine:
        x = build_input(c, "cuda")
        if c.in_scale == "pow2":
            assert kfac._pow2_scale(x).item() == pow2_scale_model(x) == 2.0 ** (15 + 17 - 1)
        assert_exact(c, x)


@pytest.mark.parametrize("C", NCHW_C)
def test_gradient_factor_impulses(C):
    """A single 1 at the last position of the last image in channel C - 1; and, across a slab edge, ones at position 31 in
    channels 0 and C - 1 and at position 32 in channels 1 and C - 1: G[0][C-1] = G[1][C-1] = 1 with their mirrors, G[0][1] = 0
    (the two positions share no sum), G[C-1][C-1] = 2."""
    from kfac_gram_support import Case
    for side in (6, 12):
        shape = (3, C, side, side)
        case = Case("impulse", f"nchw C={C} side={side}", "patch", shape, NCHW_GEOMETRY, "int", 0, 0, None, 1.0)
        g = torch.zeros(shape, device="cuda")
        g.view(3, C, -1)[2, C - 1, side * side - 1] = 1.0
        want = torch.zeros(C, C, dtype=torch.float64, device="cuda")
        want[C - 1, C - 1] = 1.0
        assert_exact(case, g, want)
        g = torch.zeros(shape, device="cuda")
        flat = g.view(3, C, -1)
        flat[1, 0, 31] = flat[1, C - 1, 31] = flat[1, 1, 32] = flat[1, C - 1, 32] = 1.0
        want = torch.zeros(C, C, dtype=torch.float64, device="cuda")
        want[0, 0] = want[1, 1] = want[0, C - 1] = want[C - 1, 0] = want[1, C - 1] = want[C - 1, 1] = 1.0
        want[C - 1, C - 1] = 2.0
        assert torch.equal(ref_gram(g, 1.0, NCHW_GEOMETRY), want)
        assert_exact(case, g, want)


def test_gradient_factor_from_a_misaligned_tensor():
    """An x pointer 4 bytes off a 16-byte boundary cannot take k_gram_nchw's float4 loads: the entry runs the general path
    (k_patches_t_plane as a 1x1 patch matrix), inside the same queried workspace, and gives the aligned call's bits."""
    (c,) = cases("nchw_offset")
    x = build_input(c, "cuda")
    aligned = assert_exact(c, x)
    room = torch.zeros(x.numel() + 4, device="cuda")
    shifted = room[1:1 + x.numel()].view(x.shape)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    got = call_patch(shifted, c.geometry, c.scale, c.in_scale, x_ptr=ctypes.c_void_p(shifted.data_ptr()))
    assert torch.equal(got, aligned), describe_gram_diff(got, aligned)


# ---- the lo half -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases("lo"), ids=lambda c: c.name)
def test_lo_half_is_exact(case):
    """Entries 64 h + m 2^-6 (kfac_gram_support.lo_input): hi = h, lo = m / 2, so the ah bl and al bh products and LO_UNSCALE
    carry half-integers that the factor must show exactly: == ref_gram_three_term bit for bit.  That reference differs from
    the hi-only product at these inputs (dropping a lo MFMA or its 2^-11 cannot pass), and from the true float64 Gram by the
    m m' 2^-24 term the kernels leave out by design."""
    x = build_input(case, "cuda")
    want = ref_gram_three_term(x, case.scale, None, case.geometry)
    hi_only = ref_gram_three_term(x, case.scale, None, case.geometry, terms=1)
    differ = (want != hi_only).float().mean().item()
    assert differ > 0.5, f"only {differ:.2f} of the entries feel the lo half"
    assert not torch.equal(want, ref_gram(x, case.scale, case.geometry))
    assert_exact(case, x, want)


# ---- the workspace contract and the arguments --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases("workspace"), ids=lambda c: c.name)
def test_factor_does_not_depend_on_what_the_workspace_held(case):
    """The workspace full of zeros, of 0xFF (f16 NaN) and of 0x7C00 (f16 +Inf): k_patches_t_plane leaves the operand's rows
    d .. dpad unwritten and k_gram2_f16x3 reads them (its row clamp is dpad - 1), so at d = 27 those rows then hold 37 rows
    of NaN or Inf — what they produce must never land where k_gram_finish reads.  Same finite bits for all three fills, for
    the plane kernel, k_patches_t and the Linear entry; the guard bytes behind workspace and factor stay (call_*)."""
    x = build_input(case, "cuda")
    assert exact_condition(x, None, case.geometry) < EXACT_LIMIT, "use smaller or sparser data"
    want = ref_gram(x, case.scale, case.geometry)
    for fill in (0x00, NAN_FILL, INF_FILL):
        got = call(case, x, None, fill)
        assert bool(torch.isfinite(got).all()), f"fill {fill:#x}"
        assert torch.equal(got.double(), want), f"fill {fill:#x}: {describe_gram_diff(got.double(), want, case.geometry)}"


def test_refused_calls_leave_the_factor_alone_and_empty_inputs_zero_it():
    """NULL or misaligned pointers, stride 0, d > 8192, no output row: BAD_ARG or UNSUPPORTED and nothing launches — the factor
    keeps its fill.  batch = 0 and rows = 0 are sums over nothing: zeros."""
    nat, L = native()
    st = nat.stream_ptr()
    x = torch.ones(4, 3, 12, 12, device="cuda")
    a = torch.ones(100, 27, device="cuda")
    ws = workspace(max(int(L.tron_kfac_patch_gram_workspace(4, 3, 12, 12, 3, 3, 1, 1)), int(L.tron_kfac_gram_workspace(100, 27))), NAN_FILL)
    gbuf, gram = factor_buffer(27, 7.0)
    X, A, G, W = nat.ptr(x), nat.ptr(a), nat.ptr(gram), nat.ptr(ws)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    assert gram.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    geo = (3, 3, 1, 1)
    bad, unsupported = nat.ERR_BAD_ARG, nat.ERR_UNSUPPORTED
    assert L.tron_kfac_patch_gram(None, 4, 3, 12, 12, *geo, 1.0, None, G, W, st) == bad
    assert L.tron_kfac_patch_gram(X, 4, 3, 12, 12, *geo, 1.0, None, None, W, st) == bad
    assert L.tron_kfac_patch_gram(X, 4, 3, 12, 12, *geo, 1.0, None, G, None, st) == bad
    assert L.tron_kfac_patch_gram(X, 4, 3, 12, 12, *geo, 1.0, None, off(gram, 4), W, st) == bad
    assert L.tron_kfac_patch_gram(X, 4, 3, 12, 12, *geo, 1.0, None, G, off(ws, 8), st) == bad
    assert L.tron_kfac_patch_gram(X, 4, 3, 12, 12, 3, 3, 1, 0, 1.0, None, G, W, st) == bad           # stride 0
    assert L.tron_kfac_patch_gram(X, 4, 3, 2, 12, 3, 3, 0, 1, 1.0, None, G, W, st) == bad            # OH = 0
    assert L.tron_kfac_patch_gram(X, -1, 3, 12, 12, *geo, 1.0, None, G, W, st) == bad
    assert L.tron_kfac_patch_gram(X, 4, 1024, 12, 12, *geo, 1.0, None, G, W, st) == unsupported      # d = 9216
    assert L.tron_kfac_gram(None, 100, 27, 1.0, None, G, W, st) == bad
    assert L.tron_kfac_gram(A, 100, 27, 1.0, None, None, W, st) == bad
    assert L.tron_kfac_gram(A, 100, 27, 1.0, None, G, None, st) == bad
    assert L.tron_kfac_gram(A, 100, 27, 1.0, None, off(gram, 4), W, st) == bad
    assert L.tron_kfac_gram(A, 100, 27, 1.0, None, G, off(ws, 8), st) == bad
    assert L.tron_kfac_gram(A, -1, 27, 1.0, None, G, W, st) == bad and L.tron_kfac_gram(A, 100, 0, 1.0, None, G, W, st) == bad
    assert L.tron_kfac_gram(A, 100, 8193, 1.0, None, G, W, st) == unsupported
    torch.cuda.synchronize()
    assert bool((gram == 7.0).all()) and bool((gbuf[27 * 27 * 4:] == GUARD).all())
    assert L.tron_kfac_patch_gram(X, 0, 3, 12, 12, *geo, 1.0, None, G, W, st) == nat.OK
    torch.cuda.synchronize()
    assert torch.count_nonzero(gram).item() == 0 and bool((gbuf[27 * 27 * 4:] == GUARD).all())
    gram.fill_(7.0)
    assert L.tron_kfac_gram(A, 0, 27, 1.0, None, G, W, st) == nat.OK
    torch.cuda.synchronize()
    assert torch.count_nonzero(gram).item() == 0 and bool((gbuf[27 * 27 * 4:] == GUARD).all())
    assert bool((ws[-TAIL:] == GUARD).all())
