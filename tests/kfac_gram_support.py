"""What the tests of csrc/tron_kfac.hip's Gram kernels share (tests/test_gpu_kfac_gram.py, tests/test_kfac_gram_model_cpu.py):
the host plan of the file written out again in Python, float64 references of the factor and of the
three-term split-f16 product the kernels define, the condition under which that product is exact in f32 whatever the order of
the additions, the inputs, and the one table of cases both test files run.  A plain module, imported by name; nothing here
needs a GPU.

Why "exact": an operand value enters the matrix unit as u = x * in_scale / 64 = hi + lo 2^-11 (two f16).  With the inputs built
here every hi and lo is a small multiple of a power of two, every product hi hi', hi lo' 2^-11 is a multiple of one common
unit, and while the sum of the products' magnitudes over all rows stays below 2^24 units (exact_condition) every partial sum —
inside an MFMA, across K chunks, across passes (`+=` into the partial buffer), across splits in k_gram_finish — is an f32
without rounding.  The factor then equals the float64 reference bit for bit, and a power-of-two scale only moves exponents."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from kfac_px_support import EXACT_LIMIT, int_input

# ---- the host plan of csrc/tron_kfac.hip -----------------------------------------------------------------------------------
GRAM_CHUNK_BYTES = 512 << 20                                     # the split transposed operand of one pass
G2_T, G2_K, GK = 128, 32, 64                                     # k_gram2_f16x3's tile and K chunk; the plan's K unit
MAX_D = 8192
NCHW_MAX_SPLITS = 2048
NCHW_GEOMETRY = (1, 1, 0, 1)                                     # a gradient factor: a 1x1 "patch matrix"


def gram_plan(rows_total, rows_unit, d):
    """gram_plan() of csrc/tron_kfac.hip: the padded width, the rows of one pass, the K splits and the workspace bytes."""
    dpad = (d + 63) // 64 * 64
    rows = GRAM_CHUNK_BYTES // (4 * dpad)                         # hi + lo, 2 bytes each
    rows = rows // rows_unit * rows_unit                         # whole images per pass
    if rows < rows_unit:
        rows = rows_unit
    if rows > rows_total:
        rows = (rows_total + rows_unit - 1) // rows_unit * rows_unit
    rows_chunk = (rows + 63) // 64 * 64
    nb2 = (dpad + G2_T - 1) // G2_T
    upper = nb2 * (nb2 + 1) // 2
    ks = 768 // upper
    nk = rows_chunk // GK
    ks = max(min(ks, nk // 16), 1)                               # a split walks at least 16 K chunks of 64
    ks = min(ks, 256)
    x_bytes = dpad * rows_chunk * 2
    partial_bytes = ks * d * dpad * 4
    return dict(dpad=dpad, rows_chunk=rows_chunk, ksplit=ks, x_bytes=x_bytes, partial_bytes=partial_bytes,
                total=2 * x_bytes + partial_bytes + 512)


def out_size(H, W, kh, kw, pad, stride):
    return (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1


def px_supported(B, C, H, W, kh, kw, pad, stride):
    """tron_kfac_px_supported: the shapes tron_kfac_patch_gram hands to the PX kernel (when no in_scale is given)."""
    return (1 <= B < 1 << 30 and (kh, kw, pad, stride) == (3, 3, 1, 1) and H == W and C in (32, 64) and H in (12, 26, 34))


def nchw_geometry(C, kh, kw, pad, stride, per):
    return (kh, kw, pad, stride) == NCHW_GEOMETRY and C in (32, 64) and per % 4 == 0


def nchw_splits(B):
    return min(B, NCHW_MAX_SPLITS)


def patch_workspace(B, C, H, W, kh, kw, pad, stride):
    """tron_kfac_patch_gram_workspace without the PX kernel's share (which can only raise it): the plan's bytes, or
    k_gram_nchw's min(B, 2048) C x C blocks of partial sums where those are more; 0 where the query refuses."""
    if B < 1 or C < 1 or H < 1 or W < 1 or kh < 1 or kw < 1 or pad < 0 or stride < 1:
        return 0
    OH, OW = out_size(H, W, kh, kw, pad, stride)
    if OH < 1 or OW < 1 or C * kh * kw > MAX_D:
        return 0
    per = OH * OW
    need = gram_plan(B * per, per, C * kh * kw)["total"]
    if nchw_geometry(C, kh, kw, pad, stride, per):
        need = max(need, nchw_splits(B) * C * C * 4 + 512)
    return need


def linear_workspace(rows, d):
    return 0 if rows < 1 or d < 1 or d > MAX_D else gram_plan(rows, 64, d)["total"]


def passes(B, per, d, rows_unit=None):
    """[(images, rows_pad)] of every pass of the entry's loop over B images of `per` rows each.  The Linear entry is
    passes(rows, 1, d, rows_unit=64): its "images" are single rows and a pass takes rows_chunk of them."""
    p = gram_plan(B * per, per if rows_unit is None else rows_unit, d)
    imgs = max(p["rows_chunk"] // per, 1)
    return [(min(imgs, B - i), (min(imgs, B - i) * per + 63) // 64 * 64) for i in range(0, B, imgs)]


def k_ranges(rows_pad, ksplit):
    """(k_lo, k_hi) of every split as k_gram2_f16x3 computes them: nk = rows_pad / 32 chunks dealt to ksplit splits."""
    nk = rows_pad // G2_K
    return [(nk * s // ksplit, nk * (s + 1) // ksplit) for s in range(ksplit)]


def which_patch_kernel(C, H, W, kh, kw, pad, stride):
    """The kernel that writes the split operand for this geometry: the plane kernel needs rows per image % 4 == 0 and a
    padded plane of at most 48 KB."""
    OH, OW = out_size(H, W, kh, kw, pad, stride)
    return "k_patches_t_plane" if (OH * OW) % 4 == 0 and (H + 2 * pad) * (W + 2 * pad) * 4 <= 48 * 1024 else "k_patches_t"


def spill_batch(C, H, W, kh, kw, pad, stride):
    """The smallest batch whose patch matrix spills into a second pass: one image more than a pass takes."""
    OH, OW = out_size(H, W, kh, kw, pad, stride)
    per, d = OH * OW, C * kh * kw
    return max(gram_plan(1 << 40, per, d)["rows_chunk"] // per, 1) + 1


def linear_spill(tail=1):
    """(rows, d) of the Linear entry's multi-pass case: rows_chunk + tail rows at the d whose input is smallest."""
    d = min(range(1, 130), key=lambda d: gram_plan(1 << 40, 64, d)["rows_chunk"] * d)
    return gram_plan(1 << 40, 64, d)["rows_chunk"] + tail, d


def uneven_split_rows(d, least=3):
    """The fewest rows of a single pass with ksplit >= least whose K chunks do not divide evenly among the splits."""
    rows = 1
    while True:
        p = gram_plan(rows, 64, d)
        if p["ksplit"] >= least and ((rows + 63) // 64 * 64 // G2_K) % p["ksplit"]:
            return rows
        rows += 1


# ---- references ------------------------------------------------------------------------------------------------------------
def _row_chunks(x, geometry=None, limit=1 << 24):
    """x as the rows of the matrix whose Gram the entry computes, float64 [n, d] pieces of at most `limit` elements: a 2-D
    input's own rows, a patch geometry's F.unfold rows (zero padded), an NCHW gradient's (image, position) rows."""
    if x.dim() == 2:
        step = max(1, limit // x.shape[1])
        for i in range(0, x.shape[0], step):
            yield x[i:i + step].double()
        return
    B, C, H, W = x.shape
    kh, kw, pad, stride = geometry
    OH, OW = out_size(H, W, kh, kw, pad, stride)
    d = C * kh * kw
    step = max(1, limit // (d * OH * OW))
    for i in range(0, B, step):
        xc = x[i:i + step].double()
        if tuple(geometry) == NCHW_GEOMETRY:
            yield xc.permute(0, 2, 3, 1).reshape(-1, C)          # == xc.permute(1, 0, 2, 3).reshape(C, -1).t()
        else:
            yield F.unfold(xc, (kh, kw), padding=pad, stride=stride).transpose(1, 2).reshape(-1, d)


def ref_gram(x, scale, geometry=None):
    """scale * P^T P in float64 on x's device, P = x's rows (see _row_chunks)."""
    A = None
    for P in _row_chunks(x, geometry):
        A = P.t() @ P if A is None else A + P.t() @ P
    return A * scale


def split_model(v):
    """tron_f16x3.hpp::split on a float32 tensor: hi = f16(v), lo = f16((v - hi) * 2^11), both round-to-nearest-even."""
    assert v.dtype == torch.float32
    hi = v.to(torch.float16)
    lo = ((v - hi.float()) * 2048.0).to(torch.float16)
    return hi, lo


def operand(x, in_scale=None):
    """(hi, lo) of what the kernels feed the matrix unit: x * (in_scale / 64) in f32, split."""
    sc = (1.0 if in_scale is None else float(in_scale)) / 64.0
    return split_model(x.float() * sc)


def ref_gram_three_term(x, scale, in_scale=None, geometry=None, terms=3):
    """The product the kernels define, in float64: (sum hi hi' + (sum hi lo' + lo hi') 2^-11) * 4096 * scale / in_scale^2 —
    no lo lo' term, by design.  terms = 1 keeps the hi halves only."""
    hi, lo = operand(x, in_scale)
    A = None
    for H, L in zip(_row_chunks(hi, geometry), _row_chunks(lo, geometry)):
        part = H.t() @ H
        if terms == 3:
            part = part + (H.t() @ L + L.t() @ H) * 2.0 ** -11
        A = part if A is None else A + part
    return A * (4096.0 * scale / (1.0 if in_scale is None else float(in_scale)) ** 2)


def _low_bit(t):
    """The smallest set bit over the nonzero entries of an f16 tensor, in units of 2^-24 (f16's smallest subnormal); None if
    all are zero."""
    k = (t.reshape(-1).double() * 2.0 ** 24).to(torch.int64).abs()
    k = k[k > 0]
    return int((k & -k).min().item()) if k.numel() else None


def exact_condition(x, in_scale=None, geometry=None):
    """The largest numerator any partial sum of the three-term product can reach, in units of the smallest bit present.
    From the data: with (hi, lo) = operand(x), bh and bl the smallest set bits among the hi and lo entries, every product
    hi hi' is a multiple of bh^2 and every hi lo' 2^-11 of bh bl 2^-11; a partial sum — any subset of the rows, any
    signs — is a multiple of the smaller of the two and at most
        max over (i, j) of  sum_r |hi_ri| |hi_rj| + (|hi_ri| |lo_rj| + |lo_ri| |hi_rj|) 2^-11.
    Below EXACT_LIMIT = 2^24 of those units every partial sum is an f32.  Where every lo is zero the maximum sits on the
    diagonal (Cauchy-Schwarz: sum |a| |b| <= max(sum a^2, sum b^2)), so the column sums of hi^2 are enough.  Walks x in
    pieces of whole images (rows) of about 2^22 entries."""
    step = max(1, (1 << 22) // max(x[0].numel(), 1))
    bh = bl = S = D = None
    least = lambda a, b: b if a is None else a if b is None else min(a, b)
    for i in range(0, x.shape[0], step):
        hi, lo = operand(x[i:i + step], in_scale)
        bh, bl = least(bh, _low_bit(hi)), least(bl, _low_bit(lo))
        for H in _row_chunks(hi, geometry):
            D = (H * H).sum(0) if D is None else D + (H * H).sum(0)
        if bl is not None:                                               # (the lo family's inputs are small: full matrices)
            for H, L in zip(_row_chunks(hi.abs(), geometry), _row_chunks(lo.abs(), geometry)):
                part = H.t() @ H + (H.t() @ L + L.t() @ H) * 2.0 ** -11
                S = part if S is None else S + part
    if bh is None:
        return 0
    if bl is None:
        unit, top = bh * bh * 2048, float(D.max().item())                # (units of 2^-59)
    else:
        assert x.shape[0] <= step, "a lo-carrying input of more than one piece"
        unit, top = min(bh * bh * 2048, bh * bl), float(S.max().item())
    return int(math.ceil(top * 2.0 ** 59 / unit))


def describe_gram_diff(got, want, geometry=None, limit=12):
    """The first entries where two factors differ: (row, col), the 128 x 128 tile of k_gram2_f16x3 they sit in and, for a patch
    geometry, the (channel, ky, kx) of row and column."""
    bad = (got != want).nonzero().tolist()
    lines = [f"{len(bad)} of {got.numel()} entries differ"]
    for r, c in bad[:limit]:
        where = f"  [{r}][{c}] tile ({r // G2_T}, {c // G2_T})"
        if geometry is not None:
            kh, kw = geometry[0], geometry[1]
            name = lambda j: f"(c={j // (kh * kw)} ky={j % (kh * kw) // kw} kx={j % kw})"
            where += f" {name(r)} x {name(c)}"
        lines.append(f"{where}: got {got[r, c].item()!r}, want {want[r, c].item()!r}")
    return "\n".join(lines)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
TILE_ABOVE, TILE_PERIOD = 1 << 24, 61


def ints(shape, nonneg, seed, device="cpu"):
    """kfac_px_support.int_input for any shape: {-2 .. 2} or {0, 1, 2}, a third zeros.  A tensor of more than 2^24 entries
    repeats TILE_PERIOD = 61 seeded images in turn (image b = base[b % 61]): 61 is prime to every split and pass count, so an
    image dealt to the wrong split or dropped still changes the sums, and the big batches cost no host time."""
    shape = tuple(shape)
    if math.prod(shape) > TILE_ABOVE and shape[0] > TILE_PERIOD:
        base = ints((TILE_PERIOD,) + shape[1:], nonneg, seed, device)
        return base[torch.arange(shape[0], device=device) % TILE_PERIOD].contiguous()
    return int_input(shape[0], math.prod(shape[1:]), 1, nonneg, seed, device).reshape(shape)


def lo_input(shape, seed, density=0.5, device="cpu"):
    """The lo-carrying family: entries 64 h + m 2^-6, h in {+-1, +-2}, m in {+-1}, present with probability `density`, else 0.
    x / 64 = h + m 2^-12 is within half an f16 ulp of h (strictly, except 1 - 2^-12 and -1 + 2^-12, which sit midway between
    h and its odd neighbour and round to the even h), so hi = h and lo = f16(m 2^-12 2^11) = m / 2: acc0 holds integers, acc1
    half-integers, and acc0 + acc1 2^-11 spans 2^-12 up to sum |h h'| — exact while that sum stays below 2^12, which the
    density decides and exact_condition checks."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    h = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, shape, generator=g)]
    m = torch.randint(0, 2, shape, generator=g).float() * 2.0 - 1.0
    keep = (torch.rand(shape, generator=g) < density).float()
    return ((64.0 * h + m * 2.0 ** -6) * keep).to(device)


def lo_parts(x):
    """(h, m) of a lo_input tensor, recovered from its values."""
    h = torch.round(x / 64.0)
    return h, (x - 64.0 * h) * 64.0


# ---- the cases -------------------------------------------------------------------------------------------------------------
# kind "linear": shape (rows, d) through tron_kfac_gram; kind "patch": shape (B, C, H, W) with geometry (kh, kw, pad, stride)
# through tron_kfac_patch_gram.  The input is family(shape, seed) * 2^-k; in_scale is None, a float, or "pow2" (the scale
# Net/kfac.py::_pow2_scale finds on the device, see pow2_scale_model).
Case = namedtuple("Case", "group name kind shape geometry family seed k in_scale scale")


def build_input(case, device="cpu"):
    if case.family == "lo":
        x = lo_input(case.shape, case.seed, device=device)
    else:
        x = ints(case.shape, case.family == "nonneg", case.seed, device)
    return x * 2.0 ** -case.k if case.k else x


def pow2_scale_model(x):
    """Net/kfac.py::_pow2_scale: the power of two that brings max |x| = f 2^e, f in [0.5, 1), to f 2^16; 1 for zeros."""
    m = float(x.abs().max().item())
    return 2.0 ** (16 - math.frexp(m)[1]) if m > 0 else 1.0


def in_scale_of(case, x):
    return pow2_scale_model(x) if case.in_scale == "pow2" else case.in_scale


LINEAR_D = (1, 27, 63, 64, 65, 127, 128, 129, 192, 257)
LINEAR_ROWS = (1, 31, 32, 33, 63, 64, 65, 1000)
CONV1_12, CONV1_34 = ((3, 12, 12), (3, 3, 1, 1)), ((4, 34, 34), (3, 3, 1, 1))
CONV7_17, CONV7_15 = ((64, 17, 17), (7, 7, 3, 2)), ((64, 15, 15), (7, 7, 3, 2))
ODD_9x11, SIDE_13 = ((5, 9, 11), (3, 3, 0, 1)), ((32, 13, 13), (3, 3, 1, 1))
PATCH_GEOMETRIES = (CONV1_12, CONV1_34, CONV7_17, CONV7_15, ODD_9x11, SIDE_13)
PATCH_BATCHES = (1, 2, 7)
NCHW_C, NCHW_PER, NCHW_B = (32, 64), (4, 16, 36, 144, 676), (1, 2, 3, 2047, 2048, 2049, 4099)
NCHW_SIDES = {4: (2, 2), 16: (4, 4), 36: (6, 6), 144: (12, 12), 676: (26, 26)}
NCHW_K = 17                                                     # gradient-sized inputs: integers * 2^-17


def _cases():
    out = []
    add = lambda *a: out.append(Case(*a))
    for d in LINEAR_D:
        for rows in LINEAR_ROWS:
            add("linear", f"rows{rows}-d{d}-s1", "linear", (rows, d), None, "int", 7 * rows + d, 0, None, 1.0)
            add("linear", f"rows{rows}-d{d}-s2^-10", "linear", (rows, d), None, "nonneg", 7 * rows + d + 1, 0, None, 2.0 ** -10)
    add("linear_split", "uneven", "linear", (uneven_split_rows(64), 64), None, "int", 64, 0, None, 1.0)
    for k in (-20, 0, 12):
        add("linear_in_scale", f"k{k}", "linear", (1000, 129), None, "int", 300 + k, k, 2.0 ** k, 2.0 ** -10)
    for (chw, geo) in PATCH_GEOMETRIES:
        for B in PATCH_BATCHES:
            name = "x".join(map(str, chw)) + f"-B{B}"
            add("patch", name + "-int", "patch", (B,) + chw, geo, "int", 31 * B + chw[0] + chw[1], 0, None, 1.0)
            add("patch", name + "-nonneg", "patch", (B,) + chw, geo, "nonneg", 31 * B + chw[0] + chw[2], 0, None, 2.0 ** -10)
    # multi-pass: one image (one row) more than a pass takes; the last two put a one-image last pass behind 256 splits
    for chw, geo in (CONV7_17, CONV7_15, CONV1_12, ODD_9x11):
        B = spill_batch(*chw, *geo)
        add("multipass", "x".join(map(str, chw)), "patch", (B,) + chw, geo, "nonneg", B, 0, None, 1.0)
    add("multipass", "linear-tail1", "linear", linear_spill(1), None, "int", 1, 0, None, 1.0)
    add("multipass", "linear-d3-tail20000", "linear", (gram_plan(1 << 40, 64, 3)["rows_chunk"] + 20000, 3), None, "int", 3, 0, None, 1.0)
    for C in NCHW_C:
        for per in NCHW_PER:
            for B in NCHW_B:
                for in_scale in ("pow2", 2.0 ** NCHW_K):
                    tag = "pow2" if in_scale == "pow2" else "hand"
                    add("nchw", f"C{C}-per{per}-B{B}-{tag}", "patch", (B, C) + NCHW_SIDES[per], NCHW_GEOMETRY,
                        "nonneg" if tag == "pow2" else "int", C + per + B, NCHW_K, in_scale, 2.0 ** -3)
    add("nchw_offset", "C32-per36-B3", "patch", (3, 32, 6, 6), NCHW_GEOMETRY, "int", 5, NCHW_K, 2.0 ** NCHW_K, 1.0)
    add("lo", "linear", "linear", (1000, 129), None, "lo", 11, 0, None, 1.0)
    add("lo", "conv1", "patch", (7, 3, 12, 12), (3, 3, 1, 1), "lo", 12, 0, None, 1.0)
    add("lo", "odd", "patch", (7, 5, 9, 11), (3, 3, 0, 1), "lo", 13, 0, None, 2.0 ** -10)
    add("lo", "nchw", "patch", (7, 64, 12, 12), NCHW_GEOMETRY, "lo", 14, 0, None, 1.0)
    add("workspace", "plane-d27", "patch", (5, 3, 12, 12), (3, 3, 1, 1), "int", 21, 0, None, 1.0)
    add("workspace", "patches_t", "patch", (5, 5, 9, 11), (3, 3, 0, 1), "int", 22, 0, None, 1.0)
    add("workspace", "linear", "linear", (100, 27), None, "int", 23, 0, None, 1.0)
    return out


CASES = _cases()


def cases(group):
    return [c for c in CASES if c.group == group]
