"""GPU tests of csrc/tron_kfac_px.hip — K-FAC's input factor of a 3x3 / pad 1 / stride 1 layer from the PX16 window, no patch
matrix — through both of its entries: tron_kfac_patch_gram on an f32 NCHW tensor (kfac._gram_hip) and tron_kfac_gram_px16 on
a PX16 image (PX16.kfac_input_gram).

Most comparisons are exact.  With integer inputs |x| <= 2 the kernel's x / 64 is an f16 with a zero lo half, every product is
a multiple of 2^-12 of at most 4 of them, and a sum of B S^2 products has a numerator below 2^24 while 4 B S^2 < 2^24
(kfac_px_support.exact_bound): every partial sum, in the matrix unit, in a flush and in the finish kernel, is then an f32
without rounding, whatever the order of the additions, and with a power-of-two scale so is the factor.  The reference is
kfac_px_support.ref_factor (F.unfold and a float64 product; tests/test_kfac_px_reference_cpu.py checks it against the
definition), evaluated on the device."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from kfac_px_support import (EXACT_LIMIT, PX_KERNELS, describe_diff, exact_bound, flush_batch, flushes, int_input,
                             least_flush_batches, px_plan, ref_factor)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


SHAPES = sorted(PX_KERNELS)                                      # (C, S): {32, 64} x {12, 26, 34}, the six instantiations
MAX_FLUSH_BATCH = 12000


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def conv_of(C):
    import torch.nn as nn
    return nn.Conv2d(C, 8, 3, padding=1)


def both_entries(x, scale):
    """(tron_kfac_patch_gram on the f32 tensor, tron_kfac_gram_px16 on its PX16 image); neither may decline these shapes."""
    from Net import kfac
    from Net.fused import PX16
    a = kfac._gram_hip(x, conv_of(x.shape[1]), scale)
    b = PX16.from_f32(x).kfac_input_gram(scale)
    assert a is not None and b is not None
    return a, b


def assert_exact(x, scale, want=None):
    """Both entries == ref_factor bit for bit, == each other, symmetric, and the same bits when run again."""
    B, C, S, _ = x.shape
    assert exact_bound(B, S, int(x.abs().max().item())) < EXACT_LIMIT, "the factor of this batch is not exact in f32: use a smaller one"
    want = ref_factor(x, scale) if want is None else want
    a, b = both_entries(x, scale)
    for name, got in (("tron_kfac_patch_gram", a), ("tron_kfac_gram_px16", b)):
        assert got.shape == want.shape and got.dtype == torch.float32
        assert torch.equal(got.double(), want), f"{name} B={B} C={C} S={S}: {describe_diff(got.double(), want)}"
        assert torch.equal(got, got.t()), name
    assert torch.equal(a, b)
    a2, b2 = both_entries(x, scale)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    return want


def small_batches(C, S):
    """1, 2, 3, 7 (at side 12, two images a stack: a lone image, a full stack, a last stack of one image) and one batch just
    above per_kind stacks — with two images a stack an odd one — so that workgroups of every band take a second stack."""
    p = px_plan(cus(), C, S, 1 << 20)
    over = p["NI"] * (p["per_kind"] + 1) - (p["NI"] - 1)
    assert all(px_plan(cus(), C, S, over)["nstack"] > n for n in p["n"])
    return [1, 2, 3, 7, over]


@pytest.mark.parametrize("nonneg", [False, True], ids=["signed", "nonneg"])
@pytest.mark.parametrize("C,S", SHAPES)
def test_integer_factor_is_exact(C, S, nonneg):
    """Integers in {-2 .. 2} and in {0, 1, 2}, a third of them zero, scale 1: all six instantiations, both entries, batches
    of small_batches()."""
    for B in small_batches(C, S):
        assert_exact(int_input(B, C, S, nonneg, seed=1000 * S + 10 * C + B % 7, device="cuda"), 1.0)


@pytest.mark.parametrize("C,S", SHAPES)
def test_integer_factor_with_a_power_of_two_scale(C, S):
    """scale = 2^-10 only moves the exponent: still exact."""
    assert_exact(int_input(7, C, S, False, seed=S + C, device="cuda"), 2.0 ** -10)


def impulse_factor(C, c, y, x, S):
    """The factor of a single 1 at pixel (y, x) of channel c: output position (y - dy, x - dx) sees it through tap
    t = 3 (dy + 1) + (dx + 1), where that position exists — ones on the diagonal at c 9 + t for those taps."""
    want = torch.zeros(9 * C, 9 * C, dtype=torch.float64, device="cuda")
    for t in range(9):
        if 0 <= y - (t // 3 - 1) < S and 0 <= x - (t % 3 - 1) < S:
            want[c * 9 + t, c * 9 + t] = 1.0
    return want


@pytest.mark.parametrize("C,S", SHAPES)
def test_impulses_name_the_tap(C, S):
    """Three images, a single 1: at a corner pixel and at an edge pixel of the first image and at the last pixel of the last
    image (at side 12 the lone image of the last stack), in channel 0 and in channel C - 1.  The expected factor is written
    down without unfold; a wrong halo, tap shift or mirror placement shows as the list of (channel, tap) entries that differ."""
    for c in (0, C - 1):
        for img, y, x in ((0, 0, 0), (0, S // 2, S - 1), (2, S - 1, S - 1)):
            inp = torch.zeros(3, C, S, S, device="cuda")
            inp[img, c, y, x] = 1.0
            want = impulse_factor(C, c, y, x, S)
            assert want.sum().item() == (4 if y in (0, S - 1) else 6)
            assert torch.equal(ref_factor(inp, 1.0), want)
            assert_exact(inp, 1.0, want)


# (image of three, row) of the pixel q the tap-pair sweep is centred on: q's three neighbour rows straddle an edge between two
# row bands of the stack (R = 6: rows 5 | 6, ..., and the short last band 23 | 24 at side 26, 29 | 30 at side 34; side 12 stacks
# two images and cuts R = 8 rows: 7 | 8 of a stack's first image, 3 | 4 of its second)
PAIR_CENTRES = {12: ((0, 7), (1, 4)), 26: ((1, 5), (1, 24)), 34: ((1, 5), (1, 30))}


@pytest.mark.parametrize("C,S", SHAPES)
def test_impulse_pairs_name_the_tap_pair(C, S):
    """A single 1 never fills a block with t' != t, so: a 1 at pixel q of channel 0 and a 1 at q + (dy, dx) of channel C - 1,
    for the nine (dy, dx).  Besides the two diagonals, A[0 9 + t][(C - 1) 9 + t'] = 1 (and its mirror) exactly where t' - t
    is that offset: the output position that sees q through tap t sees q + (dy, dx) through tap t + 3 dy + dx."""
    for img, qy in PAIR_CENTRES[S]:
        qx = S // 2
        for d in range(9):
            dy, dx = d // 3 - 1, d % 3 - 1
            inp = torch.zeros(3, C, S, S, device="cuda")
            inp[img, 0, qy, qx] = 1.0
            inp[img, C - 1, qy + dy, qx + dx] = 1.0
            want = impulse_factor(C, 0, qy, qx, S) + impulse_factor(C, C - 1, qy + dy, qx + dx, S)
            for t in range(9):
                ty, tx = t // 3 + dy, t % 3 + dx
                if 0 <= ty < 3 and 0 <= tx < 3 and 0 <= qy - (t // 3 - 1) < S and 0 <= qx - (t % 3 - 1) < S:
                    want[t, (C - 1) * 9 + 3 * ty + tx] = want[(C - 1) * 9 + 3 * ty + tx, t] = 1.0
            assert torch.equal(ref_factor(inp, 1.0), want)
            assert_exact(inp, 1.0, want)
    R = PX_KERNELS[(C, S)][1]
    for r in range(R - 1, S - 1, R) if S != 12 else ():          # every other band edge, diagonally across it, at the image's left border
        inp = torch.zeros(3, C, S, S, device="cuda")
        inp[2, 0, r, 0] = 1.0
        inp[2, C - 1, r + 1, 1] = 1.0
        assert_exact(inp, 1.0)


# ---- the flush ---------------------------------------------------------------------------------------------------------
def flushing_batch(C, S):
    """The batch of the flush tests on this device.  A wave of kfac_px_body adds its accumulators into the partial buffer and
    restarts them (`spill(wrote)`) once `since >= FLUSH_STEPS = 256` slab steps have run AND another stack follows.  From
    the kernel's plan (kfac_px_support.px_plan): per_kind = max(CUs / 5, NB) workgroups a kind, n[b] = per_kind slabs[b] / tot
    of them on band b, workgroup w taking stacks w, w + n[b], ...; wave group k runs ceil((nslab - k) / KG) steps a stack.
    Wave group 0 of workgroup 0 of band b therefore spills first after i0 = ceil(256 / ceil(nslab / KG)) stacks provided
    stack i0 n[b] exists: B >= NI i0 n[b] + 1 (least_flush_batches; 256 CUs, band 0: 2 925, 8 705, 573, 1 409, 297, 1 025 for
    (64, 12), (32, 12), (64, 26), (32, 26), (64, 34), (32, 34); the short last band of sides 26 and 34: 513, 1 025, 313, 769).
    The test batch is the largest of the bands' — every band has flushed and gone on — plus a small ragged remainder, odd at
    side 12 (flush_batch); flushes() walks the kernel's loop to confirm it."""
    least = least_flush_batches(cus(), C, S)
    B = flush_batch(cus(), C, S)
    if B > MAX_FLUSH_BATCH:
        pytest.fail(f"C={C} S={S}: on {cus()} CUs the accumulators first flush at {max(least)} images (> {MAX_FLUSH_BATCH}): "
                    "this device needs another way to reach the flush")
    assert min(least) <= max(least) < B and all(f >= 1 for f in flushes(cus(), C, S, B))
    assert px_plan(cus(), C, S, B)["NI"] == 1 or B % 2 == 1
    return B


@pytest.mark.parametrize("C,S", SHAPES)
def test_flush_is_exact_on_integers(C, S):
    """{0, 1, 2} inputs at the flushing batch: a flush that overwrites instead of adding, adds twice or drops the
    accumulators' restart is an exact mismatch."""
    B = flushing_batch(C, S)
    assert_exact(int_input(B, C, S, True, seed=S * C, device="cuda"), 1.0)


@pytest.mark.parametrize("C,S", SHAPES)
def test_flush_matches_float64_on_positive_data(C, S):
    """mish(randn) — values in (-0.31, inf), mostly positive: the data the flush exists for — at the flushing batch against
    the float64 factor, within the project's 2e-6 of the largest entry (test_gpu_kfac.py::test_patch_gram_matches_float64).
    Prints the signed relative error of the trace, the all-positive diagonal whose drift the flush bounds (DESIGN.md keeps
    the values measured on an MI355X)."""
    import torch.nn.functional as F
    B = flushing_batch(C, S)
    x = F.mish(torch.randn(B, C, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(S * C + 1)))
    scale = 1.0 / B
    want = ref_factor(x, scale)
    a, b = both_entries(x, scale)
    err = (a.double() - want).abs().max().item() / want.abs().max().item()
    drift = ((a.double().trace() - want.trace()) / want.trace()).item()
    print(f"\nkfac_px flush C={C} S={S} B={B}: max error / max entry {err:.3e}, trace drift {drift:+.3e}")
    assert err < 2e-6
    assert torch.equal(a, b) and torch.equal(a, a.t())


# ---- workspace, arguments, the Python path -----------------------------------------------------------------------------
def test_px16_entry_stays_inside_its_workspace_and_reads_only_what_it_wrote():
    """tron_kfac_gram_px16 with a workspace of exactly tron_kfac_gram_px16_workspace bytes followed by 8 MB of 0x5A: the tail
    is intact and the factor exact; the same with the workspace full of NaN bit patterns gives the same bits, so every part
    k_kfac_px_finish reads was written by a workgroup or zeroed.  Covers grids with idle workgroups (wgs != used: their parts
    are zeroed by a memset) and without (side 26 on 256 CUs), and batches below and above one stack per workgroup."""
    from Net import fused
    PX16, nat = fused.PX16, fused.nat                             # the image class and the library binding it calls through
    L = nat.lib()
    seen = set()
    for C, S in ((32, 12), (64, 26), (64, 34)):
        for B in (3, small_batches(C, S)[-1]):
            p = px_plan(cus(), C, S, B)
            seen.add(p["wgs"] != p["used"])
            x = int_input(B, C, S, True, seed=B + S, device="cuda")
            img = PX16.from_f32(x)
            need = int(L.tron_kfac_gram_px16_workspace(B, C, S))
            assert need >= 5 * p["wgs"] * p["KG"] * 9 * C * C * 4             # the partial sums alone: 5 kinds x (wgs x KG) parts x 9 pairs x C x C floats
            tail = 8 << 20
            grams = []
            for fill in (0x5A, 0xFF):
                buf = torch.full((need + tail,), fill, dtype=torch.uint8, device="cuda")
                gram = torch.empty(9 * C, 9 * C, device="cuda")
                nat.check(L.tron_kfac_gram_px16(nat.ptr(img.buf), B, C, S, 1.0, nat.ptr(gram), nat.ptr(buf), nat.stream_ptr()), "tron_kfac_gram_px16")
                torch.cuda.synchronize()
                assert bool((buf[need:] == fill).all()), f"C={C} S={S} B={B}: wrote past the workspace the size query reserved"
                grams.append(gram)
            want = ref_factor(x, 1.0)
            assert torch.equal(grams[0].double(), want), describe_diff(grams[0].double(), want)
            assert torch.equal(grams[0], grams[1]), "the factor depends on what the workspace held before the call"
    assert seen == {True, False} or cus() != 256


def test_px16_entry_arguments():
    """No instantiation for 48 channels or side 9, and none for an empty batch: the size query answers 0, the entry
    UNSUPPORTED (BAD_ARG for the empty batch).  NULL or misaligned pointers: BAD_ARG.  Nothing launches: the factor buffer
    keeps its fill."""
    from Net import fused
    PX16, nat = fused.PX16, fused.nat                             # the image class and the library binding it calls through
    L = nat.lib()
    assert L.tron_kfac_gram_px16_workspace(4, 48, 12) == 0 and L.tron_kfac_gram_px16_workspace(4, 64, 9) == 0
    assert L.tron_kfac_gram_px16_workspace(0, 64, 12) == 0 and L.tron_kfac_gram_px16_workspace(-1, 64, 12) == 0
    assert all(L.tron_kfac_gram_px16_workspace(4, C, S) > 0 for C, S in SHAPES)
    B, C, S = 4, 64, 12
    img = PX16.from_f32(int_input(B, C, S, True, seed=1, device="cuda"))
    ws = torch.empty(int(L.tron_kfac_gram_px16_workspace(B, C, S)) + 16, dtype=torch.uint8, device="cuda")
    gram = torch.full((9 * C, 9 * C), 7.0, device="cuda")
    i, g, w, st = nat.ptr(img.buf), nat.ptr(gram), nat.ptr(ws), nat.stream_ptr()
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 8)
    assert img.buf.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    assert L.tron_kfac_gram_px16(i, B, 48, S, 1.0, g, w, st) == nat.ERR_UNSUPPORTED
    assert L.tron_kfac_gram_px16(i, B, C, 9, 1.0, g, w, st) == nat.ERR_UNSUPPORTED
    assert L.tron_kfac_gram_px16(i, 0, C, S, 1.0, g, w, st) == nat.ERR_BAD_ARG
    assert L.tron_kfac_gram_px16(None, B, C, S, 1.0, g, w, st) == nat.ERR_BAD_ARG
    assert L.tron_kfac_gram_px16(i, B, C, S, 1.0, None, w, st) == nat.ERR_BAD_ARG
    assert L.tron_kfac_gram_px16(i, B, C, S, 1.0, g, None, st) == nat.ERR_BAD_ARG
    assert L.tron_kfac_gram_px16(off(img.buf), B - 1, C, S, 1.0, g, w, st) == nat.ERR_BAD_ARG
    assert L.tron_kfac_gram_px16(i, B, C, S, 1.0, g, off(ws), st) == nat.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((gram == 7.0).all())
    assert L.tron_kfac_gram_px16(i, B, C, S, 1.0, g, w, st) == nat.OK
    torch.cuda.synchronize()
    assert not bool((gram == 7.0).any())


@pytest.mark.parametrize("C,S,B,micro", [(32, 12, 23, 7), (64, 26, 9, 4), (32, 34, 6, 5)])
def test_cov_inputs_on_a_px16_image_equals_cov_inputs_on_the_tensor(C, S, B, micro):
    """Net/kfac.py::cov_inputs takes a layer's input as an f32 tensor or as the PX16 image the weight-stationary trunk hands
    over; both convert with k_nchw_to_px16 and run the same kernels with the same scale, so the bits agree — for the whole
    batch and for micro-batches' shares of it — and the factor is the reference's P^T P / (B (S S)^2) in float64."""
    import torch.nn.functional as F
    from Net import kfac
    from Net.fused import PX16
    conv = conv_of(C)
    a = F.mish(torch.randn(B, C, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(B)))
    whole = kfac.cov_inputs(a, conv)
    assert torch.equal(kfac.cov_inputs(PX16.from_f32(a), conv), whole)
    want = ref_factor(a, 1.0 / (B * float(S * S) ** 2))
    assert (whole.double() - want).abs().max().item() / want.abs().max().item() < 2e-6
    parts = None
    for i in range(0, B, micro):
        t = kfac.cov_inputs(a[i:i + micro], conv, B)
        assert torch.equal(kfac.cov_inputs(PX16.from_f32(a[i:i + micro]), conv, B), t)
        parts = t if parts is None else parts + t
    assert (parts.double() - want).abs().max().item() / want.abs().max().item() < 2e-6
