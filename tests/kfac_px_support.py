"""What the tests of csrc/tron_kfac_px.hip share (tests/test_gpu_kfac_px.py, tests/test_kfac_px_reference_cpu.py): the float64
reference of a 3x3 / pad 1 / stride 1 layer's input factor, the integer inputs whose factor is exact in f32, and the kernel's
launch plan written out again in Python, from which the tests derive the batches at which its accumulators flush.  A plain
module, imported by name; nothing here needs a GPU."""
import torch
import torch.nn.functional as F

# (C, S) -> (NI images per stack, R rows per band, KG wave groups that split a band's slabs): kfac_px_dispatch's six KCfg
PX_KERNELS = {(64, 12): (2, 8, 1), (32, 12): (2, 8, 4), (64, 26): (1, 6, 1), (32, 26): (1, 6, 4), (64, 34): (1, 6, 1), (32, 34): (1, 6, 4)}
FLUSH_STEPS = 256                                                # kfac_px_body: slab steps between two spills of a wave
KINDS = 5                                                        # workgroup kinds: each takes nine of the 45 tap pairs
EXACT_LIMIT = 1 << 24                                            # integers an f32 holds exactly


def ref_factor(x_int, scale, chunk=512):
    """scale * P^T P in float64, P = the patch matrix of x_int [B, C, S, S] for a 3x3 / pad 1 / stride 1 convolution: a
    [9 C, 9 C] tensor on x_int's device, rows and columns channel-major (c * 9 + t, t = 3 ky + kx: F.unfold's order).  Built
    with F.unfold over chunks of at most `chunk` images (fewer where a chunk's patches would pass 256 MB)."""
    B, C, S, S2 = x_int.shape
    assert S == S2
    d = 9 * C
    step = max(1, min(chunk, 512, (1 << 25) // (d * S * S)))
    A = torch.zeros(d, d, dtype=torch.float64, device=x_int.device)
    for i in range(0, B, step):
        cols = F.unfold(x_int[i:i + step].to(torch.float64), 3, padding=1)          # [n, 9 C, S S]
        P = cols.transpose(1, 2).reshape(-1, d)
        A += P.t() @ P
    return A * scale


def int_input(B, C, S, nonneg, seed, device="cpu"):
    """Integers as f32 [B, C, S, S] from a fixed seed, a third of them zero: {-2 .. 2} (0 twice as likely as each other
    value), or with nonneg {0, 1, 2} — all non-negative, as post-activation data is."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    if nonneg:
        v = torch.randint(0, 3, (B, C, S, S), generator=g, dtype=torch.int8)
    else:
        v = torch.tensor([0, 0, -2, -1, 1, 2], dtype=torch.int8)[torch.randint(0, 6, (B, C, S, S), generator=g)]
    return v.to(device).float()


def exact_bound(B, S, vmax=2):
    """The largest numerator a partial sum of the factor can reach, in units of 2^-12: inputs |x| <= vmax go in as x / 64, so a
    product is a multiple of 2^-12 of at most vmax^2 of them, and an entry sums B S^2 products.  Below EXACT_LIMIT every
    partial sum is an f32, whatever the order or the rounding mode of the additions."""
    return B * S * S * vmax * vmax


def px_plan(cus, C, S, B):
    """kfac_px_run's launch plan for B images on a device of `cus` compute units: per kind, band b (R rows of the NI-image
    stack) gets n[b] workgroups in proportion to its 32-pixel slabs, never more than there are stacks; workgroup w of a band
    takes the stacks w, w + n[b], ...; the grid is rounded up to whole groups of eight."""
    NI, R, KG = PX_KERNELS[(C, S)]
    rows = NI * S
    NB = (rows + R - 1) // R
    per_kind = max(cus // KINDS, NB)
    slabs = [(min(R, rows - b * R) * S + 31) // 32 for b in range(NB)]
    tot = sum(slabs)
    nstack = (B + NI - 1) // NI
    n = [min(max(per_kind * s // tot, 1), nstack) for s in slabs]
    used = sum(n)
    return dict(NI=NI, R=R, KG=KG, NB=NB, per_kind=per_kind, slabs=slabs, n=n, nstack=nstack, used=used, wgs=(used + 7) // 8 * 8)


def steps_per_stack(nslab, KG, kgroup):
    """Slab steps wave group `kgroup` runs per stack: the slabs kgroup, kgroup + KG, ... of the band's nslab."""
    return (nslab - kgroup + KG - 1) // KG if kgroup < nslab else 0


def flushes(cus, C, S, B):
    """Per band, the most mid-run spills (`since >= FLUSH_STEPS` with another stack behind it) any wave of the band does: the
    kernel's stack loop, walked for every (workgroup, wave group)."""
    p = px_plan(cus, C, S, B)
    out = []
    for b in range(p["NB"]):
        most = 0
        for wb in range(p["n"][b]):
            for k in range(p["KG"]):
                per, since, count = steps_per_stack(p["slabs"][b], p["KG"], k), 0, 0
                for stack in range(wb, p["nstack"], p["n"][b]):
                    since += per
                    if since >= FLUSH_STEPS and stack + p["n"][b] < p["nstack"]:
                        count, since = count + 1, 0
                most = max(most, count)
        out.append(most)
    return out


def least_flush_batches(cus, C, S):
    """Per band, the least batch at which one of its waves spills and then goes on accumulating.  Wave group 0 of workgroup 0
    gets there first: it runs ceil(nslab / KG) steps per stack, so `since` reaches FLUSH_STEPS after
    i0 = ceil(FLUSH_STEPS / steps) stacks, the last of them stack (i0 - 1) n[b]; the spill needs the next one, i0 n[b], to
    exist: nstack >= i0 n[b] + 1, that is B >= NI i0 n[b] + 1 (n[b] uncapped: there are far more stacks than workgroups)."""
    p = px_plan(cus, C, S, 1 << 20)
    out = []
    for b in range(p["NB"]):
        i0 = -(-FLUSH_STEPS // steps_per_stack(p["slabs"][b], p["KG"], 0))
        out.append(p["NI"] * i0 * p["n"][b] + 1)
    return out


def flush_batch(cus, C, S):
    """The batch the flush tests run: the least at which EVERY band has a wave that spills and goes on (the largest of
    least_flush_batches; its smallest is where the first wave of the launch does), plus the smallest remainder >= 5 that
    leaves every band ragged (the stacks no multiple of its workgroups) and, with two images per stack, the batch odd, so
    that the last stack holds one image."""
    least = max(least_flush_batches(cus, C, S))
    B = least + 5
    while True:
        p = px_plan(cus, C, S, B)
        if all(p["nstack"] % n for n in p["n"] if n > 1) and (p["NI"] == 1 or B % 2):
            return B
        B += 1


def describe_diff(got, want, limit=12):
    """The first entries where two factors differ, named by (channel, tap) of row and column."""
    bad = (got != want).nonzero().tolist()
    lines = [f"{len(bad)} entries differ"]
    for r, c in bad[:limit]:
        lines.append(f"  A[c={r // 9} t={r % 9}][c'={c // 9} t'={c % 9}]: got {got[r, c].item()!r}, want {want[r, c].item()!r}")
    return "\n".join(lines)
