"""Helpers of the activation-range tests (tests/test_activation_range_cpu.py, tests/test_gpu_activation_range.py): the sweep of
planted pre-activations, its placement in an image, the host side of the PX16 format in float64, and the float64 references of
mish and mish'.  Nothing here needs a GPU at import."""
import numpy as np
import torch

F = torch.nn.functional


def _neighbours(v, ks):
    """The float32 values k ulps away from float32(v), k in ks."""
    out = []
    for k in ks:
        x = np.float32(v)
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
        out.append(float(x))
    return out


def special_points():
    """The points at which one copy of the fast formula could go wrong while another does not (float32)."""
    pts = [0.0, -0.0]
    pts += _neighbours(20.0, (-1, 0, 1))                     # the select of the mish1 copies
    pts += _neighbours(-1.1924, (-3, -1, 0, 1, 3))           # the derivative's zero: (1 - t^2)'s sign shows left of it
    pts += [41.4465, 44.3614]                                # ln 1e18 (the cap); e * e overflows
    pts += [-87.3365, -87.4, -103.9, 88.8]                   # exp2's flush boundary; denormal e^x; exp overflows
    for m in (1e3, 3e4, 1e6, 1e-3, 1e-6, 1e-9):
        pts += [m, -m]
    return torch.tensor(pts, dtype=torch.float32)


def sweep():
    """Every planted value: the activation's range on a grid, plus special_points()."""
    return torch.cat([torch.linspace(-110.0, 110.0, 4001, dtype=torch.float64).float(), special_points()])


def band_rows(S):
    """The rows on either side of a band edge of the convolution kernels: S / 2 at 26 (and, by the same rule, at 12), rows 8 / 9,
    16 / 17, 24 / 25 at 34."""
    return (8, 9, 16, 17, 24, 25) if S == 34 else (S // 2 - 1, S // 2)


def placement(B, C, S, seed):
    """Where fill() puts special point k: three [n, 4] index arrays (image, channel, row, column) — an image corner, a row end
    that is no corner, an interior pixel of a row beside a band edge; all positions distinct."""
    n = special_points().numel()
    rs = np.random.RandomState(seed)
    assert 4 * B * C >= n and S >= 6
    planes = rs.permutation(B * C * 4)[:n]
    corner = np.stack([planes // 4 // C, planes // 4 % C, (planes % 4 // 2) * (S - 1), (planes % 2) * (S - 1)], 1)
    ends = rs.permutation(B * C * (S - 2) * 2)[:n]
    row_end = np.stack([ends // (2 * (S - 2)) // C, ends // (2 * (S - 2)) % C, 1 + ends // 2 % (S - 2), (ends % 2) * (S - 1)], 1)
    rows = np.asarray(band_rows(S))
    bands = rs.permutation(B * C * len(rows) * (S - 2))[:n]
    pl, rest = bands // (len(rows) * (S - 2)), bands % (len(rows) * (S - 2))
    band = np.stack([pl // C, pl % C, rows[rest // (S - 2)], 1 + rest % (S - 2)], 1)
    return corner, row_end, band


def check_placement(t, B, C, S, seed):
    """fill()'s guarantee, bit for bit (so that -0.0 counts): every special point sits in a corner, at a row end and beside a band edge."""
    bits = t.contiguous().view(torch.int32)
    sp = special_points().view(torch.int32)
    rows = band_rows(S)
    for name, idx in zip(("corner", "row end", "band edge"), placement(B, C, S, seed)):
        b, c, y, x = (torch.from_numpy(idx[:, i].astype(np.int64)) for i in range(4))
        assert torch.equal(bits[b, c, y, x], sp), name
        if name == "corner":
            assert all(int(v) in (0, S - 1) for v in y) and all(int(v) in (0, S - 1) for v in x)
        elif name == "row end":
            assert all(0 < int(v) < S - 1 for v in y) and all(int(v) in (0, S - 1) for v in x)
        else:
            assert all(int(v) in rows for v in y) and all(0 < int(v) < S - 1 for v in x)


def fill(B, C, S, seed):
    """float32 [B, C, S, S]: a seeded permutation of sweep(), tiled, with every special point planted in an image corner, at a row
    end and in a row beside a band edge (asserted)."""
    sw = sweep()
    n = B * C * S * S
    g = torch.Generator().manual_seed(seed)
    perm = sw[torch.randperm(sw.numel(), generator=g)]
    t = perm.repeat((n + perm.numel() - 1) // perm.numel())[:n].reshape(B, C, S, S).clone()
    sp = special_points()
    for idx in placement(B, C, S, seed):
        b, c, y, x = (torch.from_numpy(idx[:, i].astype(np.int64)) for i in range(4))
        t[b, c, y, x] = sp
    check_placement(t, B, C, S, seed)
    return t


# ---- PX16 on the host, float64: per image [hi | lo][channel octet][pixel][8 channels] f16, value / 64 = hi + lo / 2048 ------

def pack_px(x, scale=None):
    """[B, C, S, S] -> the PX16 bytes (uint8, flat) of x * scale."""
    B, C, S, _ = x.shape
    v = (x.double() * (1.0 if scale is None else scale) / 64.0)
    hi = v.to(torch.float16)
    lo = ((v - hi.double()) * 2048.0).to(torch.float16)
    def lay(t):                                                      # [B, C, S, S] -> [B][octet][pixel][8 channels]
        return t.reshape(B, C // 8, 8, S * S).permute(0, 1, 3, 2).contiguous()
    img = torch.stack([lay(hi), lay(lo)], 1).contiguous()            # [B][hi | lo][octet][pixel][8]
    return img.view(torch.uint8).reshape(-1)


def unpack_px(buf, B, C, S):
    """The PX16 bytes -> float64 [B, C, S, S]: 64 (hi + lo / 2048), exactly."""
    img = buf.view(torch.float16).reshape(B, 2, C // 8, S * S, 8).double()
    v = 64.0 * (img[:, 0] + img[:, 1] / 2048.0)                      # [B][octet][pixel][8]
    return v.permute(0, 1, 3, 2).reshape(B, C, S, S).contiguous()


def to_px(fused, x, scale=None):
    """f32 [B, C, S, S] -> a PX16 image (host-side packing: test infrastructure) of x * scale."""
    B, C, S, _ = x.shape
    px = fused.PX16(B, C, S, x.device)
    px.buf.copy_(pack_px(x, scale))
    return px


def px_value(px):
    """What a PX16 (or gradient) image's bytes say, float64, unscaled."""
    return unpack_px(px.buf, *px.shape[:3])


def out_floor(ref):
    """|ref - unpack(pack(ref))|: what storing the reference itself as PX16 would lose ([B, C, S, S], C a multiple of 8)."""
    B, C, S, _ = ref.shape
    return (ref.double() - unpack_px(pack_px(ref), B, C, S)).abs()


# ---- float64 references ---------------------------------------------------------------------------------------------------

def mish64(x):
    """x tanh(softplus x), the composed form, float64."""
    x = x.double()
    return x * torch.tanh(F.softplus(x))                             # (softplus is x itself beyond 20, where tanh is 1 to 1e-17)


def dmish64(x):
    """d mish / dx by float64 autograd of the composed form."""
    x = x.double().detach().clone().requires_grad_(True)
    mish64(x).sum().backward()
    return x.grad


# ---- the fast formula of the fused epilogues, emulated in float32 with correctly rounded exp2 and 1 / x ------------------------

def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def fast_formula(x):
    """(mish, mish') of float32 x by e = min(exp2(x log2 e), 1e18) (results below the smallest normal flushed to 0), n = e e + 2 e,
    r = 1 / (n + 2), t = n r, y = x t, m = t + x (2 r (1 + t)) e / (1 + e): every operation rounded to float32 once."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        arg = x * np.float32(1.44269504088896341)
        e = _f32(np.exp2(arg.astype(np.float64)))
        e[np.abs(e) < np.finfo(np.float32).tiny] = 0.0
        e = np.minimum(e, np.array(0x5D5E0B6B, dtype=np.uint32).view(np.float32))
        e64 = e.astype(np.float64)
        n = _f32(e64 * e64 + (e + e).astype(np.float64))              # one fma
        d = n + np.float32(2.0)
        r = _f32(1.0 / d.astype(np.float64))
        t = n * r
        y = x * t
        q = _f32(1.0 / (e + np.float32(1.0)).astype(np.float64))
        m = t + x * ((r + r) * (np.float32(1.0) + t)) * (e * q)
    return y, m
