"""Host model of the gradient-scale arithmetic of csrc/tron_f16x3.hpp (wave_absmax / absmax_scale and their open-coded copies)
and of k_absmax_pow2 (csrc/tron_dqn.hip), in numpy from frexp / ldexp, and the inputs the scale tests share: the f32 exponent
sweep, the spike positions and the planted tensors.  No GPU, no torch in the models."""
import numpy as np

F32 = np.float32
THREADS = (256, 512)                     # workgroup sizes of the consumers' absmax loops (k_wgrad / k_wgrad_rows; k_conv3x3_f16)
SCALE_E_MIN, SCALE_E_MAX = -100, 128     # absmax_scale scales maxima m = f 2^e, f in [0.5, 1), with -100 <= e <= 128: every finite one from 2^-101 up
POW2_CLAMP = 60                          # k_absmax_pow2 clamps its exponent to +-60 (the scale's square stays finite)
BIAS_SEGS = 64                           # tron_bias_mish_bwd: batch segments per channel
SPIKE = 1024.0                           # against uniform(-1, 1): a missed spike is scaled to >= 2^23 and overflows f16


# ---- the models -------------------------------------------------------------------------------------------------------------

def absmax_scale(m, fallback):
    """tron_f16x3.hpp::absmax_scale: 2^(14 - e) for m = f 2^e, f in [0.5, 1); the fallback for m <= 0 (or NaN), e < -100 and inf
    (the kernel's e > 128).  A huge finite maximum is scaled like any other: unscaled it would overflow f16 to inf.
    (The kernel reads e from the exponent field, -126 for a denormal: frexp's e is smaller still, the fallback either way.)"""
    m = F32(m)
    if not m > 0:
        return F32(fallback)
    if np.isinf(m):
        return F32(fallback)
    _, e = np.frexp(np.float64(m))
    if e < SCALE_E_MIN or e > SCALE_E_MAX:
        return F32(fallback)
    return F32(np.ldexp(1.0, 14 - int(e)))


def absmax_pow2(m, target_exp):
    """k_absmax_pow2's out[0]: 2^k, k = clamp(target_exp - e, -60, 60) for the maximum m = f 2^e; 1 for an all-zero tensor.  The
    kernel takes e = -126 for a denormal where frexp says less: k >= -60 + 126 > 60 in both, so the clamp gives the same 2^60."""
    m = F32(m)
    if not m > 0:
        return F32(1.0)
    _, e = np.frexp(np.float64(m))
    k = min(max(int(target_exp) - int(e), -POW2_CLAMP), POW2_CLAMP)
    return F32(np.ldexp(1.0, k))


def absmax_scale_bits(m, fallback):
    """The kernel's own spelling of absmax_scale, on the bit pattern (a second, independent route to the same numbers)."""
    bits = int(np.array(m, dtype=F32).view(np.uint32))
    e = ((bits >> 23) & 255) - 126
    if not F32(m) > 0 or e < SCALE_E_MIN or e > SCALE_E_MAX:
        return F32(fallback)
    return np.array((127 + 14 - e) << 23, dtype=np.uint32).view(F32)[()]


def absmax_pow2_bits(m, target_exp):
    bits = int(np.array(m, dtype=F32).view(np.uint32))
    e = ((bits >> 23) & 255) - 126
    k = min(max(int(target_exp) - e, -POW2_CLAMP), POW2_CLAMP)
    return np.array((127 + k) << 23, dtype=np.uint32).view(F32)[()] if F32(m) > 0 else F32(1.0)


# ---- the exponent sweep -----------------------------------------------------------------------------------------------------

def normal_sweep():
    """Every f32 exponent at both mantissa ends: 2^k and the float just below it, k = -126 .. 127 (nextafter(2^-126, 0) is the
    largest denormal and belongs to denormal_sweep)."""
    out = []
    for k in range(-126, 128):
        p = F32(np.ldexp(1.0, k))
        out.append(p)
        if k > -126:
            out.append(np.nextafter(p, F32(0.0), dtype=F32))
    out.append(np.finfo(F32).max)
    return out


def denormal_sweep():
    """2^k and the float below it for k = -149 .. -127, and the largest denormal."""
    out = []
    for k in range(-149, -126):
        p = F32(np.ldexp(1.0, k))
        out.append(p)
        below = np.nextafter(p, F32(0.0), dtype=F32)
        if below > 0 and below != out[-2 if len(out) > 1 else 0]:      # (the float below 2^-148 is 2^-149 itself)
            out.append(below)
    out.append(np.nextafter(F32(np.ldexp(1.0, -126)), F32(0.0), dtype=F32))
    return out


def sweep():
    return denormal_sweep() + normal_sweep()


# ---- planted tensors --------------------------------------------------------------------------------------------------------

def pow2_positions(n, grid_stride=None):
    """Where tron_absmax_pow2's tests plant the maximum in a tensor of n floats: both ends, the n % 4 tail, the middle, the first
    and last element of a 256 x 4 and of a 1024 x 4 block, and (grid_stride = gridDim 1024 float4) the first float4 a workgroup
    reads on its second trip."""
    want = [0, n - 1, n - 2, n - 3, n // 2, 1023, 1024, 2047, 4095, 4096]
    if grid_stride is not None:
        want += [4 * grid_stride - 1, 4 * grid_stride, 4 * grid_stride + 5]
    return sorted({p for p in want if 0 <= p < n})


def pow2_grid(n):
    """tron_absmax_pow2's launch (csrc/tron_dqn.hip): workgroups of 1 024 threads, four float4 per thread before another
    workgroup pays, at most 256."""
    blocks = (n // 4 + 4095) // 4096
    return min(max(blocks, 1), 256)


def background(n, seed):
    """uniform(-1, 1) * 2^-4, f32 [n]."""
    return (np.random.RandomState(seed).uniform(-1.0, 1.0, n) * 2.0 ** -4).astype(F32)


def planted(n, p, v, seed):
    """uniform(-1, 1) * 2^-4 with x[p] = v.  Where |v| < 1 the background is scaled by |v| as well (in float64, then rounded), so
    that the planted value stays the tensor's only maximum down to the denormals (the background then rounds to smaller
    denormals or to zero)."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1.0, 1.0, n) * 2.0 ** -4 * min(1.0, abs(float(v)))
    x = x.astype(F32)
    x[p] = v
    assert np.abs(np.delete(x, p)).max(initial=0.0) < abs(F32(v)) or n == 1
    return x


def spike_positions(B, C, S, ragged_group=16, octet=True):
    """(name, (b, c, y, x)) of the entries a spike test plants, in a [B, C, S, S] tensor: first and last element, last image, last
    channel, the four corner pixels (in a middle image and channel), the last image of a ragged group of `ragged_group` images,
    the last channel of an octet."""
    bm, cm = B // 2, C // 2 + 1
    pos = [("first", (0, 0, 0, 0)), ("last", (B - 1, C - 1, S - 1, S - 1)), ("last image", (B - 1, 1, 3, 4)),
           ("last channel", (0, C - 1, 5, 2)), ("corner 00", (bm, cm, 0, 0)), ("corner 0S", (bm, cm, 0, S - 1)),
           ("corner S0", (bm, cm, S - 1, 0)), ("corner SS", (bm, cm, S - 1, S - 1))]
    if B % ragged_group:
        pos.append(("ragged group", (B - 1, cm, S // 2, S // 2)))
    if octet:
        pos.append(("octet end", (bm, 7, 1, S - 2)))
        pos.append(("last octet end", (bm, C - 1, S - 2, 1)))
    seen, out = set(), []
    for name, p in pos:
        if p not in seen:
            seen.add(p)
            out.append((name, p))
    return out


def segment_bounds(N, seg):
    """tron_bias_mish_bwd's block (c, seg) owns the images [N seg / 64, N (seg + 1) / 64)."""
    return N * seg // BIAS_SEGS, N * (seg + 1) // BIAS_SEGS


def absmax_indices(n):
    """Where the n_absmax tests put the only large record: both ends and the seams of the consumers' strided loops."""
    want = [0, n - 1]
    for t in THREADS:
        want += [t - 1, t]
    return sorted({i for i in want if 0 <= i < n})
