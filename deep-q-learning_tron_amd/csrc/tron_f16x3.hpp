// tron_f16x3.hpp — the split-f16 number format that the matrix-core kernels hand each other, stated once.
//
// gfx950 has no reduced-precision fast path for f32 inputs (v_mfma_f32_16x16x4_f32 runs at 1/16 of the f16 rate), so an
// f32 value travels as two f16 halves,
//     v = hi + lo * 2^-11,      hi = f16(v),  lo = f16((v - hi) * 2^11)                         (to within 2^-22 |v|),
// and a product is three f16 MFMAs with f32 accumulation: ah*bh + (ah*bl + al*bh) * 2^-11 (tron_conv_f16.hip has the
// error bound).  What keeps the halves inside f16 is a power-of-two scale applied BEFORE the split and undone, exactly,
// by whoever reads the accumulators:
//   * activations carry ACT_SCALE = 2^-6 (|x| up to 4e6 stays inside f16; tiny values lose nothing, because lo picks up
//     what hi's subnormal rounding drops); weights are split as they are;
//   * a gradient tensor is orders of magnitude smaller and carries the power of two that puts its largest magnitude in
//     [2^13, 2^14), found from per-block maxima of |g| (wave_absmax / absmax_scale below).
// One kernel writes this format and another reads it — the conv epilogue's split image feeds the next layer's staging,
// the PX16 image feeds the head and K-FAC, the weight-gradient operands are split the same way — so the constants and
// helpers live here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tron {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float ACT_SCALE = 1.0f / 64.0f, ACT_UNSCALE = 64.0f, LO_SCALE = 2048.0f, LO_UNSCALE = 1.0f / 2048.0f;

// v -> (hi, lo): v = hi + lo * 2^-11 up to 2^-22 |v|
__device__ __forceinline__ void split(float v, f16 &hi, f16 &lo)
{
    hi = (f16)v;
    lo = (f16)((v - (float)hi) * LO_SCALE);
}
__device__ __forceinline__ uint32_t pack2(f16 a, f16 b)
{
    const f16x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, v);
}

// ---- a gradient's scale -------------------------------------------------------------------------------------------------
// A gradient tensor's producer leaves per-block maxima of |g| in absmax[0, n); the consumer's workgroup (THREADS threads)
// turns them into one power-of-two scale in three steps:
//   1. wave_absmax: every wave's maximum into red[wave] (THREADS / 64 floats of LDS), then a __syncthreads();
//   2. the caller takes the maximum of red[0 .. THREADS / 64) — a handful of fmaxf that the kernels order differently (a
//      tree in tron_conv_wgrad.hip, a chain from 0 in tron_conv_wgrad_rows.hip); either order changes the other kernel's
//      machine code (which maxima pair up in v_max3_f32), so that line stays with each caller;
//   3. absmax_scale: 2^(14 - e) for a maximum m = f 2^e, which puts it in [2^13, 2^14) — or the caller's fallback where
//      there is no usable maximum: zero, denormal (below 2^-101), infinite or NaN gradients.  A huge finite maximum IS scaled
//      (down): fed to split() unscaled it would overflow f16 to inf and the MFMAs would sum inf - inf.
// The fallback is deliberately not the same everywhere: the weight-gradient kernels fall back to 1.0 (the gradient goes
// in unscaled), tron_conv_f16.hip's data-gradient call keeps the activation scale ACT_SCALE / ACT_UNSCALE it starts from.
// NOT shared, each with its own copy of this arithmetic because sharing changed its machine code:
//   * tron_conv_f16.hip's k_conv3x3_f16 (open-coded at its top; it needs the scale and its inverse): with wave_absmax and a
//     shared exponent test the same instructions come out under another register allocation through the whole kernel;
//   * k_absmax_pow2 in tron_dqn.hip (ONE maximum of a whole tensor across workgroups with atomics, the target exponent
//     from its caller, a clamp to +-60): spelt with shared helpers its select compiles to a branch;
//   * pow2_at_most in tron_conv_ws_kernel.hpp rounds a bound DOWN to a power of two, clamped likewise: other arithmetic.
template <int THREADS>
__device__ __forceinline__ float wave_absmax(const float *__restrict__ absmax, int n_absmax, float *red)
{
    float m = 0.0f;
    for (int i = threadIdx.x; i < n_absmax; i += THREADS) m = fmaxf(m, absmax[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    return m;
}
__device__ __forceinline__ float absmax_scale(float m, float fallback)
{
    const uint32_t bits = __float_as_uint(m);
    const int e = (int)((bits >> 23) & 255u) - 126;                     // m = f 2^e, f in [0.5, 1)
    if (!(m > 0.0f) || e < -100 || e > 128) return fallback;           // (e = 129: inf.  Every finite maximum from 2^-101 up is scaled:
    return __uint_as_float((uint32_t)(127 + 14 - e) << 23);            // 2^(14 - e) and its inverse stay normal floats up to e = 128)
}

// ---- the product over a wave's TM x TN block of 16 x 16 MFMA tiles, one 32-deep K slab ---------------------------------------
// acc0 += ah bh, acc1 += ah bl + al bh (whoever reads them joins acc0 + acc1 * LO_UNSCALE), as three sweeps over the block:
// hi*lo, hi*hi, lo*hi.  The lo*hi MFMA adds to the accumulator the hi*lo one wrote, and a dependent MFMA issues 48 cycles
// after its producer — two sweeps (eight MFMAs at 2 x 2) apart nobody waits.
// NOT shared: k_gram2_f16x3 in tron_kfac.hip keeps the same three sweeps open-coded — through this helper the same instructions
// come out under another register allocation (its accumulators are zeroed in another order and the MFMAs name other registers);
// k_gram_nchw there interleaves the three products per tile on purpose.  The 1-D sites (one row or column of tiles per wave:
// k_conv7_wgrad, tron_kfac_px.hip, the conv kernels) have loops of their own shape.
template <int TM, int TN>
__device__ __forceinline__ void mma_f16x3(const f16x8 (&ah)[TM], const f16x8 (&al)[TM], const f16x8 (&bh)[TN], const f16x8 (&bl)[TN],
                                          f32x4 (&acc0)[TM][TN], f32x4 (&acc1)[TM][TN])
{
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc1[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bl[n], acc1[t][n], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc0[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bh[n], acc0[t][n], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < TM; ++t)
#pragma unroll
        for (int n = 0; n < TN; ++n) acc1[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], bh[n], acc1[t][n], 0, 0, 0);
}

// ---- operands read transposed out of LDS --------------------------------------------------------------------------------
// ds_read_b64_tr_b16 by inline asm, not by __builtin_amdgcn_ds_read_tr16_b64: behind the builtin hipcc (ROCm 7.2) puts an
// s_waitcnt vmcnt(0) in front of every transposed read that follows an LDS-DMA (it cannot tell the read from the copy's
// destination), which serialised each of an item's nine copies with the multiply in tron_conv_ws_train.hip's k_wgrad_px —
// 11 us per item instead of 3 (the .s showed ten vmcnt(0) per item) — and, in tron_head.hip's k_conv7_wgrad, waited for the
// next image's copy before the multiply began.  The asm is invisible to that pass; what it costs is that the waits are ours:
// a step's reads go out one step ahead, `lds_tr_wait()` (s_waitcnt lgkmcnt(0) + sched_barrier, so that no consumer moves
// above it) stands between a read and the first use of its registers, and the two 8-byte halves are joined into the MFMA
// operand only AFTER that wait (a copy the compiler might make of them then reads landed data).  EXEC must be all ones (the
// read crosses lanes).
__device__ __forceinline__ s16x4 lds_tr(uint32_t addr)
{
    s16x4 r;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=&v"(r) : "v"(addr));
    return r;
}
__device__ __forceinline__ void lds_tr_wait()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ f16x8 join8(s16x4 a, s16x4 b)
{
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(f16x8, v);
}

}  // namespace tron
