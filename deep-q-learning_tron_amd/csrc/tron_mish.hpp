// tron_mish.hpp — the activation of every net in the reference, mish(x) = x * tanh(softplus(x)) (Net/ACNet.py:56-57), in the
// three arithmetics the kernels use.  Each kernel names the one it wants; none is a drop-in for another (their last bits
// differ), which is why the activation-range sweep tests every fused epilogue.
//
// With e = exp(x):
//     tanh(log1p(e)) = ((1+e)^2 - 1) / ((1+e)^2 + 1) = n / (n + 2),   n = e * (e + 2)
// so one exp and one division give the forward value, with no cancellation anywhere (for x -> -inf, n -> 2e and the
// quotient -> e; for x > 20 the result is x to fp32 precision — the same cut-over as F.softplus's threshold — which also
// keeps e*e from overflowing).  Backward:
//     d/dx = t + x * (1 - t^2) * e / (1 + e),   t = n / (n + 2),   1 - t^2 = (2 / (n + 2)) (1 + t).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tron_f16x3.hpp"

namespace tron {

// ---- exact: expf and IEEE division (tron_nn.hip's memory-bound passes) -----------------------------------------------------
__device__ __forceinline__ float mish_exact(float x)
{
    if (x > 20.0f) return x;
    const float e = expf(x);
    const float n = e * (e + 2.0f);
    return x * (n / (n + 2.0f));
}
__device__ __forceinline__ float mish_grad_exact(float x, float gy)
{
    if (x > 20.0f) return gy;
    const float e = expf(x);
    const float n = e * (e + 2.0f);
    const float t = n / (n + 2.0f), u = 2.0f / (n + 2.0f);       // u = 1 - t without the cancellation
    return gy * (t + x * (u * (1.0f + t)) * (e / (1.0f + e)));   // sech^2 = 1 - t^2 = (1 - t)(1 + t)
}

// ---- fast scalar (tron_conv.hip, tron_conv_f16.hip's and tron_head.hip's scalar epilogues) ---------------------------------
// An epilogue runs 72-88 of these per lane with the matrix pipe idle, so it is built from the two hardware
// transcendentals: exp2 of x * log2(e) — its argument rounding costs |x| 2^-24 relative in e, which mish turns into
// < 4e-8 ABSOLUTE (x^2 e^x <= 0.55 where e matters, and n / (n + 2) -> 1 where e is large) — and a reciprocal
// refined by one Newton step (v_rcp_f32 alone is 1 ulp) instead of the ~10-instruction IEEE division.
__device__ __forceinline__ float mish_fast(float x)
{
    const float e = __builtin_amdgcn_exp2f(x * 1.44269504088896341f);
    const float n = __fmaf_rn(e, e, e + e);
    const float d = n + 2.0f;
    float r = __builtin_amdgcn_rcpf(d);
    r = __fmaf_rn(r, __fmaf_rn(-d, r, 1.0f), r);
    const float y = x * (n * r);
    return x > 20.0f ? x : y;                        // e * e overflows beyond x = 44; the quotient is 1 from 20 on
}

// ---- capped (the split-f16 kernels' vector epilogues) -----------------------------------------------------------------------
// Four values at once, written on vectors so that the compiler packs the arithmetic two per instruction (v_pk_*): the
// epilogue is VALU-issue-bound (docs/DESIGN_history_r01_r03.md 4b).  No select for large x: e^x is capped at 1e18 (an unsigned integer min
// on the bits — e is never negative — so no NaN-canonicalising v_max comes with it); n = e (e + 2) then stays finite
// and n / (n + 2) is exactly 1 up there, so the product is x itself.  One rcp (1 ulp), no Newton step.
__device__ __forceinline__ f32x4 mish4_capped(f32x4 x)
{
    const f32x4 t = x * 1.44269504088896341f;
    f32x4 e;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t b = __float_as_uint(__builtin_amdgcn_exp2f(t[i]));
        e[i] = __uint_as_float(b < 0x5D5E0B6Bu ? b : 0x5D5E0B6Bu);      // min(e, 1e18)
    }
    const f32x4 n = __builtin_elementwise_fma(e, e, e + e);
    const f32x4 d = n + 2.0f;
    const f32x4 r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1]), __builtin_amdgcn_rcpf(d[2]), __builtin_amdgcn_rcpf(d[3])};
    return x * (n * r);
}

// gy * mish'(x) the same way (mish_grad_exact with exp2 / rcp).  With e capped at 1e18, t is exactly 1 and the second term 0
// up there.
__device__ __forceinline__ f32x4 mish_grad4_capped(f32x4 x, f32x4 gy)
{
    const f32x4 t2 = x * 1.44269504088896341f;
    f32x4 e;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t b = __float_as_uint(__builtin_amdgcn_exp2f(t2[i]));
        e[i] = __uint_as_float(b < 0x5D5E0B6Bu ? b : 0x5D5E0B6Bu);
    }
    const f32x4 n = __builtin_elementwise_fma(e, e, e + e);
    const f32x4 d = n + 2.0f, e1 = e + 1.0f;
    const f32x4 r = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1]), __builtin_amdgcn_rcpf(d[2]), __builtin_amdgcn_rcpf(d[3])};
    const f32x4 q = {__builtin_amdgcn_rcpf(e1[0]), __builtin_amdgcn_rcpf(e1[1]), __builtin_amdgcn_rcpf(e1[2]), __builtin_amdgcn_rcpf(e1[3])};
    const f32x4 t = n * r, u = r + r;
    return gy * (t + x * (u * (1.0f + t)) * (e * q));
}

// mish'(x) alone, one value: mish_grad4_capped's scalar twin (tron_head.hip's k_mish_bwd_to_cl)
__device__ __forceinline__ float mish_grad_capped(float x)
{
    const uint32_t eb = __float_as_uint(__builtin_amdgcn_exp2f(x * 1.44269504088896341f));
    const float e = __uint_as_float(eb < 0x5D5E0B6Bu ? eb : 0x5D5E0B6Bu);      // e^x capped at 1e18: t is exactly 1 up there
    const float n = __fmaf_rn(e, e, e + e);                              // tanh(softplus x) = n / (n + 2)
    const float r = __builtin_amdgcn_rcpf(n + 2.0f), q = __builtin_amdgcn_rcpf(e + 1.0f);
    const float t = n * r;
    return t + x * ((r + r) * (1.0f + t)) * (e * q);                     // t + x (1 - t^2) sigmoid(x)
}

}  // namespace tron
