// twilight_amd/csrc/talco_div.hip.h -- the hoisted-reciprocal form of the IEEE fp32 division of talco_lean_kernel (talco_nuc.hip.h) and the
// guard that keeps its operands in the range where both forms give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace twl {

// n / d for a divisor that is fixed for the whole pair.  `r` is the refined reciprocal fma(fma(-d, rcp(d), 1), rcp(d), rcp(d)).
// This is the instruction sequence the compiler emits for an IEEE fp32 division (v_div_scale, v_rcp, 4 fma, v_div_fmas,
// v_div_fixup) with the parts that depend on d alone hoisted and the scaling steps left out.  v_div_scale rescales only when
// d or n/d is near the ends of the exponent range or |n| < 2^-103, and v_div_fixup only patches zeros, infinities and NaNs,
// so for 1 <= d <= 2^40 and n == 0 or 2^-73 <= |n| <= 2^80 both give the same bits (a zero quotient may differ in sign, which
// no comparison or sum downstream can see).  Three guards keep the kernels inside that range: a profile entry is zero or
// 2^-20 <= |x| <= 2^30 (div_guard_bad below), the denominator float(refNum) * float(qryNum) lies in [1, 2^40] (talco_lean_kernel,
// in front of the first tile), every score and gap_char is zero or within [2^-10, 2^10] (fast_div_in_range, twl_policy.inc.hip:
// anything else plans the IEEE-division kernels from the start).  The smallest non-zero product inside them is 2^-50, whose ulp
// is the 2^-73 above.  A pair outside the first two ends with err = kErrGuard and is re-run on the IEEE-division kernel
// (climb_ladder, Rung::Guard); a tile that also outgrew its window reports that first.  tests/test_gpu_div_edges.py compares the
// two forms bit for bit on device, through the DUMP instantiation of talco_lean_kernel, with operands on every one of these limits.
__device__ __forceinline__ float fast_div(float n, float d, float r)
{
    const float q0 = n * r;
    const float t0 = __builtin_fmaf(-d, q0, n);
    const float q1 = __builtin_fmaf(t0, r, q0);
    const float t1 = __builtin_fmaf(-d, q1, n);
    return __builtin_fmaf(t1, r, q1);
}
__device__ __forceinline__ float refined_rcp(float d)
{
    const float r0 = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, r0, 1.0f);
    return __builtin_fmaf(e, r0, r0);
}
// a profile entry fast_div's guard accepts: zero, or 2^-20 <= |x| <= 2^30
__device__ __forceinline__ bool div_guard_bad(float x)
{
    const float ax = __builtin_fabsf(x);
    return (x != 0.0f) && !(ax >= 9.5367431640625e-07f && ax <= 1073741824.0f);
}

}  // namespace twl
