// div_unscaled.h -- a CANDIDATE, included by no kernel: a / b as the reciprocal + multiply-add chain of the compiler's IEEE division without its two
// v_div_scale, its v_div_fmas and its v_div_fixup (~24 cycles against ~40).  tests/math_sweep.hip carries it in the candidate slot of its `div`
// case (-DDTOF_SWEEP_CANDIDATE); profiles/math_sweep_div_candidate.txt is the class table measured with it, and div_unscaled_safe below is the operand window
// in which that table shows no mismatch against the correctly rounded quotient.  A fast path that wants to ship has to meet the same table.
#pragma once
#include "dtof_math.h"

namespace dtof {

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float div_unscaled(float a, float b) {
    const float r0 = __builtin_amdgcn_rcpf(b);              // 1 ulp
    const float e0 = fmaf(-b, r0, 1.0f), r = fmaf(e0, r0, r0);
    const float q0 = a * r;
    const float e1 = fmaf(-b, q0, a), q1 = fmaf(e1, r, q0);
    const float e2 = fmaf(-b, q1, a);
    return fmaf(e2, r, q1);
}
#else
inline float div_unscaled(float a, float b) { return a / b; }   // the builtin exists on the device only; the candidate slot never runs on the host
#endif

// The window the class table claims to be safe, in unbiased exponents of two NORMAL, finite operands: the reciprocal stays normal (|eb| <= 125), the quotient
// stays clear of overflow and of the denormal range by the 25 bits its residual correction needs (-100 <= ea - eb <= 125), and so does the residual of a itself
// (ea >= -100).
// div_unscaled_violations names the conditions an operand pair breaks (the sweep reports the mismatches that break exactly one, and how close to the bound they come).
enum { DIVU_B_LARGE = 1, DIVU_B_SMALL = 2, DIVU_A_SMALL = 4, DIVU_Q_SMALL = 8, DIVU_Q_LARGE = 16 };
DTOF_HD constexpr int div_unscaled_violations(int ea, int eb) {
    return (eb > 125 ? DIVU_B_LARGE : 0) | (eb < -125 ? DIVU_B_SMALL : 0) | (ea < -100 ? DIVU_A_SMALL : 0) | (ea - eb < -100 ? DIVU_Q_SMALL : 0) | (ea - eb > 125 ? DIVU_Q_LARGE : 0);
}
DTOF_HD constexpr bool div_unscaled_safe(int ea, int eb) { return div_unscaled_violations(ea, eb) == 0; }

}  // namespace dtof
