#pragma once
// dtof_flat_cull.h -- the "certain miss" test trace_flat (dtof_traverse.h) puts in front of each rectangle test: whether the z row of the rectangle's world -> object
// matrix alone proves that the ray misses it.  Plain C++ over <math.h>, so that a host program (tests/test_flat_cull.py) can check it against the test's arithmetic.
//
// The rectangle test (rect_hit, trace_flat's test) computes zx, zy = the local z of the ray's origin and direction, then
//     t = RN(-zx / zy),  hit = t >= 0 && t <= maxt && |u| <= 1 && |v| <= 1.
// flat_certain_miss(zx, zy, far) is true only if `t >= 0 && t <= maxt` is false, whatever u and v are.  With the exact (real) values
//     near = zx - 2^-100 zy = -zy (t* + 2^-100),   beyond = zx + far zy = zy (far - t*),   t* = -zx / zy,
// near * beyond = zy^2 (t* + 2^-100) (t* - far) is positive exactly when t* < -2^-100 (t rounds to a negative number: |t*| is far above the denormals, no -0) or
// t* > far (then t = RN(t*) >= far > maxt: RN is monotonic and `far` is a float).  The two multiply-adds are rounded once each, so a nonzero result has the sign of its
// exact value; a product that is positive after rounding has two nonzero factors of equal sign.  Everything else -- a factor that rounds to 0, a product that underflows,
// infinities of opposite sign, NaN -- compares false and goes to the full test.  zy = +-0 with a finite `far`: near = beyond = zx, and a nonzero zx gives t = +-inf,
// below 0 or above the finite maxt.  zy = +-inf: near and beyond are infinities of opposite sign (far > 0), never a positive product.
#include <math.h>

#ifndef DTOF_HD
#if defined(__HIP__)
#define DTOF_HD __host__ __device__ __forceinline__
#else
#define DTOF_HD inline
#endif
#endif

namespace dtof {

// A float strictly above maxt for every maxt >= -0 (maxt * (1 + 2^-20) rounds above maxt in the normal range; 2^-100 lifts the denormals, 0 and -0); inf for maxt
// near the largest float or inf, which switches the "beyond" half off.  For maxt < 0 no t passes `t >= 0 && t <= maxt`, so any value is sound.
DTOF_HD float flat_cull_far(float maxt) { return fmaf(maxt, 0x1.00001p0f, 0x1p-100f); }

DTOF_HD bool flat_certain_miss(float zx, float zy, float far) {
    const float near = fmaf(-0x1p-100f, zy, zx), beyond = fmaf(far, zy, zx);
    return near * beyond > 0.f;
}

}  // namespace dtof
