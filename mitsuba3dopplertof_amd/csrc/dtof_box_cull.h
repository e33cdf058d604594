#pragma once
// dtof_box_cull.h -- the slab test of the TLAS / BLAS walks (dtof_traverse.h: trace_scene, intersect_object, node_step).  Plain C++ over <math.h>, so that a host
// program (tests/box_cull_check.cpp, built and run by tests/test_box_cull.py) can hold the very functions the kernels call to their contract.
//
// A plane at coordinate b is crossed at t = b * id - o * id: ONE multiply-add per plane with `noid` = -(o * id) computed once per ray (the difference-then-product form
// costs two instructions per plane, 12 more per node step of an issue-bound traversal).  The test only culls -- which primitive is hit, and where, is decided by the
// primitive tests -- so it has to be CONSERVATIVE, not equal to anything:
//
//     whenever the exact ray o + t d meets the UNPADDED box at some t0 in [0, tbest], box_hit returns true.
//
// The bound behind it.  With id = (1 / d)(1 + e1), noid = -(o id)(1 + e2) and the multiply-add's own rounding (1 + e3), a plane's computed distance is
//     fma(b, id, noid) = t* (1 + e1)(1 + e3) - o id e2 (1 + e3),   t* = (b - o) / d,   |e1| <= 2^-23 (v_rcp_f32: one ulp), |e2|, |e3| <= 2^-24,
// so its error is at most |id| (1.5 * 2^-23 |b - o| + 2^-24 |o|)(1 + 2^-22) <= 2^-22 |t*| (1 + 2^-22) + 2^-24 |b| |id| (1 + 2^-22).  The second term is what the host's
// padding pays for: every box is grown by (1e-5 max(|b|, extent) + 1e-6) |id| in t (scene_build.cpp: Box::pad; the half-float boxes are rounded outwards on top), 160
// times 2^-24 |b| |id|.  The first term grows with the distance between the origin and the box and no padding of the box bounds it: a small object seen from far away
// lost the rays through its rim.  It is RELATIVE to t, and so is its cure: at a true crossing t0 every near plane computes at most t0 (1 + 2^-22)(1 + 2^-22) and every
// far plane at least t0 (1 - 2^-22 (1 + 2^-22)), and tbest >= t0, so
//     tn <= tf * (1 + 2^-22)^2 / (1 - 2^-22 (1 + 2^-22)) < tf * (1 + 2^-21 + 2^-42 ...),
// which kSlabWiden = 1 + 3 * 2^-22 covers together with the rounding of the product tf * kSlabWiden itself (2^-24).  tf < 0 means there is no t0 >= 0 at all.
//
// Direction components below kSlabMinDir in magnitude (exact zeros, denormals, 1e-38) are replaced by +-kSlabMinDir: their reciprocal overflows, or o * id does, the
// plane distances become -inf and +inf - inf, and a ray that stays inside the slab for its whole length was culled.  With the replacement the slab of such an axis spans
// at least [-(padding) / kSlabMinDir, +(padding) / kSlabMinDir] around an origin inside the unpadded slab, and the padding is at least 1e-6.
//
// DOMAIN of the contract:
//     |o| <= 3e8 (o * id stays finite with |id| <= 1e30),   t0 <= 1e24 (= 1e-6 / kSlabMinDir),   no plane distance in the denormal range (|b - o| |id| >= 2^-126 or 0).
// Outside it -- origins at 1e30, directions of length 1e-30 -- and for NaN / infinite rays the test may cull; NaNs fall out of the min / max chain (fminf / fmaxf return
// the other operand) and a box whose test has no number left is missed.
#include <math.h>

#ifndef DTOF_HD
#if defined(__HIP__)
#define DTOF_HD __host__ __device__ __forceinline__
#else
#define DTOF_HD inline
#endif
#endif

namespace dtof {

constexpr float kSlabMinDir = 1e-30f;
constexpr float kSlabWiden = 0x1.000006p0f;   // 1 + 3 * 2^-22

struct SlabV { float x, y, z; };
struct SlabRay { SlabV id, noid; };

// Reciprocal for the slab test only: v_rcp_f32 (one ulp) on the device.  On the host 1.f / x; DTOF_SLAB_RCP_ULPS = +-1 moves it one ulp either way (the host check
// runs the contract with all three).
DTOF_HD float slab_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    float r = 1.f / x;
#ifdef DTOF_SLAB_RCP_ULPS
    if (r != 0.f && r - r == 0.f) r = nextafterf(r, DTOF_SLAB_RCP_ULPS > 0 ? (r > 0.f ? INFINITY : -INFINITY) : 0.f);
#endif
    return r;
#endif
}
DTOF_HD float slab_dir(float d) { return fabsf(d) < kSlabMinDir ? copysignf(kSlabMinDir, d) : d; }   // (NaN compares false and stays)
DTOF_HD SlabRay slab_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    SlabRay r;
    r.id.x = slab_rcp(slab_dir(dx)); r.id.y = slab_rcp(slab_dir(dy)); r.id.z = slab_rcp(slab_dir(dz));
    r.noid.x = -(ox * r.id.x); r.noid.y = -(oy * r.id.y); r.noid.z = -(oz * r.id.z);
    return r;
}
DTOF_HD bool box_hit(const float *bmin, const float *bmax, const SlabRay &r, float tbest, float &tn) {
    const float tx0 = fmaf(bmin[0], r.id.x, r.noid.x), tx1 = fmaf(bmax[0], r.id.x, r.noid.x);
    const float ty0 = fmaf(bmin[1], r.id.y, r.noid.y), ty1 = fmaf(bmax[1], r.id.y, r.noid.y);
    const float tz0 = fmaf(bmin[2], r.id.z, r.noid.z), tz1 = fmaf(bmax[2], r.id.z, r.noid.z);
    tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.f));
    const float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), tbest));
    return tn <= tf * kSlabWiden;
}

}  // namespace dtof
