#pragma once
// dtof_zrow_mfma.h -- the z rows of the four plain rectangles of a five-rectangle one-wall table (the wall at index 2), computed on the matrix cores
// (DESIGN 8.3 (m)).  Every ray query of trace_flat starts with flat_zrow of each rectangle: three chained fmaf for the origin, a product and two fmaf for the
// direction, whose matrix-side operands are the same in all 64 lanes.  v_mfma_f32_4x4x1_16b_f32 computes inside each group of four lanes
//     D[i][j] = A(lane i) * B(lane j) + C[i][j]        lane j holds D[0..3][j] in four consecutive registers
// so with B = a component of the lane's own ray and A = a matrix entry of rectangle kZrowRect[lane & 3], lane j receives that entry times its own ray for all four
// rectangles, no cross-lane move.  Three dependent MFMAs are the three fmaf of one chain for the four rectangles at once: an f32 MFMA is a k-ordered fmaf chain with
// one rounding per product and keeps subnormals (tests/test_zrow_mfma.py holds the eight words to the oracle's operands in every bit).
//   origin     C = the rows' z3, then z0 * o.x, z1 * o.y, z2 * o.z                       = fmaf(z2, o.z, fmaf(z1, o.y, fmaf(z0, o.x, z3)))
//   direction  C = -0.0: fma(z0, d.x, -0.0) is z0 * d.x in every bit, signed zeros too    = fmaf(z2, d.z, fmaf(z1, d.y, z0 * d.x))
// An MFMA executes in all 64 lanes whatever EXEC says: the callers issue zrow_mfma from wave-uniform control flow with every lane's ray defined (a lane without a
// query may hold anything: a group's results depend on its own four lanes' rays and on the constants only).
#include "dtof_kernels.h"

#ifndef DTOF_ZROW_MFMA
#define DTOF_ZROW_MFMA 1   // 0: flat_zrow per rectangle from the z-row table, the text before (m)
#endif

namespace dtof {

constexpr bool zrow_mfma_shape(uint32_t facts) { return DTOF_ZROW_MFMA != 0 && pair_walk_shape(facts); }

typedef float ZrowF4 __attribute__((ext_vector_type(4)));
// slot s of the eight values is rectangle s + (s >> 1): 0, 1, 3, 4
constexpr uint32_t zrow_slot(uint32_t k) { return k < 2u ? k : k - 1u; }
// the matrix-side operands, per-lane constants of a kernel: z0, z1, z2 of the lane's rectangle and the four z3
struct ZrowOperands { float a0, a1, a2; ZrowF4 c; };
// the local z of a ray's origin (o) and direction (d) in the four plain rectangles: flat_zrow(...).x / .y of rectangle s + (s >> 1) in component s
struct ZrowQuad { ZrowF4 o, d; };
struct NoZrow {};   // (what a query without them is handed in their place)

// zt: the staged DFlatZ table of the five rectangles.  Call with every lane active.
__device__ __forceinline__ ZrowOperands zrow_operands(const uint4 *zt) {
    const uint32_t s = __lane_id() & 3u;
    const uint4 mine = zt[s + (s >> 1)];
    ZrowOperands r;
    r.a0 = __uint_as_float(mine.x); r.a1 = __uint_as_float(mine.y); r.a2 = __uint_as_float(mine.z);
    r.c = ZrowF4{ __uint_as_float(zt[0].w), __uint_as_float(zt[1].w), __uint_as_float(zt[3].w), __uint_as_float(zt[4].w) };
    return r;
}
// (The operands re-read from the stage in front of every query -- the lane's row and the four z3, 118 VGPRs instead of 126 -- were built behind the switch and measured
//  no faster than the parent: the reads and their waits are what the step removes.  profiles/zrow_mfma_ab.txt.  Removed.)
__device__ __forceinline__ ZrowQuad zrow_mfma(const ZrowOperands &m, float ox, float oy, float oz, float dx, float dy, float dz) {
    ZrowQuad r;
    r.o = __builtin_amdgcn_mfma_f32_4x4x1f32(m.a0, ox, m.c, 0, 0, 0);
    r.d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.a0, dx, ZrowF4{ -0.f, -0.f, -0.f, -0.f }, 0, 0, 0);
    r.o = __builtin_amdgcn_mfma_f32_4x4x1f32(m.a1, oy, r.o, 0, 0, 0);
    r.d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.a1, dy, r.d, 0, 0, 0);
    r.o = __builtin_amdgcn_mfma_f32_4x4x1f32(m.a2, oz, r.o, 0, 0, 0);
    r.d = __builtin_amdgcn_mfma_f32_4x4x1f32(m.a2, dz, r.d, 0, 0, 0);
    return r;
}
}  // namespace dtof
