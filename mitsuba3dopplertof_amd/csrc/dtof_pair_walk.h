#pragma once
// dtof_pair_walk.h -- the merge of trace_flat's pair form (dtof_traverse.h): the closest-hit walk of a five-rectangle one-wall table (the wall at
// index 2) whose two lanes 2k and 2k + 1 hold the SAME ray (o, d, maxt) and differ in their time only, which reaches the wall alone.  The even lane walks the
// rectangles below the wall (0, 1), the odd lane those above it (3, 4), each visits the wall with its own ray.  Plain C++, so that a host program
// (tests/pair_walk_check.cpp) can check the merge against the walk it replaces.
//
// The walk it replaces visits 0, 1, 2, 3, 4 and takes a rectangle when `hit && t < best.t` (flat_best_take), best.t starting at maxt.  Its result is the smallest t
// among the rectangles with `hit && t < maxt`, the lowest index among equal t: a rectangle is taken over an earlier one only when strictly nearer, and one that
// was taken is never nearer than the result.  (A NaN t never hits: `t >= 0` is false.)
//
// The pair form reaches the same result in three ascending segments:
//   lower   the even lane's walk over 0, 1 from (maxt, none) is the walk's state after its first two visits, bit for bit: same ray, same operations.
//   wall    each lane takes the lower state (a copy of the even lane's registers) and runs the wall's visit on it with its own ray -- the walk's third visit.
//   upper   the odd lane's walk over 3, 4 from (maxt, none) holds U = the nearest of {3, 4} with `hit && t < maxt`, the lower index at equal t, or (maxt, none).
//           The walk's visits of 3 and 4 on a state S with S.t <= maxt end in U if U.t < S.t and in S otherwise: if U is none, U.t = maxt is not below S.t and
//           neither visit takes (a candidate t < S.t <= maxt would have been taken by the odd lane too); if U.t < S.t the walk takes 3 when 3 is U, and then 4 only
//           when strictly nearer -- that is when 4 is U; if U.t >= S.t no candidate is below S.t.  pair_merge_upper is that one compare.
// S.t <= maxt holds because every taken t is below the t it replaces.  (maxt = NaN: nothing hits, every state is (NaN, none) and no compare is true.)
#include <stdint.h>

#ifndef DTOF_HD
#if defined(__HIP__)
#define DTOF_HD __host__ __device__ __forceinline__
#else
#define DTOF_HD inline
#endif
#endif

namespace dtof {

struct FlatBest { float t, u, v; uint32_t obj; };

// one visit of the walk: trace_flat's `take`, operation for operation
DTOF_HD void flat_best_take(FlatBest &b, bool hit, float t, float u, float v, uint32_t oi) {
    const bool take = (int) hit & (int) (t < b.t);
    b.t = take ? t : b.t; b.u = take ? u : b.u; b.v = take ? v : b.v; b.obj = take ? oi : b.obj;
}
// the upper segment's result onto the state behind the wall's visit
DTOF_HD void pair_merge_upper(FlatBest &b, const FlatBest &upper) {
    const bool take = upper.t < b.t;
    b.t = take ? upper.t : b.t; b.u = take ? upper.u : b.u; b.v = take ? upper.v : b.v; b.obj = take ? upper.obj : b.obj;
}

}  // namespace dtof
