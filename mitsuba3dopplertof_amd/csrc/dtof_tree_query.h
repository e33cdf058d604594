// dtof_tree_query.h -- launcher of the TLAS / BLAS ray query over arrays in every form a frame's ray kernels run it (dtof_tree_query.hip; dtof_tree_query of
// include/dtof.h).  Kept out of dtof_kernels.h like dtof_flat_query.h: only the host orchestration reads it, and the translation units of the render kernels do not
// change with it.
#pragma once
#include "dtof_kernels.h"

namespace dtof {

// The forms: the instantiations of trace_rays (dtof_traverse.h) that ray_shape() / launch_rays() of dtof_kernels.hip can select for k_trace (closest hit) and k_shadow
// (occlusion), each with the MESH value of that kernel, one wave per block, one ray per lane.
//   0  float nodes, 32-bit LDS stack of the scene's depth, every shape's code (MESH = 1) -- what k_ray_query (dtof_ray_intersect) carries
//   1  the eight-wave kernels: half-float nodes (H16), STRIDE = 64, kLdsStack8 LDS entries and the private overflow array, triangle and rectangle code only (MESH = 2)
//   2  form 1 with the TLAS nodes read from the block's copy in LDS (TL)
//   3  the DEFER pair of form 1: the lane runs trace_scene<..., DEFER>, which puts the meshes behind a BLAS aside, and then trace_deferred on its OWN candidate list with
//      the hit it holds.  These are the device functions of the two launches (k_trace + k_trace_deferred, k_shadow + k_shadow_deferred) WITHOUT what lies between them
//      in a frame: the hit record's round trip through the queue and the compaction of the rays that put something aside (defer_append), which decide which lane of
//      the second launch walks which ray and nothing about its result.
//   4  the six-wave kernels of a scene with a BLAS and analytic shapes: half-float nodes, STRIDE = 64, 32-bit LDS stack of the scene's depth, every shape's code
constexpr int kTreeQueryForms = 5;
struct TreeQueryScene { uint32_t stack_depth, n_tlas_nodes; bool has_nodes16, has_analytic; };
// nullptr if the scene meets the form, else the reason it does not (nothing is launched then)
const char *tree_query_refusal(int form, const TreeQueryScene &t);
// rays = o[3], d[3], time, maxt; closest hit: out3 = t, u, v (inf, 0, 0 on a miss), ids = object, shape in its group, primitive (-1 on a miss), three words per ray;
// occlusion: ids = 1 / 0, one word per ray.  Throws when the form is refused or the stack does not fit the LDS.
void launch_tree_query(const uint8_t *scene, const TreeQueryScene &t, int form, bool any, const float *rays, float *out3, int32_t *ids, uint32_t n, hipStream_t s);

}  // namespace dtof
