// dtof_surface_query.h -- launcher of the surface-interaction fill over arrays of hits (dtof_surface_query.hip; dtof_surface_eval of include/dtof.h).  Kept out of
// dtof_kernels.h like dtof_flat_query.h: only the host orchestration reads it, and the translation units of the render kernels do not change with it.
#pragma once
#include "dtof_kernels.h"

namespace dtof {

// The forms: the instantiations and argument patterns of compute_surface (dtof_shading.h) a frame's kernels run
//   0  <MESH = true>, the overload without a memo (k_ray_query, k_aov, k_shade's mesh kernels of a scene without a memo object)
//   1  <false>, no memo                                   (k_shade's rectangle-only kernels of a scene without a memo object)
//   2  <false>, use_memo, matrix and inverse from the register arrays instance_memo_fill returned; the inverse read back from the lane's LDS column
//   3  <false>, use_memo, both read back from the lane's two LDS columns (SceneView::memo_m: the flat scenes' kernels)
//   4  <false, kFactOneWall> with the WallFrames of wall_frames_init / wall_frames_fill (the one-wall kernels)
//   5  <true>, use_memo, from the register arrays (k_shade's fused mesh kernels of a scene with ONE instance)
constexpr int kSurfaceForms = 6;
constexpr uint32_t kSurfaceIn = 10, kSurfaceOut = 32;   // o[3], d[3], time, t, b1, b2 | p, n, sh_n, sh_s, sh_t, wi, u, v, dp_du, dp_dv, offset_p(si, d), offset_p(si, -d)
struct SurfaceQueryScene { uint32_t scene_bytes, flat_off, flat_objects, memo_obj; };   // memo_obj: the scene's only instance or 0xffffffff; the flat table of form 4
// One hit per lane, blocks of one wave.  ids3 = object, shape in its group, primitive in the BLAS's order (Hit::prim), all in range (dtof_surface_eval checks them).
// Forms 1 to 4 stage the blob in LDS as k_shade's rectangle-only kernels do and throw when it does not fit.
void launch_surface_query(const uint8_t *scene, const SurfaceQueryScene &q, int form, bool want_frame, const float *in10, const int32_t *ids3, float *out32, uint32_t n, hipStream_t s);

}  // namespace dtof
