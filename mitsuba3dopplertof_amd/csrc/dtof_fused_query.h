// dtof_fused_query.h -- launcher of the tree walk the FUSED shade kernels run themselves (k_shade's three trace_scene call sites), over arrays of rays
// (dtof_fused_query.hip; dtof_fused_query of include/dtof.h).  Kept out of dtof_kernels.h like dtof_tree_query.h: only the host orchestration reads it, and the
// translation units of the render kernels do not change with it.
#pragma once
#include "dtof_kernels.h"

namespace dtof {

// The forms: trace_scene<ANY, MESH, MEMO = true, SOA, STRIDE = the block size, S16, 0, false, RH16> as k_shade instantiates it, one ray per lane, behind what k_shade
// does around the call -- the SceneView, the lane's instance-memo column in the layout of ShadeLds filled at the lane's ray time, the lane's stack column.
//   0  classic           one wave per block, float nodes from the blob (staged in LDS when launch_shade would stage it, else in global memory), every shape's code
//   1  classic_rect      form 0 with MESH = 0: rectangle code only
//   2  resident          blocks of `waves` waves; the resident stage (four SOA planes of kResNodes node pieces + the record block in LDS), 32-bit stack columns
//   3  resident_16       form 2 with S16: child references re-encoded to 16 bits while they are copied, 16-bit stack columns at a halfword address
//   4  resident_half     form 2 with RH16: two planes of DNode16 pieces (a TLAS of kResidentNodes + 1 .. 2 * kResidentNodes nodes)
//   5  resident_half_16  form 4 with S16
constexpr int kFusedQueryForms = 6;
struct FusedQueryScene {
    uint32_t scene_bytes, stack_depth, n_nodes, n_objects, small_off, small_words, memo_obj;   // memo_obj: flat_choice's (exactly one instance), else 0xffffffff
    bool has_tris, has_blas, has_nodes16, resident_layout, only_rects;
};
// the dynamic LDS of a form's launch: ShadeLds::classic / ShadeLds::resident up to and including the stack columns (the query has no park columns); stage_words of the
// classic forms is 0 when the blob is read from global memory
uint32_t fused_query_stage_words(const FusedQueryScene &t);
uint32_t fused_query_lds(int form, uint32_t waves, const FusedQueryScene &t);
// empty if the scene meets (form, waves) within lds_limit bytes of LDS (device_lds_limit()), else the reason it does not (nothing is launched then)
std::string fused_query_refusal(int form, uint32_t waves, const FusedQueryScene &t, uint32_t lds_limit);
// rays = o[3], d[3], time, maxt; the answers in dtof_tree_query's layout: closest hit: out3 = t, u, v (inf, 0, 0 on a miss), ids = object, shape in its group, primitive
// (-1 on a miss), three words per ray; occlusion: ids = 1 / 0, one word per ray.  The caller has asked fused_query_refusal.
void launch_fused_query(const uint8_t *scene, const FusedQueryScene &t, int form, uint32_t waves, bool any, const float *rays, float *out3, int32_t *ids, uint32_t n, hipStream_t s);

}  // namespace dtof
