// dtof_fused_query.hip -- trace_scene (dtof_traverse.h) over arrays of rays in the instantiations the FUSED shade kernels carry (k_shade's three call sites), each behind
// what k_shade does around the call -- the SceneView (staged, global or the resident stage's), the lane's instance-memo column in the layout of ShadeLds filled at the
// lane's ray time, the lane's stack column (32-bit, or 16-bit at a halfword address) -- and nothing else.  A translation unit of its own: the render kernels' units do
// not see it, their code objects stay what they were.
#include "dtof_device.h"
#include "dtof_fused_query.h"

namespace dtof {

template <bool ANY>
DTOF_D void fused_query_store(const SceneView &sv, bool found, const Hit &h, uint32_t i, float *out3, int32_t *ids) {
    if (ANY) { ids[i] = found ? 1 : 0; return; }
    float *w = out3 + (size_t) i * 3;
    int32_t *q = ids + (size_t) i * 3;
    q[0] = found ? (int32_t) h.obj : -1; q[1] = found ? (int32_t) h.shape : -1; q[2] = found ? (int32_t) hit_prim_index(sv, h) : -1;
    w[0] = found ? h.t : u2f(0x7f800000u); w[1] = found ? h.u : 0.f; w[2] = found ? h.v : 0.f;
}

// k_shade<LDS = STAGED, MODE != 0, ..., MESH, ..., RESW = 0>: one wave per block, dynamic LDS = [staged blob][memo column][stack column] (ShadeLds::classic)
template <bool STAGED, int MESH, bool ANY>
__global__ __launch_bounds__(kShadeBlock) void k_fused_query_classic(const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t memo_obj,
                                                                      const float *rays, float *out3, int32_t *ids, uint32_t n) {
    extern __shared__ uint4 lds[];
    constexpr uint32_t memo_words = kMemoWords * kMemoStride;
    uint32_t *stack = (uint32_t *) (lds + stage_words) + memo_words + threadIdx.x;
    const uint8_t *base = STAGED ? stage_scene(scene, scene_bytes, lds) : scene;
    SceneView sv = make_view(base);
    sv.memo_obj = memo_obj; sv.memo = (float *) (lds + stage_words) + threadIdx.x; sv.memo_m = false;
    const uint32_t i = blockIdx.x * kShadeBlock + threadIdx.x;
    if (i >= n) return;   // (behind the stage's barrier)
    const float *r = rays + (size_t) i * 8;
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const float time = r[6], maxt = r[7];
    float memo_m[12], memo_inv[12];
    if (sv.memo_obj != 0xffffffffu) instance_memo_fill(sv, time, memo_m, memo_inv);
    Hit h;
    const bool found = trace_scene<ANY, MESH, true, false, kShadeBlock>(sv, stack, o, d, time, maxt, h);
    fused_query_store<ANY>(sv, found, h, i, out3, ids);
}

// The resident stage's fill, RESTATED from k_shade (dtof_shade.h, `if (RESW)` in front of the segment loop): every thread of the block copies the node planes -- child
// references through encode_child16 under S16 -- and the record block, ONE barrier, and the view's node and record pointers resolve into LDS.  (As one device function
// of dtof_traverse.h that k_shade calls too, by value and by reference, the 49 resident k_shade kernels kept their resource figures and changed one or two scalar
// instructions of their prologues -- the kernarg loads of res_small_off / res_small_words pair differently -- so k_shade keeps its text and this is a copy: DESIGN 3.)
template <bool S16, bool RH16>
DTOF_D SceneView resident_stage_fill(const uint8_t *scene, uint32_t small_off, uint32_t small_words, uint4 *lds) {
    const BlobHeader *gh = (const BlobHeader *) scene;
    if (RH16) {   // two planes of 2 * kResNodes 16-byte pieces: (left box, left child) | (right box, right child)
        const uint4 *gn = (const uint4 *) (scene + gh->off_nodes16);
        const uint32_t n_pieces = gh->n_nodes * 2u;
        for (uint32_t i = threadIdx.x; i < n_pieces; i += blockDim.x) {
            uint4 piece = gn[i];
            if (S16) piece.w = encode_child16(piece.w);
            lds[(i & 1u) * (2u * kResNodes) + (i >> 1)] = piece;
        }
    } else {
        const uint4 *gn = (const uint4 *) (scene + gh->off_nodes);
        const uint32_t n_pieces = gh->n_nodes * 4u;
        for (uint32_t i = threadIdx.x; i < n_pieces; i += blockDim.x) {
            uint4 piece = gn[i];
            if (S16 && (i & 3u) < 2u) piece.w = encode_child16(piece.w);   // left / right child: 16-bit references, so that the stack columns are 16-bit
            lds[(i & 3u) * kResNodes + (i >> 2)] = piece;
        }
    }
    const uint4 *gs = (const uint4 *) (scene + small_off);
    for (uint32_t i = threadIdx.x; i < small_words; i += blockDim.x) lds[4u * kResNodes + i] = gs[i];
    __syncthreads();
    const uint8_t *small = (const uint8_t *) (lds + 4u * kResNodes) - small_off;   // blob offsets of the copied block resolve into LDS
    SceneView sv = make_view(scene);
    sv.nodes = (const DNode *) lds; sv.nodes16 = (const DNode16 *) lds;
    sv.groups = (const DGroup *) (small + gh->off_groups); sv.shapes = (const DShape *) (small + gh->off_shapes);
    sv.tris = (const DTri *) (small + gh->off_tris); sv.shading = (const DTriShade *) (small + gh->off_shading);
    sv.isect = (const DTriIsect *) (small + gh->off_isect);
    sv.emitters = (const DEmitter *) (small + gh->off_emitters);
    return sv;
}

// k_shade<..., RESW = WAVES, RH16> with S16 = (several films): blocks of WAVES waves, dynamic LDS = [node planes | record block][a memo column per wave, if the scene
// has a memo object][stack columns] (ShadeLds::resident without its park columns)
template <int WAVES, bool S16, bool RH16, bool ANY>
__global__ __launch_bounds__(WAVES * 64, WAVES / 4) void k_fused_query_resident(const uint8_t *scene, uint32_t small_off, uint32_t small_words, uint32_t res_memo, uint32_t memo_obj,
                                                                                const float *rays, float *out3, int32_t *ids, uint32_t n) {
    extern __shared__ uint4 lds[];
    constexpr uint32_t kStackStride = WAVES * 64;
    const uint32_t lane_id = threadIdx.x & 63u, wave_id = threadIdx.x >> 6;
    const uint32_t stage_words = 4u * kResNodes + small_words;
    const uint32_t memo_words = res_memo ? WAVES * kMemoWords * kMemoStride : 0u;
    // the resident kernels of several films: 16-bit columns, the halfword address in a uint32_t * (only trace_scene<SOA> / node_step<SOA> touch it)
    uint32_t *stack = S16 ? (uint32_t *) ((uint16_t *) ((uint32_t *) (lds + stage_words) + memo_words) + threadIdx.x) : (uint32_t *) (lds + stage_words) + memo_words + threadIdx.x;
    SceneView sv = resident_stage_fill<S16, RH16>(scene, small_off, small_words, lds);
    sv.memo_obj = memo_obj; sv.memo = (float *) (lds + stage_words) + wave_id * kMemoWords * kMemoStride + lane_id; sv.memo_m = false;
    const uint32_t i = blockIdx.x * kStackStride + threadIdx.x;
    if (i >= n) return;   // (behind the stage's barrier)
    const float *r = rays + (size_t) i * 8;
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const float time = r[6], maxt = r[7];
    float memo_m[12], memo_inv[12];
    if (sv.memo_obj != 0xffffffffu) instance_memo_fill(sv, time, memo_m, memo_inv);
    Hit h;
    const bool found = trace_scene<ANY, 1, true, true, kStackStride, S16, 0u, false, RH16>(sv, stack, o, d, time, maxt, h);
    fused_query_store<ANY>(sv, found, h, i, out3, ids);
}

// launch_shade's choice for a classic fused launch: the blob is staged if it is at most 16 KiB and fits a block's 64 KiB beside the columns
uint32_t fused_query_stage_words(const FusedQueryScene &t) {
    const uint32_t w = (t.scene_bytes + 15u) / 16u;
    return t.scene_bytes <= 16u * 1024u && w * 16u + ShadeLds::classic(0u, true, false, t.stack_depth).bytes() + 64u <= 64u * 1024u ? w : 0u;
}
uint32_t fused_query_lds(int form, uint32_t waves, const FusedQueryScene &t) {
    if (form < 2) return ShadeLds::classic(fused_query_stage_words(t), true, false, t.stack_depth).bytes();
    const ShadeLds l = ShadeLds::resident(t.small_words, waves, t.memo_obj != 0xffffffffu, form == 3 || form == 5, t.stack_depth);
    return l.stage + l.memo + l.stack;
}

std::string fused_query_refusal(int form, uint32_t waves, const FusedQueryScene &t, uint32_t lds_limit) {
    if (form < 0 || form >= kFusedQueryForms) return "form must be 0 (classic), 1 (classic_rect), 2 (resident), 3 (resident_16), 4 (resident_half) or 5 (resident_half_16)";
    if (t.n_nodes == 0) return "the scene has no TLAS";
    if (form < 2) {
        if (form == 1 && !t.only_rects) return "the classic_rect form carries rectangle code only and the scene has another shape kind";
        if (fused_query_lds(form, 0u, t) + 64u > 64u * 1024u) return "the BVH of this scene is too deep for the LDS traversal stack";
        return "";
    }
    if (waves != 8 && waves != 12 && waves != 16) return "waves must be 8, 12 or 16 for the resident forms";
    if (!t.resident_layout) return "the scene's blob has no resident layout (larger than 16 KiB, its record block within 24 KiB)";
    if (!t.has_tris || t.has_blas) return "the resident stage is for scenes with mesh code and no mesh behind a BLAS";
    const bool half = form >= 4, s16 = form == 3 || form == 5;
    if (!half && t.n_nodes > kResidentNodes) return "the scene has more than " + std::to_string(kResidentNodes) + " nodes: the float planes of the resident stage do not hold them";
    if (half && !(t.has_nodes16 && t.n_nodes > kResidentNodes && t.n_nodes <= 2 * kResidentNodes))
        return "the half-float planes are for scenes with half-float nodes and " + std::to_string(kResidentNodes + 1) + " to " + std::to_string(2 * kResidentNodes) + " nodes";
    // (plan_frame's bound: `(res_half || several films) && n_objects >= 0x7fff` -- the half-float stage of one film included)
    if ((s16 || half) && t.n_objects >= 0x7fffu) return "the 16-bit child references and the half-float planes are for scenes of fewer than 0x7fff objects";
    const uint32_t lds = fused_query_lds(form, waves, t);
    if (lds > lds_limit) return "the resident stage with its columns takes " + std::to_string(lds) + " bytes of LDS at " + std::to_string(waves) + " waves, the limit is " + std::to_string(lds_limit);
    return "";
}

template <bool STAGED, int MESH>
static void launch_classic(bool any, uint32_t grid, uint32_t lds, hipStream_t s, const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t memo_obj,
                           const float *rays, float *out3, int32_t *ids, uint32_t n) {
    if (any) hipLaunchKernelGGL((k_fused_query_classic<STAGED, MESH, true>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, memo_obj, rays, out3, ids, n);
    else hipLaunchKernelGGL((k_fused_query_classic<STAGED, MESH, false>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, memo_obj, rays, out3, ids, n);
}
template <int WAVES, bool S16, bool RH16>
static void launch_resident_kind(bool any, uint32_t lds, hipStream_t s, const uint8_t *scene, const FusedQueryScene &t, const float *rays, float *out3, int32_t *ids, uint32_t n) {
    const uint32_t block = WAVES * 64, grid = (n + block - 1u) / block, res_memo = t.memo_obj != 0xffffffffu ? 1u : 0u;
    // the dynamic LDS of a resident launch lies above the 64 KiB a kernel gets without asking
    const void *kernel = any ? (const void *) k_fused_query_resident<WAVES, S16, RH16, true> : (const void *) k_fused_query_resident<WAVES, S16, RH16, false>;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess) throw std::runtime_error("dtof_fused_query: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    if (any) {
        hipLaunchKernelGGL((k_fused_query_resident<WAVES, S16, RH16, true>), dim3(grid), dim3(block), lds, s, scene, t.small_off, t.small_words, res_memo, t.memo_obj, rays, out3, ids, n);
    } else {
        hipLaunchKernelGGL((k_fused_query_resident<WAVES, S16, RH16, false>), dim3(grid), dim3(block), lds, s, scene, t.small_off, t.small_words, res_memo, t.memo_obj, rays, out3, ids, n);
    }
}
template <int WAVES>
static void launch_resident(int form, bool any, uint32_t lds, hipStream_t s, const uint8_t *scene, const FusedQueryScene &t, const float *rays, float *out3, int32_t *ids, uint32_t n) {
    switch (form) {
        case 2: launch_resident_kind<WAVES, false, false>(any, lds, s, scene, t, rays, out3, ids, n); break;
        case 3: launch_resident_kind<WAVES, true, false>(any, lds, s, scene, t, rays, out3, ids, n); break;
        case 4: launch_resident_kind<WAVES, false, true>(any, lds, s, scene, t, rays, out3, ids, n); break;
        default: launch_resident_kind<WAVES, true, true>(any, lds, s, scene, t, rays, out3, ids, n); break;
    }
}

void launch_fused_query(const uint8_t *scene, const FusedQueryScene &t, int form, uint32_t waves, bool any, const float *rays, float *out3, int32_t *ids, uint32_t n, hipStream_t s) {
    if (!n) return;
    const uint32_t lds = fused_query_lds(form, waves, t);
    if (form < 2) {
        const uint32_t sw = fused_query_stage_words(t), grid = (n + kShadeBlock - 1u) / kShadeBlock;
        if (sw) {
            if (form == 0) launch_classic<true, 1>(any, grid, lds, s, scene, t.scene_bytes, sw, t.memo_obj, rays, out3, ids, n);
            else launch_classic<true, 0>(any, grid, lds, s, scene, t.scene_bytes, sw, t.memo_obj, rays, out3, ids, n);
        } else {
            if (form == 0) launch_classic<false, 1>(any, grid, lds, s, scene, t.scene_bytes, sw, t.memo_obj, rays, out3, ids, n);
            else launch_classic<false, 0>(any, grid, lds, s, scene, t.scene_bytes, sw, t.memo_obj, rays, out3, ids, n);
        }
        return;
    }
    if (waves == 8) launch_resident<8>(form, any, lds, s, scene, t, rays, out3, ids, n);
    else if (waves == 12) launch_resident<12>(form, any, lds, s, scene, t, rays, out3, ids, n);
    else launch_resident<16>(form, any, lds, s, scene, t, rays, out3, ids, n);
}

}  // namespace dtof
