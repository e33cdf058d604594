// dtof_flat_query.hip -- trace_flat (dtof_traverse.h) over arrays of rays: the instantiations the shade kernels of flat scenes carry, each behind what k_shade does
// around the call -- the blob staged in LDS, the lane's instance-memo column in the layout of ShadeLds, the memo filled at the lane's ray time -- and nothing else.
// A translation unit of its own: the render kernels' units do not see it, their code objects stay what they were.
#include "dtof_device.h"
#include "dtof_flat_query.h"

namespace dtof {

static_assert(kHeadlineShapeFacts == 0 || (flat_query_facts(2) & kFactFlatShape) != 0, "form 2 is the shaped walk");

template <bool ANY, uint32_t FACTS, bool PAIR_RAYS>
DTOF_D void flat_query_lane(const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t flat_off, uint32_t flat_objects,
                            uint32_t memo_obj, const float *rays, float *out3, int32_t *ids, uint32_t n) {
    extern __shared__ uint4 lds[];
    constexpr bool F_ONE_WALL = (FACTS & kFactOneWall) != 0;
    const uint8_t *base = stage_scene(scene, scene_bytes, lds);
    SceneView sv = make_view(base);
    // k_shade, fused: the memo column behind the stage, word k of this thread at memo[k * kMemoStride]; a flat scene with a memo object keeps the matrix there too (memo_m_lds)
    const bool have_memo = F_ONE_WALL || memo_obj != 0xffffffffu;
    sv.memo_obj = memo_obj; sv.memo = (float *) (lds + stage_words) + threadIdx.x; sv.memo_m = have_memo;
    const uint32_t i = blockIdx.x * kShadeBlock + threadIdx.x;
    if (i >= n) return;   // (behind the stage's barrier)
    const float *r = rays + (size_t) i * 8;
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const float time = r[6], maxt = r[7];
    float memo_m[12], memo_inv[12];
    if (have_memo) instance_memo_fill(sv, time, memo_m, memo_inv);
    Hit h;
    const bool found = trace_flat<ANY, true, FACTS, PAIR_RAYS>(sv, (ConstBytes) scene + flat_off, flat_off, flat_objects, nullptr, o, d, time, maxt, h);
    if (ANY) { ids[i] = found ? 1 : 0; return; }
    float *w = out3 + (size_t) i * 3;
    ids[i] = found ? (int32_t) h.obj : -1;
    w[0] = found ? h.t : u2f(0x7f800000u); w[1] = found ? h.u : 0.f; w[2] = found ? h.v : 0.f;
}
template <bool ANY, uint32_t FACTS>
__global__ __launch_bounds__(kShadeBlock) void k_flat_query(const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t flat_off, uint32_t flat_objects,
                                                             uint32_t memo_obj, const float *rays, float *out3, int32_t *ids, uint32_t n) {
    flat_query_lane<ANY, FACTS, false>(scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
}
// trace_flat's pair form (dtof_pair_walk.h): n is even and rays 2k and 2k + 1 hold the same o, d and maxt (dtof_flat_query_pairs checks both), so the two lanes of a pair
// are in range together -- a block holds whole pairs -- and the form's premise holds in every wave
template <bool ANY>
__global__ __launch_bounds__(kShadeBlock) void k_flat_query_pairs(const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t flat_off, uint32_t flat_objects,
                                                                   uint32_t memo_obj, const float *rays, float *out3, int32_t *ids, uint32_t n) {
    if constexpr (kFlatQueryPairsBuilt) flat_query_lane<ANY, flat_query_facts(2), true>(scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
}
// trace_flat's ZROW form of the shaped walk (dtof_zrow_mfma.h): the plain rectangles' z rows from six MFMAs issued in front of the query.  An MFMA runs in all 64
// lanes whatever EXEC says, so no lane leaves before them: a lane behind the end of the list takes part with a ray of zeros and its stores are masked -- the partial
// waves are the case of k_shade's lane-divergent call sites.  zrow8 (optional): the eight MFMA values of a ray, origin rows of rectangles 0, 1, 3, 4, then direction rows.
template <bool ANY>
__global__ __launch_bounds__(kShadeBlock) void k_flat_query_zrow(const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t flat_off, uint32_t flat_objects,
                                                                  uint32_t memo_obj, const float *rays, float *out3, int32_t *ids, float *zrow8, uint32_t n) {
    constexpr uint32_t FACTS = flat_query_facts(2);
    if constexpr (kFlatQueryZrowBuilt) {
        extern __shared__ uint4 lds[];
        const uint8_t *base = stage_scene(scene, scene_bytes, lds);
        SceneView sv = make_view(base);
        sv.memo_obj = memo_obj; sv.memo = (float *) (lds + stage_words) + threadIdx.x; sv.memo_m = true;
        const uint32_t i = blockIdx.x * kShadeBlock + threadIdx.x;
        const bool on = i < n;
        float r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = on ? rays[(size_t) i * 8 + k] : 0.f;
        const ZrowOperands m = zrow_operands((const uint4 *) ((const DFlatObject *) (sv.base + flat_off) + flat_shape_count(FACTS)) + 1);
        const ZrowQuad zq = zrow_mfma(m, r[0], r[1], r[2], r[3], r[4], r[5]);
        if (on) {
            if (zrow8) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { zrow8[(size_t) i * 8 + k] = zq.o[k]; zrow8[(size_t) i * 8 + 4 + k] = zq.d[k]; }
            }
            const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
            float memo_m[12], memo_inv[12];
            instance_memo_fill(sv, r[6], memo_m, memo_inv);
            Hit h;
            const bool found = trace_flat<ANY, true, FACTS, false, true, ZrowQuad>(sv, (ConstBytes) scene + flat_off, flat_off, flat_objects, nullptr, o, d, r[6], r[7], h, zq);
            if (ANY) ids[i] = found ? 1 : 0;
            else {
                float *w = out3 + (size_t) i * 3;
                ids[i] = found ? (int32_t) h.obj : -1;
                w[0] = found ? h.t : u2f(0x7f800000u); w[1] = found ? h.u : 0.f; w[2] = found ? h.v : 0.f;
            }
        }
    }
}

template <uint32_t FACTS>
static void launch_form(bool any, uint32_t grid, uint32_t lds, hipStream_t s, const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t flat_off,
                        uint32_t flat_objects, uint32_t memo_obj, const float *rays, float *out3, int32_t *ids, uint32_t n) {
    if (any) hipLaunchKernelGGL((k_flat_query<true, FACTS>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
    else hipLaunchKernelGGL((k_flat_query<false, FACTS>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
}

void launch_flat_query(const uint8_t *scene, uint32_t scene_bytes, uint32_t flat_off, uint32_t flat_objects, uint32_t memo_obj, int form, bool any,
                       const float *rays, float *out3, int32_t *ids, uint32_t n, hipStream_t s, float *zrow8) {
    if (!n) return;
    // the classic fused launch of a flat scene without its stack column (launch_shade, a kernel compiled with kFactFlat): stage + memo columns
    const uint32_t stage_words = (scene_bytes + 15u) / 16u;
    const uint32_t lds = ShadeLds::classic(stage_words, true, memo_obj != 0xffffffffu, 1u).without_stack();
    if (scene_bytes > 16u * 1024u) throw std::runtime_error("dtof_flat_query: the scene does not fit the LDS stage");   // (launch_shade stages up to 16 KiB)
    const uint32_t grid = (n + kShadeBlock - 1u) / kShadeBlock;
    if (form == kFlatQueryPairs) {
        if (any) hipLaunchKernelGGL((k_flat_query_pairs<true>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
        else hipLaunchKernelGGL((k_flat_query_pairs<false>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
    } else if (form == kFlatQueryZrow) {
        if (any) hipLaunchKernelGGL((k_flat_query_zrow<true>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, zrow8, n);
        else hipLaunchKernelGGL((k_flat_query_zrow<false>), dim3(grid), dim3(kShadeBlock), lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, zrow8, n);
    } else if (form == 2) launch_form<flat_query_facts(2)>(any, grid, lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
    else if (form == 1) launch_form<flat_query_facts(1)>(any, grid, lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
    else launch_form<flat_query_facts(0)>(any, grid, lds, s, scene, scene_bytes, stage_words, flat_off, flat_objects, memo_obj, rays, out3, ids, n);
}

}  // namespace dtof
