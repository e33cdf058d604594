// dtof_surface_query.hip -- compute_surface and offset_p (dtof_shading.h) over arrays of hits: the instantiations and argument patterns the kernels of a frame run,
// each behind what k_shade does around the call -- the blob staged in LDS, the lane's instance-memo columns in the layout of ShadeLds, the memo filled at the lane's
// ray time, the wall's frames -- and nothing else.  A hit is given, not traced: t, b1, b2 and the ids may be what no traversal reports.
// A translation unit of its own: the render kernels' units do not see it.
#include "dtof_device.h"
#include "dtof_surface_query.h"

namespace dtof {

template <int FORM>
__global__ __launch_bounds__(kShadeBlock) void k_surface_query(const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, uint32_t flat_off, uint32_t flat_objects,
                                                                uint32_t memo_obj, uint32_t want_frame_u, const float *in10, const int32_t *ids3, float *out32, uint32_t n) {
    extern __shared__ uint4 lds[];
    constexpr bool MESH = FORM == 0 || FORM == 5, STAGED = !MESH, MEMO = FORM >= 2, MEMO_M = FORM == 3 || FORM == 4;
    const uint8_t *base = STAGED ? stage_scene(scene, scene_bytes, lds) : scene;
    SceneView sv = make_view(base);
    // k_shade, fused: the memo column behind the stage, word k of this thread at memo[k * kMemoStride]; the flat scenes' kernels keep the matrix in a second column
    if (MEMO) { sv.memo_obj = memo_obj; sv.memo = (float *) (lds + (STAGED ? stage_words : 0u)) + threadIdx.x; sv.memo_m = MEMO_M; }
    const bool want_frame = want_frame_u != 0u;
    const uint32_t i = blockIdx.x * kShadeBlock + threadIdx.x;
    if (i >= n) return;   // (behind the stage's barrier)
    const float *r = in10 + (size_t) i * kSurfaceIn;
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const float time = r[6], t = r[7], b1 = r[8], b2 = r[9];
    const uint32_t oi = (uint32_t) ids3[(size_t) i * 3], shape_k = (uint32_t) ids3[(size_t) i * 3 + 1], prim = (uint32_t) ids3[(size_t) i * 3 + 2];
    Surface si;
    if constexpr (FORM == 0) {
        if (want_frame) compute_surface<true>(sv, oi, shape_k, prim, t, b1, b2, o, d, time, si);
        else { const float none[12] = { 0 }; compute_surface<true>(sv, oi, shape_k, prim, t, b1, b2, o, d, time, si, false, none, none, false); }
    } else if constexpr (FORM == 1) {
        const float none[12] = { 0 };
        compute_surface<false>(sv, oi, shape_k, prim, t, b1, b2, o, d, time, si, false, none, none, want_frame);
    } else {
        float memo_m[12], memo_inv[12];
        instance_memo_fill(sv, time, memo_m, memo_inv);
        if constexpr (FORM == 2) { instance_matrix(sv.objects[sv.memo_obj], time, memo_m); instance_memo_load(sv, memo_inv); }   // k_shade's later inline iterations: the inverse from the column
        if constexpr (FORM == 4) {
            WallFrames wf;
            wall_frames_init(wf, sv, flat_off, flat_objects);
            wall_frames_fill(wf, sv, memo_m, memo_inv);
            compute_surface<false, kFactOneWall>(sv, oi, shape_k, prim, t, b1, b2, o, d, time, si, true, memo_m, memo_inv, want_frame, &wf);
        } else compute_surface<MESH>(sv, oi, shape_k, prim, t, b1, b2, o, d, time, si, true, memo_m, memo_inv, want_frame);
    }
    const V3 up = offset_p(si, d), down = offset_p(si, -d);
    const V3 f[6] = { si.p, si.n, si.sh_n, si.sh_s, si.sh_t, si.wi }, g[4] = { si.dp_du, si.dp_dv, up, down };
    float *w = out32 + (size_t) i * kSurfaceOut;
    for (int k = 0; k < 6; ++k) { w[3 * k] = f[k].x; w[3 * k + 1] = f[k].y; w[3 * k + 2] = f[k].z; }
    w[18] = si.u; w[19] = si.v;
    for (int k = 0; k < 4; ++k) { w[20 + 3 * k] = g[k].x; w[21 + 3 * k] = g[k].y; w[22 + 3 * k] = g[k].z; }
}

template <int FORM>
static void launch_form(uint32_t lds, hipStream_t s, const uint8_t *scene, const SurfaceQueryScene &q, uint32_t stage_words, bool want_frame,
                        const float *in10, const int32_t *ids3, float *out32, uint32_t n) {
    hipLaunchKernelGGL((k_surface_query<FORM>), dim3((n + kShadeBlock - 1u) / kShadeBlock), dim3(kShadeBlock), lds, s, scene, q.scene_bytes, stage_words, q.flat_off, q.flat_objects,
                       q.memo_obj, want_frame ? 1u : 0u, in10, ids3, out32, n);
}

void launch_surface_query(const uint8_t *scene, const SurfaceQueryScene &q, int form, bool want_frame, const float *in10, const int32_t *ids3, float *out32, uint32_t n, hipStream_t s) {
    if (!n) return;
    const bool staged = form >= 1 && form <= 4;
    if (staged && q.scene_bytes > 16u * 1024u) throw std::logic_error("launch_surface_query: the caller checks that the blob fits the LDS stage");   // (dtof_surface_eval refuses it before any device work)
    const uint32_t stage_words = staged ? (q.scene_bytes + 15u) / 16u : 0u;
    // the classic fused launch without its stack column: the stage and one memo column, two where the matrix is kept as well (forms 3 and 4)
    const uint32_t lds = ShadeLds::classic(stage_words, true, form == 3 || form == 4, 1u).without_stack();
    switch (form) {
        case 0: launch_form<0>(lds, s, scene, q, stage_words, want_frame, in10, ids3, out32, n); break;
        case 1: launch_form<1>(lds, s, scene, q, stage_words, want_frame, in10, ids3, out32, n); break;
        case 2: launch_form<2>(lds, s, scene, q, stage_words, want_frame, in10, ids3, out32, n); break;
        case 3: launch_form<3>(lds, s, scene, q, stage_words, want_frame, in10, ids3, out32, n); break;
        case 4: launch_form<4>(lds, s, scene, q, stage_words, want_frame, in10, ids3, out32, n); break;
        default: launch_form<5>(lds, s, scene, q, stage_words, want_frame, in10, ids3, out32, n); break;
    }
}

}  // namespace dtof
