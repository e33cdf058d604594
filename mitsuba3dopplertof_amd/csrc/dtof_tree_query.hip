// dtof_tree_query.hip -- trace_scene / trace_deferred (dtof_traverse.h) over arrays of rays, in the instantiations the ray kernels of a frame carry (ray_shape() and
// launch_rays() of dtof_kernels.hip), each behind what k_trace / k_shadow do around the call -- the lane's stack column, the overflow array, the TLAS copy -- and nothing
// else.  A translation unit of its own: the render kernels' units do not see it, their code objects stay what they were.
#include "dtof_device.h"
#include "dtof_tree_query.h"

namespace dtof {

constexpr bool tree_form_w8(int form) { return form >= 1 && form <= 3; }

template <int FORM, bool ANY>
__global__ __launch_bounds__(64, tree_form_w8(FORM) ? 8 : 6) void k_tree_query(const uint8_t *scene, const float *rays, float *out3, int32_t *ids, uint32_t n, uint32_t n_tlas) {
    constexpr bool W8 = tree_form_w8(FORM);
    extern __shared__ uint4 lds[];
    uint32_t *stack = (uint32_t *) lds + threadIdx.x;
    const SceneView sv = make_view(scene);
    const BvhNode *tlas = nullptr;
    if (FORM == 2) {   // k_trace<..., TL>: the block's own copy of the TLAS nodes, behind its stack column
        uint4 *const t = lds + kLdsStack8 * 64u / 4u;
        for (uint32_t i = threadIdx.x; i < n_tlas * 4u; i += 64u) t[i] = ((const uint4 *) sv.nodes)[i];
        __syncthreads();
        tlas = (const BvhNode *) t;
    }
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool active = i < n;
    float r[8] = { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f };
    if (active) for (int k = 0; k < 8; ++k) r[k] = rays[(size_t) i * 8 + k];
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    const float time = r[6], maxt = r[7];
    Hit h;
    uint32_t ovf[W8 ? kOvfStack8 : 1];
    bool found;
    if (FORM == 0) found = trace_rays<ANY, 1>(sv, stack, active, o, d, time, maxt, h);
    else if (FORM == 1) found = trace_rays<ANY, 2, false, false, 64, kLdsStack8, false, true>(sv, stack, active, o, d, time, maxt, h, ovf);
    else if (FORM == 2) found = trace_rays<ANY, 2, false, false, 64, kLdsStack8, true, true>(sv, stack, active, o, d, time, maxt, h, ovf, tlas);
    else if (FORM == 3) {
        uint4 cand = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
        found = trace_rays<ANY, 2, false, false, 64, kLdsStack8, false, true, true>(sv, stack, active, o, d, time, maxt, h, ovf, nullptr, &cand);
        // k_trace_deferred goes on from the hit the first launch stored; k_shadow_deferred runs for the rays nothing else occludes
        if (active && cand.x != 0xffffffffu && !(ANY && found)) found = trace_deferred<ANY, 2, 64, kLdsStack8, true>(sv, stack, cand, o, d, time, maxt, h, ovf);
    }
    else found = trace_rays<ANY, 1, false, false, 64, 0u, false, true>(sv, stack, active, o, d, time, maxt, h);
    if (!active) return;
    if (ANY) { ids[i] = found ? 1 : 0; return; }
    float *w = out3 + (size_t) i * 3;
    int32_t *q = ids + (size_t) i * 3;
    q[0] = found ? (int32_t) h.obj : -1; q[1] = found ? (int32_t) h.shape : -1; q[2] = found ? (int32_t) hit_prim_index(sv, h) : -1;
    w[0] = found ? h.t : u2f(0x7f800000u); w[1] = found ? h.u : 0.f; w[2] = found ? h.v : 0.f;
}

const char *tree_query_refusal(int form, const TreeQueryScene &t) {
    if (form < 0 || form >= kTreeQueryForms) return "form must be 0 (float nodes), 1 (half-float nodes, overflow stack), 2 (form 1 with the TLAS in LDS), 3 (the DEFER pair) or 4 (half-float nodes, every shape)";
    if (form == 0) return nullptr;
    if (!t.has_nodes16) return "the scene has no half-float nodes (no mesh behind a BLAS)";
    if (form == 4) return nullptr;
    if (t.has_analytic) return "the scene has an analytic shape (sphere, disk, cylinder) and the eight-wave kernels carry triangle and rectangle code only";
    if (t.stack_depth > kLdsStack8 + kOvfStack8) return "the scene's traversal stack is deeper than the eight-wave kernels' LDS column and overflow array";
    if (form == 2 && (t.n_tlas_nodes == 0 || t.n_tlas_nodes > kTlasLds8)) return "the TLAS does not fit the eight-wave kernels' LDS copy";
    return nullptr;
}

template <int FORM>
static void launch_form(bool any, uint32_t lds, hipStream_t s, const uint8_t *scene, const float *rays, float *out3, int32_t *ids, uint32_t n, uint32_t n_tlas) {
    const dim3 grid((n + 63u) / 64u);
    if (any) hipLaunchKernelGGL((k_tree_query<FORM, true>), grid, dim3(64), lds, s, scene, rays, out3, ids, n, n_tlas);
    else hipLaunchKernelGGL((k_tree_query<FORM, false>), grid, dim3(64), lds, s, scene, rays, out3, ids, n, n_tlas);
}

void launch_tree_query(const uint8_t *scene, const TreeQueryScene &t, int form, bool any, const float *rays, float *out3, int32_t *ids, uint32_t n, hipStream_t s) {
    if (const char *why = tree_query_refusal(form, t)) throw std::runtime_error(std::string("dtof_tree_query: ") + why);
    if (!n) return;
    // ray_shape(): the stack column (the eight-wave kernels: its first kLdsStack8 entries) and, behind it, the TLAS copy
    const uint32_t lds = stack_bytes(tree_form_w8(form) ? kLdsStack8 : t.stack_depth, 64) + (form == 2 ? kTlasLds8 * 64u : 0u);
    if (lds + 64u > 64u * 1024u) throw std::runtime_error("dtof_tree_query: the BVH of this scene is too deep for the LDS traversal stack");
    switch (form) {
        case 0: launch_form<0>(any, lds, s, scene, rays, out3, ids, n, 0u); break;
        case 1: launch_form<1>(any, lds, s, scene, rays, out3, ids, n, 0u); break;
        case 2: launch_form<2>(any, lds, s, scene, rays, out3, ids, n, t.n_tlas_nodes); break;
        case 3: launch_form<3>(any, lds, s, scene, rays, out3, ids, n, 0u); break;
        default: launch_form<4>(any, lds, s, scene, rays, out3, ids, n, 0u); break;
    }
}

}  // namespace dtof
