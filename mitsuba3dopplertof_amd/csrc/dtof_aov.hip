// dtof_aov.hip -- the geometry channels of the reference's `aov` integrator (src/integrators/aov.cpp:196-330), from the camera ray to the film in one kernel:
//   query    the lane's camera ray as k_generate left it (origin, direction, time, maxt), one closest hit at the ray's OWN time (Scene::ray_intersect with
//            RayFlags::All, aov.cpp:206-207) through trace_rays, the scene staged as k_velocity stages it
//   surface  compute_surface with the frames on: dp_du / dp_dv come through instances (dtof_shading.h); every value is +0 on a miss (aov.cpp:208)
//   select   the lane's 20 values stay in registers; channel c is value slot[c], picked by selects on a wave-uniform counter (dtof_aov.h: the slots)
//   splat    the footprint, the float32 weights, the cell walks and the run reduction of dtof_splat64.h, shared with the float64 film and the moment film: the term
//            value * (wx * wy) is a float32 product (the box filter adds the value itself and 1.f), converted to double; runs of lanes with one footprint anchor are
//            summed in the wave and the run's last lane issues one atomic per cell and channel; footprints wider than 5 x 5 take one atomic per lane, cell and
//            channel.  This file keeps its order: the plane loop outside, the walk inside
// With AovArgs::values the lane's channels are written out instead of the splat (dtof_sample_aov_lanes): the same code up to the selection.
// k_aov<LDS, FLOW = true> is the flow film (dtof_render_flow, dtof_sample_flow_lanes): two more values per lane, the screen-space motion of the hit over the shutter
// interval (flow_of below), through the same selection and the same splat; the FLOW = false instantiations hold none of it (profiles/flow_resource_usage.txt).
// Compiled with -ffp-contract=off like every kernel here.
#include "dtof_splat64.h"
#include "dtof_aov.h"

namespace dtof {

namespace {
static_assert(kAovMaxChannels <= 3 * (int) kAovSlotsPerWord && kAovSlots <= 32 && kAovFlowSlots <= 32, "the channel table is three words of twelve 5-bit slots");

// Value j of the lane's 20 for a wave-uniform j.  Twenty scalars and a chain of selects, like sel() of dtof_splat64.h: an array or a struct that is indexed goes to scratch.
#define DTOF_AOV_LIST(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19)
#define DTOF_AOV_PICK(k) v = j == k ? v##k : v;
// (the two flow values only in the FLOW instantiations: the others keep their twenty selects)
#define DTOF_AOV_SEL(j_) ([&] { const uint32_t j = (j_); float v = 0.f; DTOF_AOV_LIST(DTOF_AOV_PICK) if constexpr (FLOW) { DTOF_AOV_PICK(20) DTOF_AOV_PICK(21) } return v; }())
// c is wave-uniform: scalar shifts of three argument words (an indexed table in the argument block would be copied to scratch)
DTOF_D uint32_t slot_of(const AovArgs &a, uint32_t c) {
    const uint64_t w = c < kAovSlotsPerWord ? a.slots[0] : c < 2 * kAovSlotsPerWord ? a.slots[1] : a.slots[2];
    const uint32_t k = c < kAovSlotsPerWord ? c : c < 2 * kAovSlotsPerWord ? c - kAovSlotsPerWord : c - 2 * kAovSlotsPerWord;
    return (uint32_t) (w >> (5u * k)) & 31u;
}

// The motion vector of a hit on an animated object (include/dtof.h: the flow film): the hit point is taken into the object's own frame with the inverse of the
// keyframes' interpolant at the ray's time, placed with each keyframe, and both positions are projected with S.  All in double, formed from the float32 hit and
// keyframes; every operation is the one tests/flow_ref.py names, in its order: the cofactors of affine_inverse (dtof_math.h) with a * b - c * d for each
// fmaf(a, b, -(c * d)) and (a x + b y) + c z for each three-term chain, a point through a matrix row as ((m0 x + m1 y) + m2 z) + m3.
DTOF_D double row_point(const double *m, double x, double y, double z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }
DTOF_D double row_point(const float *m, double x, double y, double z) { return (((double) m[0] * x + (double) m[1] * y) + (double) m[2] * z) + (double) m[3]; }
DTOF_D void flow_of(const DObject &ob, V3 p, float time, const double *S, float &fx, float &fy) {
    const double x = ((double) time - (double) ob.t0) / ((double) ob.t1 - (double) ob.t0);
    double u = x > 0.0 ? x : 0.0; u = u < 1.0 ? u : 1.0;
    const double omu = 1.0 - u;
    double m[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m[i] = (double) ob.key0[i] * omu + (double) ob.key1[i] * u;
    const double a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[4], a11 = m[5], a12 = m[6], a20 = m[8], a21 = m[9], a22 = m[10];
    const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double id = 1.0 / det;
    double inv[12];
    inv[0] = c00 * id; inv[1] = (a02 * a21 - a01 * a22) * id; inv[2] = (a01 * a12 - a02 * a11) * id;
    inv[4] = c01 * id; inv[5] = (a00 * a22 - a02 * a20) * id; inv[6] = (a02 * a10 - a00 * a12) * id;
    inv[8] = c02 * id; inv[9] = (a01 * a20 - a00 * a21) * id; inv[10] = (a00 * a11 - a01 * a10) * id;
    const double tx = m[3], ty = m[7], tz = m[11];
    inv[3] = -((inv[0] * tx + inv[1] * ty) + inv[2] * tz);
    inv[7] = -((inv[4] * tx + inv[5] * ty) + inv[6] * tz);
    inv[11] = -((inv[8] * tx + inv[9] * ty) + inv[10] * tz);
    const double px = (double) p.x, py = (double) p.y, pz = (double) p.z;
    const double qx = row_point(inv, px, py, pz), qy = row_point(inv + 4, px, py, pz), qz = row_point(inv + 8, px, py, pz);
    const double x0 = row_point(ob.key0, qx, qy, qz), y0 = row_point(ob.key0 + 4, qx, qy, qz), z0 = row_point(ob.key0 + 8, qx, qy, qz);   // at shutter open
    const double x1 = row_point(ob.key1, qx, qy, qz), y1 = row_point(ob.key1 + 4, qx, qy, qz), z1 = row_point(ob.key1 + 8, qx, qy, qz);   // at shutter close
    const double w0 = row_point(S + 8, x0, y0, z0), w1 = row_point(S + 8, x1, y1, z1);
    if (!(w0 > 0.0) || !(w1 > 0.0)) { fx = fy = __int_as_float(0x7fc00000); return; }   // not in front of the camera at both ends: "no history"
    fx = (float) (row_point(S, x1, y1, z1) / w1 - row_point(S, x0, y0, z0) / w0);
    fy = (float) (row_point(S + 4, x1, y1, z1) / w1 - row_point(S + 4, x0, y0, z0) / w0);
}

// Every thread of the block stays in the kernel up to the splat (the staging barrier, and the shuffles of run_sum are wave-wide); a thread without a lane has no ray,
// is a run of its own and adds nothing.  FLOW: the lane has the two flow values beside its twenty (the flow film's instantiations).
template <bool LDS, bool FLOW>
__global__ __launch_bounds__(kBlock) void k_aov(const uint8_t *scene, uint32_t scene_bytes, uint32_t stage_words, RenderParams rp, Queues q, AovArgs a) {
    extern __shared__ uint4 lds[];
    const uint8_t *base = LDS ? stage_scene(scene, scene_bytes, lds) : scene;
    uint32_t *stack = (uint32_t *) (lds + stage_words) + threadIdx.x;
    const SceneView sv = make_view(base);
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i < rp.n_lanes;
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = make_float4(0.f, 0.f, 1.f, 0.f);
    if (valid) { ra = q.ray_a[i]; rb = q.ray_b[i]; }
    const V3 o = mk(ra.x, ra.y, ra.z), d = mk(rb.x, rb.y, rb.z);
    Hit h;
    const bool found = trace_rays<false, true>(sv, stack, valid, o, d, ra.w, rb.w, h);
#define DTOF_AOV_DECL(k) float v##k = 0.f;
    DTOF_AOV_LIST(DTOF_AOV_DECL)
    [[maybe_unused]] DTOF_AOV_DECL(20) [[maybe_unused]] DTOF_AOV_DECL(21)
#undef DTOF_AOV_DECL
    if (found) {
        Surface si;
        compute_surface<true>(sv, h.obj, h.shape, h.prim, h.t, h.u, h.v, o, d, ra.w, si);
        v0 = h.t;
        v1 = si.p.x; v2 = si.p.y; v3 = si.p.z;
        v4 = si.u; v5 = si.v;
        v6 = si.n.x; v7 = si.n.y; v8 = si.n.z;
        v9 = si.sh_n.x; v10 = si.sh_n.y; v11 = si.sh_n.z;
        v12 = si.dp_du.x; v13 = si.dp_du.y; v14 = si.dp_du.z;
        v15 = si.dp_dv.x; v16 = si.dp_dv.y; v17 = si.dp_dv.z;
        v18 = (float) hit_prim_index(sv, h);
        v19 = (float) (1u + (uint32_t) (si.shape - sv.shapes));
        if constexpr (FLOW) {   // a miss, and a hit on an object without a second keyframe, keep (+0, +0)
            const DObject &ob = sv.objects[h.obj];
            if (ob.n_keys > 1) flow_of(ob, si.p, ra.w, a.S, v20, v21);
        }
    }
    const uint32_t C = a.n_channels;
    if (a.values) {   // the per-lane entry: the channels of the lane, no splat
        if (!valid) return;
        float *out = a.values + (size_t) i * C;
#pragma unroll 1
        for (uint32_t c = 0; c < C; ++c) out[c] = DTOF_AOV_SEL(slot_of(a, c));
        return;
    }
    double *const film = a.film;
    const Footprint f = footprint_of(rp, i, valid, q.pos);
    if (f.cnt > kRunCells) {
        if (valid) walk_wide(rp, f, [&](size_t pixel, float w) {
            double *cell = film + (size_t) kMomentCell * pixel;
            add_f64(cell, (double) w);
#pragma unroll 1
            for (uint32_t c = 0; c < C; ++c) add_f64(cell + 1 + c, (double) (DTOF_AOV_SEL(slot_of(a, c)) * w));
        });
        return;
    }
    const RunCells rc = run_cells_of(rp, f, valid);
    // The PLANE loop is the outer one (plane 0: the weight, the value 1; plane 1 + c: channel c), so a channel's value is selected once and not once per cell; the
    // walk inside it redoes a cell's address and weight per plane, a handful of instructions against the twenty selects (the runs and the ten weights are rc's,
    // computed once).  The plane loop stays rolled like the walk's: its counter is a scalar.  1.f * w is w, so the weight takes the channels' code.
#pragma unroll 1
    for (uint32_t pl = 0; pl <= C; ++pl) {
        const float v = pl == 0 ? (valid ? 1.f : 0.f) : DTOF_AOV_SEL(slot_of(a, pl - 1u));
        walk_runs(rp, f, rc, [&](float w, bool write, size_t pixel) {
            const double sum = run_sum(term(v, w, f.box), rc.dist, rc.steps);
            if (write) add_f64(film + (size_t) kMomentCell * pixel + pl, sum);
        });
    }
}
#undef DTOF_AOV_SEL
#undef DTOF_AOV_PICK
#undef DTOF_AOV_LIST

// launch_velocity's staging rule (dtof_kernels.hip): the blob goes to LDS while it is small and leaves room for the stack columns within the 64 KiB a block may ask for
constexpr uint32_t kAovSceneLimit = 16 * 1024, kAovBlockLimit = 64 * 1024;
}  // namespace

void launch_aov(const uint8_t *scene, uint32_t scene_bytes, const RenderParams &rp, const Queues &q, const AovArgs &a, uint32_t stack_depth, const LaunchSwitches &ls,
                hipStream_t s) {
    if (rp.n_lanes == 0) return;
    if (a.n_channels < 1 || a.n_channels > (uint32_t) kAovMaxChannels || (!a.film && !a.values)) throw std::runtime_error("internal error: launch_aov without channels or without a destination");
    for (uint32_t c = 0; c < a.n_channels; ++c)
        if (((a.slots[c / kAovSlotsPerWord] >> (5u * (c % kAovSlotsPerWord))) & 31u) >= (uint64_t) (a.flow ? kAovFlowSlots : kAovSlots)) throw std::runtime_error("internal error: launch_aov with a channel table beyond the lane's values");
    const uint32_t stack = stack_bytes(stack_depth), words = (scene_bytes + 15) / 16;
    const uint32_t sw = ls.stage && scene_bytes <= kAovSceneLimit && words * 16 + stack + 64 <= kAovBlockLimit ? words : 0;
    const uint32_t lds = sw * 16 + stack;
    if (lds + 64 > kAovBlockLimit) throw std::runtime_error("the BVH of this scene is too deep for the LDS traversal stack");
    const dim3 grid(nblk(rp.n_lanes)), block(kBlock);
    if (a.flow) {
        if (sw) hipLaunchKernelGGL((k_aov<true, true>), grid, block, lds, s, scene, scene_bytes, sw, rp, q, a);
        else hipLaunchKernelGGL((k_aov<false, true>), grid, block, lds, s, scene, scene_bytes, sw, rp, q, a);
    } else if (sw) hipLaunchKernelGGL((k_aov<true, false>), grid, block, lds, s, scene, scene_bytes, sw, rp, q, a);
    else hipLaunchKernelGGL((k_aov<false, false>), grid, block, lds, s, scene, scene_bytes, sw, rp, q, a);
}

}  // namespace dtof
