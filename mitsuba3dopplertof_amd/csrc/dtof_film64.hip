// dtof_film64.hip -- the float64 film: the splat of ImageBlock::put (src/render/imageblock.cpp:414-531) with a double accumulator.  (Its develop, taken in double,
// is the double instantiation of dtof_develop.hip.)
//   splat_f64 : every term is the float32 product the float32 film adds (w = wx * wy, value * w, w for the weight channel; the box filter adds the value itself and
//               1.f -- splat_lane, dtof_device.h); the term is converted to double and from there on only double additions happen.  A double sum of a few thousand
//               float32 terms carries ~29 spare bits, so the order of the additions no longer reaches the developed float.
// The footprint, the walk over its cells (per lane for wide footprints, per run of lanes otherwise) and the run reduction are dtof_splat64.h's, shared with the moment
// film and the aov film; this file keeps what a cell receives: K films of RGBW, film_stride apart.  Compiled with -ffp-contract=off like every kernel here.
#include "dtof_splat64.h"
#include "dtof_film64.h"

namespace dtof {

namespace {
constexpr int kFilm64Block = 256;
static_assert(kMaxOffsets == 4, "sel() picks a film's value out of four registers");

// q.pos, q.res plane k at k * q.capacity and the pixel from global_lane, as k_splat_generic reads them.  Every thread of the block stays in the kernel on the run path
// (the shuffles of run_sum are wave-wide); a thread without a lane is a run of its own that adds nothing.
__global__ __launch_bounds__(kFilm64Block) void k_splat_f64(RenderParams rp, Queues q, double *film, size_t film_stride) {
    const uint32_t i = blockIdx.x * kFilm64Block + threadIdx.x;
    const bool valid = i < rp.n_lanes;
    const int K = rp.n_offsets;
    const Footprint f = footprint_of(rp, i, valid, q.pos);
    if (f.cnt > kRunCells) {
        if (valid) walk_wide(rp, f, [&](size_t pixel, float w) {
            for (int k = 0; k < K; ++k) {
                const float4 r = q.res[(size_t) k * q.capacity + i];
                double *c = film + (size_t) k * film_stride + 4 * pixel;
                add_f64(c, (double) (r.x * w)); add_f64(c + 1, (double) (r.y * w)); add_f64(c + 2, (double) (r.z * w)); add_f64(c + 3, (double) w);
            }
        });
        return;
    }
    const RunCells rc = run_cells_of(rp, f, valid);
    float rr[kMaxOffsets], rg[kMaxOffsets], rb[kMaxOffsets];   // (only ever indexed by constants)
#pragma unroll
    for (int k = 0; k < kMaxOffsets; ++k) {
        const float4 v = valid && k < K ? q.res[(size_t) k * q.capacity + i] : make_float4(0.f, 0.f, 0.f, 0.f);
        rr[k] = v.x; rg[k] = v.y; rb[k] = v.z;
    }
    walk_runs(rp, f, rc, [&](float w, bool write, size_t pixel) {
        const double ws = run_sum(valid ? term(1.f, w, f.box) : 0.0, rc.dist, rc.steps);   // the weight channel's value is 1 (1.f * w is w)
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const double sr = run_sum(term(sel(k, rr[0], rr[1], rr[2], rr[3]), w, f.box), rc.dist, rc.steps);
            const double sg = run_sum(term(sel(k, rg[0], rg[1], rg[2], rg[3]), w, f.box), rc.dist, rc.steps);
            const double sb = run_sum(term(sel(k, rb[0], rb[1], rb[2], rb[3]), w, f.box), rc.dist, rc.steps);
            if (write) {
                double *c = film + (size_t) k * film_stride + 4 * pixel;
                add_f64(c, sr); add_f64(c + 1, sg); add_f64(c + 2, sb); add_f64(c + 3, ws);
            }
        }
    });
}
}  // namespace

void launch_splat_f64(const RenderParams &rp, const Queues &q, double *film64, uint64_t plane_stride_doubles, hipStream_t s) {
    if (rp.n_lanes == 0) return;
    hipLaunchKernelGGL(k_splat_f64, dim3((rp.n_lanes + kFilm64Block - 1) / kFilm64Block), dim3(kFilm64Block), 0, s, rp, q, film64, (size_t) plane_stride_doubles);
}

}  // namespace dtof
