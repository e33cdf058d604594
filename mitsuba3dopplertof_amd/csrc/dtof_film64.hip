// dtof_film64.hip -- the float64 film: the splat of ImageBlock::put (src/render/imageblock.cpp:414-531) with a double accumulator.  (Its develop, taken in double,
// is the double instantiation of dtof_develop.hip.)
//   splat_f64 : every term is the float32 product the float32 film adds (w = wx * wy, value * w, w for the weight channel; the box filter adds the value itself and
//               1.f -- splat_lane, dtof_device.h); the term is converted to double and from there on only double additions happen.  A double sum of a few thousand
//               float32 terms carries ~29 spare bits, so the order of the additions no longer reaches the developed float.
// Compiled with -ffp-contract=off like every kernel here.
#include "dtof_device.h"
#include "dtof_splat_runs.h"
#include "dtof_film64.h"

namespace dtof {

namespace {
constexpr int kFilm64Block = 256;
// run_sum, pick, add_f64, find_runs and kRunCells: dtof_splat_runs.h (shared with the moment film, dtof_moments.hip)

// q.pos, q.res plane k at k * q.capacity and the pixel from global_lane, as k_splat_generic reads them.  Every thread of the block stays in the kernel (the shuffles
// of run_sum are wave-wide); a thread without a lane is a run of its own that adds nothing.
__global__ __launch_bounds__(kFilm64Block) void k_splat_f64(RenderParams rp, Queues q, double *film, size_t film_stride) {
    const uint32_t i = blockIdx.x * kFilm64Block + threadIdx.x;
    const bool valid = i < rp.n_lanes;
    const int W = rp.crop_w, H = rp.crop_h, K = rp.n_offsets;
    const bool box = rp.filter == FILTER_BOX;
    const int n = box ? 0 : (int) ceilf(rp.filter_radius - .5f), cnt = 2 * n + 1;
    const float2 p = valid ? q.pos[i] : make_float2(0.f, 0.f);
    // the footprint's anchor in film coordinates (splat_lane): the box filter splats at the lane's own pixel, every other at floor(position) - n
    int ax, ay; float relx = 0.f, rely = 0.f;
    if (box) {
        const uint32_t pix = fdiv(global_lane(rp, rp.lane_base + (valid ? i : 0u)), rp.d_spp);
        ay = (int) fdiv(pix, rp.d_w); ax = (int) (pix - (uint32_t) W * (uint32_t) ay);
    } else {
        const int pix = (int) floorf(p.x) - n, piy = (int) floorf(p.y) - n;
        relx = (float) pix + .5f - p.x; rely = (float) piy + .5f - p.y;
        ax = pix - rp.crop_x; ay = piy - rp.crop_y;
    }
    if (cnt > kRunCells) {   // wide footprints (the Lanczos filter's 7 x 7): one atomic per lane, cell and channel
        if (!valid) return;
        for (int ys = 0; ys < cnt; ++ys) {
            const float wy = filter_weight(rp, rely + (float) ys);
            for (int xs = 0; xs < cnt; ++xs) {
                const float w = filter_weight(rp, relx + (float) xs) * wy;
                const int x = ax + xs, y = ay + ys;
                if ((unsigned) x >= (unsigned) W || (unsigned) y >= (unsigned) H) continue;
                for (int k = 0; k < K; ++k) {
                    const float4 r = q.res[(size_t) k * q.capacity + i];
                    double *c = film + (size_t) k * film_stride + 4 * ((size_t) y * W + x);
                    add_f64(c, (double) (r.x * w)); add_f64(c + 1, (double) (r.y * w)); add_f64(c + 2, (double) (r.z * w)); add_f64(c + 3, (double) w);
                }
            }
        }
        return;
    }
    const Runs runs = find_runs(ax, ay, valid);
    const uint32_t dist = runs.dist, steps = runs.steps;
    const bool last = runs.last;
    float wx[kRunCells];
#pragma unroll
    for (int a = 0; a < kRunCells; ++a) wx[a] = a < cnt && !box ? filter_weight(rp, relx + (float) a) : 0.f;
    float rr[kMaxOffsets], rg[kMaxOffsets], rb[kMaxOffsets];
#pragma unroll
    for (int k = 0; k < kMaxOffsets; ++k) {
        const float4 v = valid && k < K ? q.res[(size_t) k * q.capacity + i] : make_float4(0.f, 0.f, 0.f, 0.f);
        rr[k] = v.x; rg[k] = v.y; rb[k] = v.z;
    }
    // The cell and film loops stay rolled (25 cells x 13 sums unrolled would be ~60 KiB of code): their counters are scalars, pick() turns into selects on them.
#pragma unroll 1
    for (int ys = 0; ys < cnt; ++ys) {
        const float wys = box ? 1.f : filter_weight(rp, rely + (float) ys);
#pragma unroll 1
        for (int xs = 0; xs < cnt; ++xs) {
            const int x = ax + xs, y = ay + ys;
            const bool write = valid && last && (unsigned) x < (unsigned) W && (unsigned) y < (unsigned) H;   // the same cell for every lane of the run
            double *cell = film + 4 * ((size_t) (write ? y : 0) * W + (write ? x : 0));
            const float w = box ? 1.f : pick(wx, xs) * wys;
            const double ws = run_sum(valid ? (double) w : 0.0, dist, steps);
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const float vr = pick(rr, k), vg = pick(rg, k), vb = pick(rb, k);
                // the box filter adds the value itself (value * 1.f is the same float)
                const double sr = run_sum((double) (box ? vr : vr * w), dist, steps);
                const double sg = run_sum((double) (box ? vg : vg * w), dist, steps);
                const double sb = run_sum((double) (box ? vb : vb * w), dist, steps);
                if (write) {
                    double *c = cell + (size_t) k * film_stride;
                    add_f64(c, sr); add_f64(c + 1, sg); add_f64(c + 2, sb); add_f64(c + 3, ws);
                }
            }
        }
    }
}
}  // namespace

void launch_splat_f64(const RenderParams &rp, const Queues &q, double *film64, uint64_t plane_stride_doubles, hipStream_t s) {
    if (rp.n_lanes == 0) return;
    hipLaunchKernelGGL(k_splat_f64, dim3((rp.n_lanes + kFilm64Block - 1) / kFilm64Block), dim3(kFilm64Block), 0, s, rp, q, film64, (size_t) plane_stride_doubles);
}

}  // namespace dtof
