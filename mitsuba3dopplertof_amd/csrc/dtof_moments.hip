// dtof_moments.hip -- the per-pixel moment film: first and second moments of every sample's XYZ (the AOVs of the reference's `moment` integrator,
// src/integrators/moment.cpp:85-104) and the cross moments Y_j * Y_k between the variants of one traversal, splatted like the image (ImageBlock::put,
// src/render/imageblock.cpp:414-531) into a film of doubles.
//   terms    per lane and variant k, in float32 without contraction: XYZ = srgb_to_xyz(rgb) (include/mitsuba/core/spectrum.h:396-402, the sums left to right like
//            luminance(), dtof_shading.h), the squares X * X, Y * Y, Z * Z (dr::sqr of the AOV) and, per pair j < k, Y_j * Y_k
//   splat    every value through the footprint and float32 weights of k_splat_f64 (dtof_film64.hip): w = wx * wy, the term value * w a float32 product (the box filter
//            adds the value itself and 1.f), converted to double; from there on only double additions.  One weight sum per pixel serves all planes.
//   reduce   runs of lanes that share a footprint anchor are summed in the wave first (dtof_splat_runs.h), so a run issues one atomic per cell and plane
//   develop  every plane but the weight divided by (W == 0 ? 1 : W) in double, into dense planes
// Plane order and device layout: dtof_moments.h.  Compiled with -ffp-contract=off like every kernel here.
#include "dtof_device.h"
#include "dtof_splat_runs.h"
#include "dtof_moments.h"

namespace dtof {

namespace {
constexpr int kMomentsBlock = 256;
constexpr int kPairs = kMaxOffsets * (kMaxOffsets - 1) / 2;
static_assert(kMaxOffsets == 4 && moment_planes(kMaxOffsets) <= kMomentCell, "the pair tables and the cell are laid out for at most four variants");
// k of pair i of (j, k) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3): two bits per entry
DTOF_D int pair_k(int i) { return (0xfb9 >> (2 * i)) & 3; }

// Value j of a few registers for a wave-uniform j.  Scalars, not pick() over arrays: with these many selects the optimiser turned the chains over a private array
// back into an indexed load, and the arrays into LDS and scratch.
DTOF_D float sel(int j, float a0, float a1, float a2, float a3) { float v = a0; v = j == 1 ? a1 : v; v = j == 2 ? a2 : v; return j == 3 ? a3 : v; }
DTOF_D float sel(int j, float a0, float a1, float a2, float a3, float a4) { const float v = sel(j, a0, a1, a2, a3); return j == 4 ? a4 : v; }
DTOF_D float sel(int j, float a0, float a1, float a2, float a3, float a4, float a5) { const float v = sel(j, a0, a1, a2, a3, a4); return j == 5 ? a5 : v; }
#define DTOF_SEL4(a, j) sel(j, a##0, a##1, a##2, a##3)

DTOF_D double term(float v, float w, bool box) { return (double) (box ? v : v * w); }   // the box filter adds the value itself (value * 1.f is the same float)

// q.pos, q.res plane k at k * q.capacity and the pixel from global_lane, as k_splat_f64 reads them.  Every thread of the block stays in the kernel on the run path (the
// shuffles of run_sum are wave-wide); a thread without a lane is a run of its own that adds nothing.
__global__ __launch_bounds__(kMomentsBlock) void k_splat_moments_f64(RenderParams rp, Queues q, double *film) {
    const uint32_t i = blockIdx.x * kMomentsBlock + threadIdx.x;
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
    // the lane's values: XYZ of every variant (0 beyond K and for a thread without a lane) and the products of the pairs
    float vx0, vx1, vx2, vx3, vy0, vy1, vy2, vy3, vz0, vz1, vz2, vz3;
#define DTOF_LOAD_XYZ(k) { \
        const float4 v = valid && k < K ? q.res[(size_t) k * q.capacity + i] : make_float4(0.f, 0.f, 0.f, 0.f); \
        vx##k = (0.412453f * v.x + 0.357580f * v.y) + 0.180423f * v.z; \
        vy##k = (0.212671f * v.x + 0.715160f * v.y) + 0.072169f * v.z; \
        vz##k = (0.019334f * v.x + 0.119193f * v.y) + 0.950227f * v.z; }
    DTOF_LOAD_XYZ(0) DTOF_LOAD_XYZ(1) DTOF_LOAD_XYZ(2) DTOF_LOAD_XYZ(3)
#undef DTOF_LOAD_XYZ
    const float yy0 = vy0 * vy1, yy1 = vy0 * vy2, yy2 = vy0 * vy3, yy3 = vy1 * vy2, yy4 = vy1 * vy3, yy5 = vy2 * vy3;
    if (cnt > kRunCells) {   // wide footprints (the Lanczos filter's 7 x 7): one atomic per lane, cell and plane
        if (!valid) return;
#pragma unroll 1
        for (int ys = 0; ys < cnt; ++ys) {
            const float wy = filter_weight(rp, rely + (float) ys);
#pragma unroll 1
            for (int xs = 0; xs < cnt; ++xs) {
                const float w = filter_weight(rp, relx + (float) xs) * wy;
                const int x = ax + xs, y = ay + ys;
                if ((unsigned) x >= (unsigned) W || (unsigned) y >= (unsigned) H) continue;
                double *c = film + (size_t) kMomentCell * ((size_t) y * W + x);
                add_f64(c, (double) w);
#pragma unroll 1
                for (int k = 0; k < K; ++k) {
                    const float X = DTOF_SEL4(vx, k), Y = DTOF_SEL4(vy, k), Z = DTOF_SEL4(vz, k);
                    double *m = c + 1 + 6 * k;
                    add_f64(m, (double) (X * w)); add_f64(m + 1, (double) (Y * w)); add_f64(m + 2, (double) (Z * w));
                    add_f64(m + 3, (double) ((X * X) * w)); add_f64(m + 4, (double) ((Y * Y) * w)); add_f64(m + 5, (double) ((Z * Z) * w));
                }
                double *m = c + 1 + 6 * K;
#pragma unroll 1
                for (int pr = 0; pr < kPairs; ++pr)
                    if (pair_k(pr) < K) { add_f64(m, (double) (sel(pr, yy0, yy1, yy2, yy3, yy4, yy5) * w)); ++m; }
            }
        }
        return;
    }
    const Runs runs = find_runs(ax, ay, valid);
    const uint32_t dist = runs.dist, steps = runs.steps;
    static_assert(kRunCells == 5, "five column weights are kept in registers");
#define DTOF_WX(a) (a < cnt && !box ? filter_weight(rp, relx + (float) a) : 0.f)
    const float wx0 = DTOF_WX(0), wx1 = DTOF_WX(1), wx2 = DTOF_WX(2), wx3 = DTOF_WX(3), wx4 = DTOF_WX(4);
#undef DTOF_WX
    // The cell, variant and pair loops stay rolled (25 cells x 31 sums unrolled would be far beyond the instruction cache): their counters are scalars, sel() is selects
    // on them.
#pragma unroll 1
    for (int ys = 0; ys < cnt; ++ys) {
        const float wys = box ? 1.f : filter_weight(rp, rely + (float) ys);
#pragma unroll 1
        for (int xs = 0; xs < cnt; ++xs) {
            const int x = ax + xs, y = ay + ys;
            const bool write = valid && runs.last && (unsigned) x < (unsigned) W && (unsigned) y < (unsigned) H;   // the same cell for every lane of the run
            double *cell = film + (size_t) kMomentCell * ((size_t) (write ? y : 0) * W + (write ? x : 0));
            const float w = box ? 1.f : sel(xs, wx0, wx1, wx2, wx3, wx4) * wys;
            const double ws = run_sum(valid ? (double) w : 0.0, dist, steps);
            if (write) add_f64(cell, ws);
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const float X = DTOF_SEL4(vx, k), Y = DTOF_SEL4(vy, k), Z = DTOF_SEL4(vz, k);
                const double s0 = run_sum(term(X, w, box), dist, steps);
                const double s1 = run_sum(term(Y, w, box), dist, steps);
                const double s2 = run_sum(term(Z, w, box), dist, steps);
                const double s3 = run_sum(term(X * X, w, box), dist, steps);
                const double s4 = run_sum(term(Y * Y, w, box), dist, steps);
                const double s5 = run_sum(term(Z * Z, w, box), dist, steps);
                if (write) {
                    double *m = cell + 1 + 6 * k;
                    add_f64(m, s0); add_f64(m + 1, s1); add_f64(m + 2, s2); add_f64(m + 3, s3); add_f64(m + 4, s4); add_f64(m + 5, s5);
                }
            }
            int slot = 1 + 6 * K;
#pragma unroll 1
            for (int pr = 0; pr < kPairs; ++pr) {
                if (pair_k(pr) >= K) continue;   // wave-uniform
                const double sp = run_sum(term(sel(pr, yy0, yy1, yy2, yy3, yy4, yy5), w, box), dist, steps);
                if (write) add_f64(cell + slot, sp);
                ++slot;
            }
        }
    }
}

// blockIdx.y = the plane
__global__ __launch_bounds__(kMomentsBlock) void k_develop_moments(const double *film, double *out, int64_t n, int divide) {
    const int64_t i = (int64_t) blockIdx.x * kMomentsBlock + threadIdx.x;
    if (i >= n) return;
    const double *c = film + (int64_t) kMomentCell * i;
    const uint32_t pl = blockIdx.y;
    const double w = c[0] == 0.0 ? 1.0 : c[0];
    out[(int64_t) pl * n + i] = pl == 0 || !divide ? c[pl] : c[pl] / w;
}
#undef DTOF_SEL4
}  // namespace

void launch_splat_moments(const RenderParams &rp, const Queues &q, double *film, hipStream_t s) {
    if (rp.n_lanes == 0) return;
    hipLaunchKernelGGL(k_splat_moments_f64, dim3((rp.n_lanes + kMomentsBlock - 1) / kMomentsBlock), dim3(kMomentsBlock), 0, s, rp, q, film);
}
void launch_develop_moments(const double *film, int32_t planes, bool divide, double *out, int64_t n_pixels, hipStream_t s) {
    if (n_pixels <= 0 || planes <= 0 || planes > kMomentCell) return;
    hipLaunchKernelGGL(k_develop_moments, dim3((uint32_t) ((n_pixels + kMomentsBlock - 1) / kMomentsBlock), (uint32_t) planes), dim3(kMomentsBlock), 0, s,
                       film, out, n_pixels, divide ? 1 : 0);
}

}  // namespace dtof
