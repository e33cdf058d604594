// dtof_moments.hip -- the per-pixel moment film: first and second moments of every sample's XYZ (the AOVs of the reference's `moment` integrator,
// src/integrators/moment.cpp:85-104) and the cross moments Y_j * Y_k between the variants of one traversal, splatted like the image (ImageBlock::put,
// src/render/imageblock.cpp:414-531) into a film of doubles.
//   terms    per lane and variant k, in float32 without contraction: XYZ = srgb_to_xyz(rgb) (include/mitsuba/core/spectrum.h:396-402, the sums left to right like
//            luminance(), dtof_shading.h), the squares X * X, Y * Y, Z * Z (dr::sqr of the AOV) and, per pair j < k, Y_j * Y_k
//   splat    every value through the footprint, the float32 weights, the cell walks and the run reduction of dtof_splat64.h, shared with the float64 film and the aov
//            film: w = wx * wy, the term value * w a float32 product (the box filter adds the value itself and 1.f), converted to double; from there on only double
//            additions.  This file keeps what a cell receives: one weight sum per pixel that serves all planes, six sums per variant, and the pairs
//   develop  every plane but the weight divided by (W == 0 ? 1 : W) in double, into dense planes: k_develop_moments, dtof_develop.hip
// Plane order and device layout: dtof_moments.h.  Compiled with -ffp-contract=off like every kernel here.
#include "dtof_splat64.h"
#include "dtof_moments.h"

namespace dtof {

namespace {
constexpr int kMomentsBlock = 256;
constexpr int kPairs = kMaxOffsets * (kMaxOffsets - 1) / 2;
static_assert(kMaxOffsets == 4 && moment_planes(kMaxOffsets) <= kMomentCell, "the pair tables and the cell are laid out for at most four variants");
// k of pair i of (j, k) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3): two bits per entry
DTOF_D int pair_k(int i) { return (0xfb9 >> (2 * i)) & 3; }
#define DTOF_SEL4(a, j) sel(j, a##0, a##1, a##2, a##3)

// q.pos, q.res plane k at k * q.capacity and the pixel from global_lane, as k_splat_f64 reads them.  Every thread of the block stays in the kernel on the run path (the
// shuffles of run_sum are wave-wide); a thread without a lane is a run of its own that adds nothing.
__global__ __launch_bounds__(kMomentsBlock) void k_splat_moments_f64(RenderParams rp, Queues q, double *film) {
    const uint32_t i = blockIdx.x * kMomentsBlock + threadIdx.x;
    const bool valid = i < rp.n_lanes;
    const int K = rp.n_offsets;
    const Footprint f = footprint_of(rp, i, valid, q.pos);
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
    if (f.cnt > kRunCells) {
        if (valid) walk_wide(rp, f, [&](size_t pixel, float w) {
            double *c = film + (size_t) kMomentCell * pixel;
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
        });
        return;
    }
    const RunCells rc = run_cells_of(rp, f, valid);
    // The variant and pair loops stay rolled like the walk's cell loops: their counters are scalars, sel() is selects on them.
    walk_runs(rp, f, rc, [&](float w, bool write, size_t pixel) {
        double *cell = film + (size_t) kMomentCell * pixel;
        const double ws = run_sum(valid ? term(1.f, w, f.box) : 0.0, rc.dist, rc.steps);   // the weight plane's value is 1 (1.f * w is w)
        if (write) add_f64(cell, ws);
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            const float X = DTOF_SEL4(vx, k), Y = DTOF_SEL4(vy, k), Z = DTOF_SEL4(vz, k);
            const double s0 = run_sum(term(X, w, f.box), rc.dist, rc.steps);
            const double s1 = run_sum(term(Y, w, f.box), rc.dist, rc.steps);
            const double s2 = run_sum(term(Z, w, f.box), rc.dist, rc.steps);
            const double s3 = run_sum(term(X * X, w, f.box), rc.dist, rc.steps);
            const double s4 = run_sum(term(Y * Y, w, f.box), rc.dist, rc.steps);
            const double s5 = run_sum(term(Z * Z, w, f.box), rc.dist, rc.steps);
            if (write) {
                double *m = cell + 1 + 6 * k;
                add_f64(m, s0); add_f64(m + 1, s1); add_f64(m + 2, s2); add_f64(m + 3, s3); add_f64(m + 4, s4); add_f64(m + 5, s5);
            }
        }
        int slot = 1 + 6 * K;
#pragma unroll 1
        for (int pr = 0; pr < kPairs; ++pr) {
            if (pair_k(pr) >= K) continue;   // wave-uniform
            const double sp = run_sum(term(sel(pr, yy0, yy1, yy2, yy3, yy4, yy5), w, f.box), rc.dist, rc.steps);
            if (write) add_f64(cell + slot, sp);
            ++slot;
        }
    });
}
#undef DTOF_SEL4
}  // namespace

void launch_splat_moments(const RenderParams &rp, const Queues &q, double *film, hipStream_t s) {
    if (rp.n_lanes == 0) return;
    hipLaunchKernelGGL(k_splat_moments_f64, dim3((rp.n_lanes + kMomentsBlock - 1) / kMomentsBlock), dim3(kMomentsBlock), 0, s, rp, q, film);
}

}  // namespace dtof
