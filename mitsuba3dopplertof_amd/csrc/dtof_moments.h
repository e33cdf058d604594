// dtof_moments.h -- launchers of the per-pixel moment film (dtof_moments.hip): what the reference's `moment` integrator records (src/integrators/moment.cpp:85-104 -- the
// XYZ of every sample, srgb_to_xyz of include/mitsuba/core/spectrum.h:396-402, and its square as AOVs, filtered like the image by ImageBlock::put,
// src/render/imageblock.cpp:414-531), of every variant of ONE traversal, plus the cross moment Y_j * Y_k of every pair of variants, which has no reference counterpart.
// Terms are formed in float32 and accumulated in double like the float64 film's (dtof_film64.h).  Only the host orchestration reads this header.
//
// Planes of K variants, P(K) = 1 + 6 K + K (K - 1) / 2 sums per pixel, in this order:
//   0                          sum w
//   1 + 6 k + 0, 1, 2          sum w X_k, w Y_k, w Z_k          k = 0 .. K - 1
//   1 + 6 k + 3, 4, 5          sum w X_k^2, w Y_k^2, w Z_k^2
//   1 + 6 K + pair             sum w Y_j Y_k for (j, k) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) restricted to k < K, in that order
// DEVICE LAYOUT: one CELL of kMomentCell = 32 doubles per pixel, cell[p] = plane p (P(4) = 31; the last doubles of a cell are never written).  A cell is 256 bytes, two
// 128-byte lines, so the atomics a run of lanes issues for one pixel stay in two cache lines whatever K is.  launch_develop_moments turns the cells into the dense
// [P][n_pixels] planes the C ABI hands out.
#pragma once
#include "dtof_kernels.h"

namespace dtof {

constexpr int kMomentCell = 32;
constexpr int moment_planes(int K) { return 1 + 6 * K + K * (K - 1) / 2; }

// q.res planes 0 .. rp.n_offsets - 1 of the batch into the cells of `film` (crop_h * crop_w * kMomentCell doubles): the footprint and float32 weights of launch_splat_f64
void launch_splat_moments(const RenderParams &rp, const Queues &q, double *film, hipStream_t s);
// k_develop_moments (dtof_develop.hip, with the other develop kernels): out[p][i] = cell i's plane p, for p >= 1 divided in double by (W == 0 ? 1 : W) of the cell when `divide` (plane 0, the weight, is always copied)
void launch_develop_moments(const double *film, int32_t planes, bool divide, double *out, int64_t n_pixels, hipStream_t s);

}  // namespace dtof
