// dtof_adaptive.h -- launcher of the adaptive-sampling selection (dtof_adaptive.hip): from the moment sums of every pixel (dtof_moments.h) and the samples it has had
// so far, the ascending list of the pixels whose estimated error is still above a tolerance -- the pixels a further pass would render.  A stage behind the films, like
// dtof_reconstruct.h and dtof_denoise.h.  Host code only reads this header.
//
// All in double, no fused multiply-add, the operations in the order written here (tests/adaptive_ref.py is the same text in numpy).  S = the pixel's P(K) sums:
//   per variant k   Wd = (S[0] == 0 ? 1 : S[0]); mean_k = S[1 + 6 k + 1] / Wd; m2_k = S[1 + 6 k + 4] / Wd; var_k = m2_k - mean_k * mean_k; n = (double) count
//   image           se_k = sqrt(max(var_k, 0) / n); metric = max over k of se_k / max(|mean_k|, floor); selected iff metric > tol; n == 0: metric 0, not selected
//   velocity        per pair (h, t): a = mean_h, b = mean_t, cov = S[cross(h, t)] / Wd - a * b, r = b / a,
//                   var_r = ((var_t - (2 r) cov) + (r r) var_h) / ((a a) n), slope = ((0.5 * 3e8) / (w_g 1e6)) / (T ((r - 1) (r - 1))), se = sqrt(max(var_r, 0)) slope;
//                   valid iff a != 0 && -1 < r < 0.999; a valid pair with a finite se selects iff se > tol, any other pair iff var_h > 0 || var_t > 0;
//                   selected iff any pair selects; metric = the largest finite se of the valid pairs, NaN without one
// max(x, y) is numpy's: (x >= y || x is NaN) ? x : y.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>

namespace dtof {

constexpr int kAdaptiveImage = 0, kAdaptiveVelocity = 1;
constexpr int kAdaptiveMaxPairs = 2;
constexpr uint32_t kAdaptiveBlock = 256;                      // pixels per block of the flag and scatter kernels, and counts per block of the scan
constexpr uint32_t kAdaptiveMaxPixels = 1u << 24;             // blocks of 256 pixels and two scan levels of 256 counts: every film up to 4096 x 4096

struct AdaptiveArgs {
    int32_t mode, n_variants, n_pairs;
    int32_t hom[kAdaptiveMaxPairs], het[kAdaptiveMaxPairs], cross[kAdaptiveMaxPairs];   // variant indices of a pair and the plane of its cross moment
    double tol, floor, exposure_time, w_g_mhz;
    uint32_t spp;
    // where plane p of pixel i lies: S[i * pixel_stride + p * plane_stride] -- (kMomentCell, 1) for the cell film, (1, n_pixels) for dense planes
    int64_t pixel_stride, plane_stride;
};
// the plane of sum w Y_j Y_k (j != k) among the P(K) planes of K variants (dtof_moments.h)
inline int adaptive_cross_plane(int K, int j, int k) {
    if (j > k) { const int t = j; j = k; k = t; }
    int slot = 0;
    for (int a = 0; a < 4; ++a) for (int b = a + 1; b < 4; ++b) { if (b >= K) continue; if (a == j && b == k) return 1 + 6 * K + slot; ++slot; }
    return -1;
}
// words of scratch a selection over n pixels needs: the waves' ballots and the block counts of every scan level with their prefix sums
size_t adaptive_scratch_words(uint32_t n_pixels);
// count[n] is read, and raised by spp for the selected pixels; out_pixels[n]: the ascending list, *out_n its length; metric_or_null[n].  Device pointers; launches
// on `s` that never wait on one another inside a kernel: flags + block counts, one scan launch per level, the offsets' way back down, the scatter.
void launch_adaptive_select(const AdaptiveArgs &a, const double *S, uint32_t n_pixels, uint32_t *count, uint32_t *out_pixels, uint32_t *out_n, double *metric_or_null,
                            uint32_t *scratch, hipStream_t s);

// the metric alone (count is only read; nothing is selected): one launch of the flag kernel, whose ballots and block counts land in `scratch` and are dropped
void launch_adaptive_metric(const AdaptiveArgs &a, const double *S, uint32_t n_pixels, const uint32_t *count, double *metric, uint32_t *scratch, hipStream_t s);

}  // namespace dtof
