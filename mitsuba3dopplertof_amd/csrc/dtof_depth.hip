// dtof_depth.hip -- the range half of a correlation time-of-flight camera, on the device: from the sum of the developed passes (k_develop,
// dtof_develop.hip) the ToF values (tof_of, dtof_reconstruct.h) of the homodyne I / Q films at every modulation frequency, their wrapped phase, and -- with two or more frequencies -- the wrap
// counts that make the frequencies agree on one path length.  The definition is written out in include/dtof.h ("depth map") and restated in numpy by
// tests/depth_ref.py and harness.calc_depth_from_homodynes; every output equals theirs word for word.
// Elementwise: one lane per pixel, no LDS.  Only atan2_ of dtof_math.h (float32, the oracle's orc_atan2f bit for bit) and IEEE double + - * /, sqrt, floor and rint.
// Compiled with -ffp-contract=off like every kernel here: no multiply-add below is fused, which the equality with numpy depends on.
#include "dtof_depth.h"
#include "dtof_reconstruct.h"
#include "dtof_math.h"

namespace dtof {

namespace {
constexpr int kDepthBlock = 256;
constexpr double kTwoPiD = 6.283185307179586;

__global__ __launch_bounds__(kDepthBlock) void k_depth_map(const float *rgb_sum, DepthMapArgs a, int64_t n, double *depth, double *residual, int32_t *wraps,
                                                           double *amplitude, float *phase, float *tof) {
    const int64_t i = (int64_t) blockIdx.x * kDepthBlock + threadIdx.x;
    if (i >= n) return;
    const int F = a.n_frequencies;
    float ph[kMaxDepthFrequencies];
    double amp[kMaxDepthFrequencies], w[kMaxDepthFrequencies];
#pragma unroll
    for (int j = 0; j < kMaxDepthFrequencies; ++j) if (j < F) {
        const float I = tof_of(rgb_sum, n, a.i_plane[j], i, a.n_passes, a.exposure_time), Q = tof_of(rgb_sum, n, a.q_plane[j], i, a.n_passes, a.exposure_time);
        ph[j] = atan2_(-Q, I);
        double p = (double) ph[j];
        if (p < 0.0) p = p + kTwoPiD;
        amp[j] = sqrt((double) I * (double) I + (double) Q * (double) Q);
        w[j] = (p / kTwoPiD) * a.wavelength[j];
    }
    // the winning candidate: c, the other frequencies' e_j and every wrap count
    double best_err = 0.0, best_c = w[0], best_e[kMaxDepthFrequencies] = { 0.0, 0.0, 0.0, 0.0 }, best_m[kMaxDepthFrequencies] = { 0.0, 0.0, 0.0, 0.0 };
    bool won = F == 1;   // one frequency: path = w_0, wraps 0, residual 0
    if (F > 1) {
        for (int32_t cand = 0; cand < a.n_candidates; ++cand) {
            const double c = w[0] + (double) cand * a.wavelength[0];
            double err = 0.0, e[kMaxDepthFrequencies], m[kMaxDepthFrequencies];
#pragma unroll
            for (int j = 1; j < kMaxDepthFrequencies; ++j) if (j < F) {
                double mj = rint((c - w[j]) / a.wavelength[j]);
                if (mj < 0.0) mj = 0.0;
                m[j] = mj; e[j] = w[j] + mj * a.wavelength[j];
                const double r = e[j] - c;
                err = err + r * r;
            }
            if (won ? err < best_err : err == err) {   // strict: the first wins on ties; a NaN never wins
                won = true; best_err = err; best_c = c; best_m[0] = (double) cand;
#pragma unroll
                for (int j = 1; j < kMaxDepthFrequencies; ++j) if (j < F) { best_e[j] = e[j]; best_m[j] = m[j]; }
            }
        }
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double path = nan;
    if (won && F == 1) path = w[0];
    else if (won) {
        double S = amp[0], num = amp[0] * best_c;
#pragma unroll
        for (int j = 1; j < kMaxDepthFrequencies; ++j) if (j < F) { S = S + amp[j]; num = num + amp[j] * best_e[j]; }
        path = S > 0.0 ? num / S : 0.0;
    }
    depth[i] = won ? 0.5 * path : nan;
    if (residual) residual[i] = won ? sqrt(best_err) : nan;
#pragma unroll
    for (int j = 0; j < kMaxDepthFrequencies; ++j) if (j < F) {
        if (wraps) wraps[(int64_t) j * n + i] = won ? (int32_t) best_m[j] : -1;
        if (amplitude) amplitude[(int64_t) j * n + i] = won ? amp[j] : nan;
        if (phase) phase[(int64_t) j * n + i] = won ? ph[j] : __int_as_float(0x7fc00000);
    }
    if (tof)
        for (int32_t p = 0; p < 2 * F; ++p) tof[(int64_t) p * n + i] = tof_of(rgb_sum, n, p, i, a.n_passes, a.exposure_time);
}
}  // namespace

void launch_depth_map(const float *rgb_sum, const DepthMapArgs &a, int64_t n_pixels, double *depth, double *residual, int32_t *wraps, double *amplitude, float *phase,
                      float *tof, hipStream_t s) {
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_depth_map, dim3((uint32_t) ((n_pixels + kDepthBlock - 1) / kDepthBlock)), dim3(kDepthBlock), 0, s, rgb_sum, a, n_pixels, depth, residual, wraps,
                       amplitude, phase, tof);
}

}  // namespace dtof
