// dtof_reconstruct.hip -- what follows the develop-accumulate (dtof_develop.hip) of a velocity-map render, on the device:
//   velocity_map : mean of the passes, to_tof_image (doppler_tutorials/src/utils/image_utils.py:20-31) in float32 (tof_of, dtof_reconstruct.h), then
//                  calc_velocity_from_homo_hetero(s) (image_utils.py:140-199) in double -- every operation in the order numpy evaluates it, so the map is the host
//                  route's bit for bit.
// Elementwise and bound by memory traffic: one lane per pixel, no LDS.  Compiled with -ffp-contract=off like every kernel here: no multiply-add below is fused, which
// the bit parity with numpy depends on.
#include "dtof_reconstruct.h"

namespace dtof {

namespace {
constexpr int kReconBlock = 256;

// _velocity_from_ratio: np.clip lets a NaN through (fmin / fmax would return the bound), then dw = ratio / (T (ratio - 1)), v = -(c / 2) dw / w_g
__device__ __forceinline__ double velocity_of(double ratio, const VelocityMapArgs &a) {
    ratio = ratio < -1.0 ? -1.0 : ratio;
    ratio = ratio > 0.999 ? 0.999 : ratio;
    const double dw = (ratio * a.inv_time) / (ratio - 1.0);
    return -(((0.5 * dw) * 3e8) / a.w_g_hz);
}

__global__ __launch_bounds__(kReconBlock) void k_velocity_map(const float *rgb_sum, VelocityMapArgs a, int64_t n, float *tof, double *pair_maps, double *velocity) {
    const int64_t i = (int64_t) blockIdx.x * kReconBlock + threadIdx.x;
    if (i >= n) return;
    double num = 0.0, den = 0.0;
    for (int32_t k = 0; k < a.n_pairs; ++k) {
        const double hom = (double) tof_of(rgb_sum, n, a.hom[k], i, a.n_passes, a.exposure_time);
        const double het = (double) tof_of(rgb_sum, n, a.het[k], i, a.n_passes, a.exposure_time);
        const double mag = fabs(hom);
        const double ratio = mag > 0.0 ? het / hom : 0.0;   // np.divide(..., out = zeros, where = |hom| > 0): false for a NaN as well
        const double conf = mag + a.conf_floor;
        num = num + ratio * conf; den = den + conf;        // from 0.0: the first term is 0.0 + x as in the reference
        if (pair_maps) pair_maps[(int64_t) k * n + i] = velocity_of(ratio, a);
    }
    velocity[i] = velocity_of(num / den, a);
    if (tof)
        for (int32_t p = 0; p < 2 * a.n_pairs; ++p) tof[(int64_t) p * n + i] = tof_of(rgb_sum, n, p, i, a.n_passes, a.exposure_time);
}

// The same map of DOUBLE ToF planes: channel 0 of planes[2 * n_pairs][n][3], the denoiser's output of the replicated ToF films.  From the ratio onwards it is
// k_velocity_map's arithmetic, i.e. harness.calc_velocity_from_homo_heteros of those planes; n_passes and exposure_time of `a` are not read.
__global__ __launch_bounds__(kReconBlock) void k_velocity_map_planes(const double *planes, VelocityMapArgs a, int64_t n, double *velocity) {
    const int64_t i = (int64_t) blockIdx.x * kReconBlock + threadIdx.x;
    if (i >= n) return;
    double num = 0.0, den = 0.0;
    for (int32_t k = 0; k < a.n_pairs; ++k) {
        const double hom = planes[((int64_t) a.hom[k] * n + i) * 3], het = planes[((int64_t) a.het[k] * n + i) * 3];
        const double mag = fabs(hom);
        const double ratio = mag > 0.0 ? het / hom : 0.0;
        const double conf = mag + a.conf_floor;
        num = num + ratio * conf; den = den + conf;
    }
    velocity[i] = velocity_of(num / den, a);
}
}  // namespace

void launch_velocity_map_planes(const double *planes, const VelocityMapArgs &a, int64_t n_pixels, double *velocity, hipStream_t s) {
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_velocity_map_planes, dim3((uint32_t) ((n_pixels + kReconBlock - 1) / kReconBlock)), dim3(kReconBlock), 0, s, planes, a, n_pixels, velocity);
}

void launch_velocity_map(const float *rgb_sum, const VelocityMapArgs &a, int64_t n_pixels, float *tof, double *pair_maps, double *velocity, hipStream_t s) {
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_velocity_map, dim3((uint32_t) ((n_pixels + kReconBlock - 1) / kReconBlock)), dim3(kReconBlock), 0, s, rgb_sum, a, n_pixels, tof, pair_maps, velocity);
}

}  // namespace dtof
