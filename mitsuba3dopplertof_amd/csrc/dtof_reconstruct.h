// dtof_reconstruct.h -- launcher of the reconstruction kernel (dtof_reconstruct.hip): the radial-velocity map of doppler_tutorials/src/utils/image_utils.py:140-199
// from the sum of the developed passes that launch_develop_accumulate (dtof_develop.h) leaves, and the ToF value both reconstructed maps start from.
// Kept out of dtof_kernels.h: nothing of the render kernels reads it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dtof {

constexpr int kMaxVelocityPairs = 16;   // (homodyne plane, heterodyne plane) pairs one k_velocity_map launch combines

// What k_velocity_map needs beside its buffers, passed by value.  The doubles are formed ONCE on the host, as Python forms them before numpy sees an array:
// 1.0 / exposure_time, w_g * 1e6 and the confidence floor 1e-5 * 0.0015 (image_utils.py:189 hard-codes that exposure time).
struct VelocityMapArgs {
    int32_t n_pairs;
    int32_t hom[kMaxVelocityPairs], het[kMaxVelocityPairs];   // plane indices into the sum
    float n_passes;          // (float) n_passes: the divisor of render_multi_pass (program_runner.py:31)
    float exposure_time;     // (float) T: to_tof_image multiplies a float32 image (image_utils.py:20-31)
    double inv_time, w_g_hz, conf_floor;
};

// The ToF value of pixel i of plane `plane` of the sum [planes][n][3] (k_velocity_map, and k_depth_map of dtof_depth.hip): (sum / n_passes), then luminance *
// exposure time, all in float32 (what numpy makes of Python scalars against a float32 image)
__device__ __forceinline__ float tof_of(const float *rgb_sum, int64_t n, int32_t plane, int64_t i, float n_passes, float exposure_time) {
    const float *p = rgb_sum + ((int64_t) plane * n + i) * 3;
    const float r = p[0] / n_passes, g = p[1] / n_passes, b = p[2] / n_passes;
    return ((0.2126f * r + 0.7152f * g) + 0.0722f * b) * exposure_time;
}

// tof: [2 * n_pairs][n_pixels] float32 or null; pair_maps: [n_pairs][n_pixels] double or null; velocity: [n_pixels] double
void launch_velocity_map(const float *rgb_sum, const VelocityMapArgs &a, int64_t n_pixels, float *tof, double *pair_maps, double *velocity, hipStream_t s);
// ... of double ToF planes [2 * n_pairs][n_pixels][3], channel 0 of each (the denoiser's output of the replicated ToF films): the combined map alone
void launch_velocity_map_planes(const double *planes, const VelocityMapArgs &a, int64_t n_pixels, double *velocity, hipStream_t s);

}  // namespace dtof
