// dtof_reconstruct.h -- launchers of the two reconstruction kernels (dtof_reconstruct.hip): the developed films of the passes summed on the device, and the
// radial-velocity map of doppler_tutorials/src/utils/image_utils.py:140-199 from that sum.  Kept out of dtof_kernels.h: nothing of the render kernels reads it.
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

// rgb / (W == 0 ? 1 : W) of `planes` RGBW film planes `plane_stride_floats` apart, stored into (first) or added to (later passes) the dense sum [planes][n_pixels][3]
void launch_develop_accumulate(const float *film, int32_t planes, uint64_t plane_stride_floats, float *rgb_sum, int64_t n_pixels, bool first, hipStream_t s);
// tof: [2 * n_pairs][n_pixels] float32 or null; pair_maps: [n_pairs][n_pixels] double or null; velocity: [n_pixels] double
void launch_velocity_map(const float *rgb_sum, const VelocityMapArgs &a, int64_t n_pixels, float *tof, double *pair_maps, double *velocity, hipStream_t s);

}  // namespace dtof
