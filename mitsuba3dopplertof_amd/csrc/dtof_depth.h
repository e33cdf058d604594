// dtof_depth.h -- launcher of the depth-map kernel (dtof_depth.hip): the wrapped phase of the homodyne I / Q films at up to four modulation frequencies and the
// path length that unwraps them, from the sum that launch_develop_accumulate (dtof_develop.h) leaves.  The definition is the one of include/dtof.h ("depth map").
// Kept out of dtof_kernels.h: nothing of the render kernels reads it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dtof {

constexpr int kMaxDepthFrequencies = 4;      // modulation frequencies one k_depth_map launch combines
constexpr int64_t kMaxDepthCandidates = 4096;   // wrap counts of the first frequency it tries per pixel (N)

// What k_depth_map needs beside its buffers, passed by value.  The doubles are formed ONCE on the host: L_j = 300.0 / w_g_mhz[j] (dopplertofpath.cpp:64).
struct DepthMapArgs {
    int32_t n_frequencies, n_candidates;                                   // F; N = (int64) floor(max_path_length / L_0) + 1 (1 when F == 1: not read)
    int32_t i_plane[kMaxDepthFrequencies], q_plane[kMaxDepthFrequencies];   // plane indices into the sum
    float n_passes, exposure_time;                                          // as VelocityMapArgs: (float) n_passes, (float) T
    double wavelength[kMaxDepthFrequencies];                                // L_j
};

// depth: [n_pixels] double; residual: [n_pixels] double or null; wraps: [F][n_pixels] int32 or null; amplitude: [F][n_pixels] double or null; phase: [F][n_pixels]
// float32 or null; tof: [2 F][n_pixels] float32 or null (plane p of the sum)
void launch_depth_map(const float *rgb_sum, const DepthMapArgs &a, int64_t n_pixels, double *depth, double *residual, int32_t *wraps, double *amplitude, float *phase,
                      float *tof, hipStream_t s);

}  // namespace dtof
