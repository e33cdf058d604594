// dtof_denoise_inputs.h -- launchers of the stage between the raw films of ONE traversal (the float32 pass sum launch_develop_accumulate leaves, the moment cells,
// the aov cells of "p:position,n:sh_normal") and the denoiser's arguments (dtof_denoise.h), and of the reduction that gives sigma_position its extent
// (dtof_denoise_inputs.hip).  tests/denoise_inputs_ref.py is the definition.  Kept out of dtof_kernels.h: nothing of the render kernels reads it.
#pragma once
#include <hip/hip_runtime.h>
#include "dtof_denoise_inputs_args.h"

namespace dtof {

// sum[K][n][3] float32, moments / aovs: n cells of kMomentCell doubles -> colour[K][n][3] float32, variance[K][n] double, normal / position [n][3] float32.
// One launch on `s`, one lane per pixel, no host wait.
void launch_denoise_inputs(const DenoiseInputsArgs &a, const float *sum, const double *moments, const double *aovs, float *colour, double *variance, float *normal,
                           float *position, hipStream_t s);
// position[n][3] -> extent[kDenoiseExtentWords]: per-axis min and max over the pixels whose three words are finite and their count (+inf, -inf and 0 when there is
// none).  `block_scratch`: denoise_extent_blocks(n) * kDenoiseExtentWords words.  Two launches on `s` (one when n == 0), no atomics, no host wait.
void launch_position_extent(const float *position, int64_t n_pixels, uint32_t *block_scratch, uint32_t *extent, hipStream_t s);

}  // namespace dtof
