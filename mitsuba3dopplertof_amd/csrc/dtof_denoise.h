// dtof_denoise.h -- launcher of the joint variance-guided a-trous denoiser (dtof_denoise.hip): a stage behind the films, like dtof_reconstruct.h.  Kept out of
// dtof_kernels.h: nothing of the render kernels reads it.
#pragma once
#include <hip/hip_runtime.h>
#include "dtof_denoise_args.h"

namespace dtof {

// colour[K][H][W][3] float32, variance[K][H][W] double or null, normal / position [H][W][3] float32 or null -> out_colour[K][H][W][3] double, out_variance[K][H][W]
// double or null.  `scratch`: denoise_scratch_doubles(a) doubles.  1 + a.levels launches on `s`, no host wait; the last level writes the outputs itself.
// Built with -DDTOF_DENOISE_NAIVE (make variant NAME=denoise_naive DEFS=-DDTOF_DENOISE_NAIVE) the levels run one lane per pixel with every tap's record read from
// memory instead of the LDS tile: the same arithmetic, the other side of tools/time_denoise.py's A/B.  The product build holds the tiled form alone.
void launch_denoise(const DenoiseArgs &a, const float *colour, const double *variance, const float *normal, const float *position, double *out_colour,
                    double *out_variance, double *scratch, hipStream_t s);

}  // namespace dtof
