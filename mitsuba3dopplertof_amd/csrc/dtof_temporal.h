// dtof_temporal.h -- launcher of the denoiser's temporal stage (dtof_temporal.hip): a stage behind the films and in front of the spatial levels of dtof_denoise.h.
// Kept out of dtof_kernels.h: nothing of the render kernels reads it.
#pragma once
#include <hip/hip_runtime.h>
#include "dtof_temporal_args.h"

namespace dtof {

// the buffers of dtof_temporal_buffers as DEVICE pointers, typed
struct TemporalDeviceBuffers {
    const float *colour; const double *variance; const float *normal, *ids, *flow;
    const double *h_colour, *h_variance; const float *h_normal, *h_ids, *h_length;
    double *o_colour, *o_variance; float *o_length, *o_colour_f32;
};

// One launch of k_temporal on `s`, no host wait, no scratch.  `a` comes from temporal_check over the same buffers.
void launch_temporal(const TemporalArgs &a, const TemporalDeviceBuffers &b, hipStream_t s);

}  // namespace dtof
