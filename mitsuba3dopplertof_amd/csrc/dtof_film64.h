// dtof_film64.h -- launcher of the float64 film's splat (dtof_film64.hip): the splat terms of ImageBlock::put (src/render/imageblock.cpp:414-531) formed in float32 as
// everywhere else, but ACCUMULATED in double.  What differs from the float32 film is the accumulator type alone; HDRFilm::develop taken in double and rounded to
// float once is the double overload of dtof_develop.h.  Kept out of dtof_kernels.h like dtof_reconstruct.h: only the host orchestration reads it.
#pragma once
#include "dtof_kernels.h"

namespace dtof {

// q.res planes 0 .. rp.n_offsets - 1 of the batch into the RGBW planes film64 + k * plane_stride_doubles (the alpha film: the caller runs it again over q.valid_out)
void launch_splat_f64(const RenderParams &rp, const Queues &q, double *film64, uint64_t plane_stride_doubles, hipStream_t s);

}  // namespace dtof
