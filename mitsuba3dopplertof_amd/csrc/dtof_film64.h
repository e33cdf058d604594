// dtof_film64.h -- launchers of the float64 film (dtof_film64.hip): the splat terms of ImageBlock::put (src/render/imageblock.cpp:414-531) formed in float32 as
// everywhere else, but ACCUMULATED in double, and HDRFilm::develop (src/films/hdrfilm.cpp:305-406) taken in double and rounded to float once.  What differs from the
// float32 film is the accumulator type alone.  Kept out of dtof_kernels.h like dtof_reconstruct.h: only the host orchestration reads it.
#pragma once
#include "dtof_kernels.h"

namespace dtof {

// q.res planes 0 .. rp.n_offsets - 1 of the batch into the RGBW planes film64 + k * plane_stride_doubles (the alpha film: the caller runs it again over q.valid_out)
void launch_splat_f64(const RenderParams &rp, const Queues &q, double *film64, uint64_t plane_stride_doubles, hipStream_t s);
// (float) (RGB / (W == 0 ? 1 : W)) in double, of `planes` planes plane_stride_doubles apart (0 = dense) into the dense rgb[planes][n_pixels][3]
void launch_develop_f64(const double *film64, int32_t planes, uint64_t plane_stride_doubles, float *rgb, int64_t n_pixels, hipStream_t s);
// ... of an rgba film: (R, G, B) / W of the colour film, A / W of the alpha film
void launch_develop_rgba_f64(const double *film64, const double *alpha_film64, float *rgba, int64_t n_pixels, hipStream_t s);
// the float64-film twin of launch_develop_accumulate (dtof_reconstruct.h): the same develop, then the same float32 running sum with the same first-pass assignment
void launch_develop_accumulate_f64(const double *film64, int32_t planes, uint64_t plane_stride_doubles, float *rgb_sum, int64_t n_pixels, bool first, hipStream_t s);

}  // namespace dtof
