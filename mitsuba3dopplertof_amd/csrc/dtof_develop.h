// dtof_develop.h -- launchers of the film develop (dtof_develop.hip): HDRFilm::develop (src/films/hdrfilm.cpp:305-406), rgb / (W == 0 ? 1 : W), of the float32 film
// and of the float64 film.  One signature shape, overloaded on the film's element type: the float32 film is divided in float32, the float64 film in double and
// rounded to float once.  Kept out of dtof_kernels.h: only the host orchestration reads it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dtof {

// The weight a developed value is divided by: W == 0 ? 1 : W (HDRFilm::develop).  The one spelling of the rule on the device: the develop kernels and the
// adaptive metric (dtof_adaptive.hip) call it.
__device__ __forceinline__ float develop_weight(float w) { return w == 0.f ? 1.f : w; }
__device__ __forceinline__ double develop_weight(double w) { return w == 0.0 ? 1.0 : w; }

// `planes` RGBW film planes `plane_stride` elements of the film's type apart (0 = dense) into the dense rgb[planes][n_pixels][3].  A float32 film is read with 16-byte
// loads (every plane 16-byte aligned), a float64 film with 8-byte loads
void launch_develop(const float *film, int32_t planes, uint64_t plane_stride, float *rgb, int64_t n_pixels, hipStream_t s);
void launch_develop(const double *film, int32_t planes, uint64_t plane_stride, float *rgb, int64_t n_pixels, hipStream_t s);
// ... stored into (first: launch_develop itself) or added in float32 to (later passes) the running sum of render_multi_pass
// (doppler_tutorials/src/program_runner.py:11-31: acc = img if acc is None else acc + img)
void launch_develop_accumulate(const float *film, int32_t planes, uint64_t plane_stride, float *rgb_sum, int64_t n_pixels, bool first, hipStream_t s);
void launch_develop_accumulate(const double *film, int32_t planes, uint64_t plane_stride, float *rgb_sum, int64_t n_pixels, bool first, hipStream_t s);
// pixel_format = rgba (hdrfilm.cpp:339-400): (R, G, B) / W of the colour film, A / W of the alpha film, into the 16-byte aligned rgba[n_pixels][4]
void launch_develop_rgba(const float *film, const float *alpha_film, float *rgba, int64_t n_pixels, hipStream_t s);
void launch_develop_rgba(const double *film, const double *alpha_film, float *rgba, int64_t n_pixels, hipStream_t s);

}  // namespace dtof
