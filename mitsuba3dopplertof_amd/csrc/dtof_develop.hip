// dtof_develop.hip -- HDRFilm::develop (src/films/hdrfilm.cpp:305-406) on the device: rgb / (W == 0 ? 1 : W) of an RGBW film.
//   developed      : the expression, once per element type of the film.  float32: one 16-byte load, the division in float32.  float64: four 8-byte loads (the
//                    float64 entries promise 8-byte alignment only), the division in double, rounded to float once.
//   k_develop      : one lane per pixel and plane into the dense [planes][n][3]; ADD = false stores (a develop, and the first pass of a running sum: acc = img, so
//                    that -0 survives and what the sum held before does not matter), ADD = true adds in float32 (acc + img, in that order)
//   k_develop_rgba : colour film and alpha film -- (A, 0, 0, W), accumulated with the same weights -- into [n][4]
//   k_develop_moments : the cells of the moment film and of the aov film (dtof_moments.h declares its launcher) into dense planes of doubles, every plane but the
//                    weight divided in double or not
// The weight rule itself is develop_weight (dtof_develop.h).  Elementwise and bound by memory traffic: no LDS.  Compiled with -ffp-contract=off like every kernel here.
#include "dtof_develop.h"
#include "dtof_moments.h"

namespace dtof {

namespace {
constexpr int kDevelopBlock = 256;

__device__ __forceinline__ float3 developed(const float *pixel) {
    const float4 f = *(const float4 *) pixel;
    const float w = develop_weight(f.w);
    return make_float3(f.x / w, f.y / w, f.z / w);
}
__device__ __forceinline__ float3 developed(const double *pixel) {
    const double w = develop_weight(pixel[3]);
    return make_float3((float) (pixel[0] / w), (float) (pixel[1] / w), (float) (pixel[2] / w));
}

template <typename T, bool ADD> __global__ __launch_bounds__(kDevelopBlock) void k_develop(const T *film, uint64_t plane_stride, float *rgb, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * kDevelopBlock + threadIdx.x;
    if (i >= n) return;
    const float3 v = developed(film + (uint64_t) blockIdx.y * plane_stride + 4 * i);
    float *o = rgb + ((int64_t) blockIdx.y * n + i) * 3;
    if (ADD) { o[0] = o[0] + v.x; o[1] = o[1] + v.y; o[2] = o[2] + v.z; }
    else { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
}

template <typename T> __global__ __launch_bounds__(kDevelopBlock) void k_develop_rgba(const T *film, const T *alpha_film, float *rgba, int64_t n) {
    const int64_t i = (int64_t) blockIdx.x * kDevelopBlock + threadIdx.x;
    if (i >= n) return;
    const float3 c = developed(film + 4 * i);
    ((float4 *) rgba)[i] = make_float4(c.x, c.y, c.z, developed(alpha_film + 4 * i).x);   // (only the alpha film's A and W are loaded)
}

// the moment film's cells (dtof_moments.h) into the dense [planes][n] doubles; blockIdx.y = the plane
__global__ __launch_bounds__(kDevelopBlock) void k_develop_moments(const double *film, double *out, int64_t n, int divide) {
    const int64_t i = (int64_t) blockIdx.x * kDevelopBlock + threadIdx.x;
    if (i >= n) return;
    const double *c = film + (int64_t) kMomentCell * i;
    const uint32_t pl = blockIdx.y;
    out[(int64_t) pl * n + i] = pl == 0 || !divide ? c[pl] : c[pl] / develop_weight(c[0]);
}

dim3 pixel_grid(int64_t n_pixels, int32_t planes) { return dim3((uint32_t) ((n_pixels + kDevelopBlock - 1) / kDevelopBlock), (uint32_t) planes); }

template <typename T, bool ADD> void develop(const T *film, int32_t planes, uint64_t plane_stride, float *rgb, int64_t n_pixels, hipStream_t s) {
    if (n_pixels == 0 || planes <= 0) return;
    hipLaunchKernelGGL((k_develop<T, ADD>), pixel_grid(n_pixels, planes), dim3(kDevelopBlock), 0, s, film, plane_stride ? plane_stride : (uint64_t) n_pixels * 4, rgb,
                       n_pixels);
}
template <typename T> void develop_rgba(const T *film, const T *alpha_film, float *rgba, int64_t n_pixels, hipStream_t s) {
    if (n_pixels == 0) return;
    hipLaunchKernelGGL(k_develop_rgba<T>, pixel_grid(n_pixels, 1), dim3(kDevelopBlock), 0, s, film, alpha_film, rgba, n_pixels);
}
}  // namespace

void launch_develop(const float *film, int32_t planes, uint64_t stride, float *rgb, int64_t n, hipStream_t s) { develop<float, false>(film, planes, stride, rgb, n, s); }
void launch_develop(const double *film, int32_t planes, uint64_t stride, float *rgb, int64_t n, hipStream_t s) { develop<double, false>(film, planes, stride, rgb, n, s); }
void launch_develop_accumulate(const float *film, int32_t planes, uint64_t stride, float *sum, int64_t n, bool first, hipStream_t s) {
    if (first) develop<float, false>(film, planes, stride, sum, n, s); else develop<float, true>(film, planes, stride, sum, n, s);
}
void launch_develop_accumulate(const double *film, int32_t planes, uint64_t stride, float *sum, int64_t n, bool first, hipStream_t s) {
    if (first) develop<double, false>(film, planes, stride, sum, n, s); else develop<double, true>(film, planes, stride, sum, n, s);
}
void launch_develop_rgba(const float *film, const float *alpha_film, float *rgba, int64_t n, hipStream_t s) { develop_rgba(film, alpha_film, rgba, n, s); }
void launch_develop_rgba(const double *film, const double *alpha_film, float *rgba, int64_t n, hipStream_t s) { develop_rgba(film, alpha_film, rgba, n, s); }
void launch_develop_moments(const double *film, int32_t planes, bool divide, double *out, int64_t n_pixels, hipStream_t s) {
    if (n_pixels <= 0 || planes <= 0 || planes > kMomentCell) return;
    hipLaunchKernelGGL(k_develop_moments, pixel_grid(n_pixels, planes), dim3(kDevelopBlock), 0, s, film, out, n_pixels, divide ? 1 : 0);
}

}  // namespace dtof
