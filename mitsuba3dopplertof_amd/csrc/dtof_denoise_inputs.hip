// dtof_denoise_inputs.hip -- what lies between the raw films of one traversal and dtof_denoise_async, on the device:
//   denoise_inputs   : the pass mean (IMAGE) or the ToF value replicated into three channels (TOF) as the colour, the variance of every plane's luminance estimate from
//                      the moment cells, and the position / shading-normal guides from the aov cells -- every operation in the order Scene.render_denoised and
//                      harness.velocity_map_denoised evaluate it in numpy, so the denoiser's arguments are the host route's bit for bit (tests/denoise_inputs_ref.py).
//   position_extent  : per-axis min and max of the finite positions and their count, for the automatic sigma_position.  Min, max and an integer count do not depend on
//                      the order of the reduction, so the result is exact: a wave reduction, LDS across the block, then one block over the block results.
// Elementwise and bound by memory traffic: one lane per pixel, no atomics.  Compiled with -ffp-contract=off like every kernel here: no multiply-add below is fused,
// which the bit parity with numpy depends on.
#include "dtof_denoise_inputs.h"
#include "dtof_develop.h"
#include "dtof_moments.h"
#include "dtof_reconstruct.h"

namespace dtof {

namespace {
constexpr int kInputsBlock = 256, kInputsWaves = kInputsBlock / 64;
static_assert(kMomentCell == 32, "denoise_inputs_check sizes the cell films by 32 doubles per pixel");

__global__ __launch_bounds__(kInputsBlock) void k_denoise_inputs(const float *sum, const double *moments, const double *aovs, DenoiseInputsArgs a, float *colour,
                                                                 double *variance, float *normal, float *position) {
    const int64_t n = a.n_pixels, i = (int64_t) blockIdx.x * kInputsBlock + threadIdx.x;
    if (i >= n) return;
    const double *m = moments + (int64_t) kMomentCell * i;
    const double wd = develop_weight(m[0]);
    for (int32_t k = 0; k < a.n_planes; ++k) {
        float *c = colour + ((int64_t) k * n + i) * 3;
        if (a.mode == kDenoiseInputsTof) {
            const float t = tof_of(sum, n, k, i, a.n_passes, a.exposure_time);
            c[0] = t; c[1] = t; c[2] = t;
        } else {
            const float *p = sum + ((int64_t) k * n + i) * 3;
            c[0] = p[0] / a.n_passes; c[1] = p[1] / a.n_passes; c[2] = p[2] / a.n_passes;
        }
        // Y and Y^2 of variant k (dtof_moments.h: planes 1 + 6 k + 1 and 1 + 6 k + 4), developed, then harness.moment_statistics' m2 - mean^2
        const double mean = m[1 + 6 * k + 1] / wd, m2 = m[1 + 6 * k + 4] / wd;
        double v = (m2 - mean * mean) / a.n_samples;
        if (a.mode == kDenoiseInputsTof) v = v * a.time2;
        variance[(int64_t) k * n + i] = v;
    }
    // the aov cells of "p:position,n:sh_normal": the weight, position x y z, normal x y z; developed in double and rounded to float32 once
    const double *g = aovs + (int64_t) kMomentCell * i;
    const double wa = develop_weight(g[0]);
    for (int c = 0; c < 3; ++c) {
        position[3 * i + c] = (float) (g[1 + c] / wa);
        normal[3 * i + c] = (float) (g[4 + c] / wa);
    }
}

struct Extent { float lo[3], hi[3]; uint32_t count; };
__device__ __forceinline__ Extent empty_extent() { return { { INFINITY, INFINITY, INFINITY }, { -INFINITY, -INFINITY, -INFINITY }, 0u }; }
__device__ __forceinline__ void join(Extent &e, const float lo[3], const float hi[3], uint32_t count) {
    for (int c = 0; c < 3; ++c) { e.lo[c] = lo[c] < e.lo[c] ? lo[c] : e.lo[c]; e.hi[c] = hi[c] > e.hi[c] ? hi[c] : e.hi[c]; }
    e.count += count;
}
// Every lane of the block calls it (no lane has left): the wave's lanes by shuffles, the block's waves through LDS; thread 0 stores the block's record.
__device__ __forceinline__ void block_reduce_store(Extent e, uint32_t *dst) {
    __shared__ Extent waves[kInputsWaves];
    for (int off = 32; off > 0; off >>= 1) {
        float lo[3], hi[3];
        for (int c = 0; c < 3; ++c) { lo[c] = __shfl_xor(e.lo[c], off); hi[c] = __shfl_xor(e.hi[c], off); }
        const uint32_t count = (uint32_t) __shfl_xor((int) e.count, off);
        join(e, lo, hi, count);
    }
    if ((threadIdx.x & 63u) == 0) waves[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kInputsWaves; ++w) join(e, waves[w].lo, waves[w].hi, waves[w].count);
    for (int c = 0; c < 3; ++c) { dst[c] = __float_as_uint(e.lo[c]); dst[3 + c] = __float_as_uint(e.hi[c]); }
    dst[6] = e.count; dst[7] = 0u;
}

__global__ __launch_bounds__(kInputsBlock) void k_position_extent(const float *position, int64_t n, uint32_t *blocks) {
    Extent e = empty_extent();
    for (int64_t i = (int64_t) blockIdx.x * kInputsBlock + threadIdx.x; i < n; i += (int64_t) gridDim.x * kInputsBlock) {
        const float p[3] = { position[3 * i], position[3 * i + 1], position[3 * i + 2] };
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) join(e, p, p, 1u);
    }
    block_reduce_store(e, blocks + (size_t) blockIdx.x * kDenoiseExtentWords);
}
__global__ __launch_bounds__(kInputsBlock) void k_position_extent_final(const uint32_t *blocks, uint32_t n_blocks, uint32_t *extent) {
    Extent e = empty_extent();
    for (uint32_t b = threadIdx.x; b < n_blocks; b += kInputsBlock) {
        const uint32_t *r = blocks + (size_t) b * kDenoiseExtentWords;
        const float lo[3] = { __uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]) }, hi[3] = { __uint_as_float(r[3]), __uint_as_float(r[4]), __uint_as_float(r[5]) };
        join(e, lo, hi, r[6]);
    }
    block_reduce_store(e, extent);
}
}  // namespace

void launch_denoise_inputs(const DenoiseInputsArgs &a, const float *sum, const double *moments, const double *aovs, float *colour, double *variance, float *normal,
                           float *position, hipStream_t s) {
    if (a.n_pixels <= 0) return;
    hipLaunchKernelGGL(k_denoise_inputs, dim3((uint32_t) ((a.n_pixels + kInputsBlock - 1) / kInputsBlock)), dim3(kInputsBlock), 0, s, sum, moments, aovs, a, colour,
                       variance, normal, position);
}

void launch_position_extent(const float *position, int64_t n_pixels, uint32_t *block_scratch, uint32_t *extent, hipStream_t s) {
    const uint32_t blocks = denoise_extent_blocks(n_pixels);
    if (blocks) hipLaunchKernelGGL(k_position_extent, dim3(blocks), dim3(kInputsBlock), 0, s, position, n_pixels, block_scratch);
    hipLaunchKernelGGL(k_position_extent_final, dim3(1), dim3(kInputsBlock), 0, s, (const uint32_t *) block_scratch, blocks, extent);
}

}  // namespace dtof
