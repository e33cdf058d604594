// dtof_temporal.hip -- the temporal stage of the denoiser: the previous frame's accumulated films are reprojected through a screen-space flow field,
// history that belongs to another surface is rejected (id and normal tests per bilinear tap), and mean and variance are blended with an exponential moving average
// whose weight follows the history length, as SVGF's temporal accumulation does.  The variance it hands to the spatial levels (dtof_denoise.hip) is the variance of the
// accumulated estimate.  tests/temporal_ref.py is the definition in numpy; every operation below is the double operation it names, in its order, and the file is
// compiled with -ffp-contract=off like every kernel here.
//   k_temporal : one lane per pixel, x fastest: the loads of the current frame are contiguous across a wave; the four taps of neighbouring lanes overlap and come
//                through L2.  No LDS, no atomics, no scratch (profiles/flow_resource_usage.txt).  A lane reads only inputs and writes only its own pixel.
#include "dtof_temporal.h"
#include <cfloat>

namespace dtof {

namespace {

constexpr int kTemporalBlock = 256;

struct TemporalKernelArgs {
    TemporalDeviceBuffers b;
    int64_t n; int32_t width, height;
    double alpha_min, max_length, tau_normal2;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }     // false for a NaN
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= DBL_MAX; }

// K planes; HV / HN / HI: a variance, normals, ids are present (and, with a history, their history buffers).  The history itself is a uniform branch.
template <int K, bool HV, bool HN, bool HI>
__global__ __launch_bounds__(kTemporalBlock) void k_temporal(TemporalKernelArgs a) {
    const int64_t p = (int64_t) blockIdx.x * kTemporalBlock + threadIdx.x;
    if (p >= a.n) return;
    const TemporalDeviceBuffers &b = a.b;
    const int32_t W = a.width, H = a.height;
    const int32_t y = (int32_t) (p / W), x = (int32_t) (p - (int64_t) y * W);

    // 1. the current pixel, converted; cur_ok: every word of it is finite
    double c[K][3], v[K];
    float np[3] = { 0.f, 0.f, 0.f }, idp = 0.f;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float *cf = b.colour + ((int64_t) k * a.n + p) * 3;
        for (int ch = 0; ch < 3; ++ch) { c[k][ch] = (double) cf[ch]; ok = ok && finite_d(c[k][ch]); }
        v[k] = 0.0;
        if constexpr (HV) { v[k] = b.variance[(int64_t) k * a.n + p]; ok = ok && finite_d(v[k]); }
    }
    if constexpr (HN) for (int ch = 0; ch < 3; ++ch) { np[ch] = b.normal[p * 3 + ch]; ok = ok && finite_f(np[ch]); }
    if constexpr (HI) { idp = b.ids[p]; ok = ok && finite_f(idp); }

    // 2. - 4. the four taps of the reprojected position, j outer, i inner
    double sw = 0.0, sn = 0.0, sc[K][3], sv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { sc[k][0] = sc[k][1] = sc[k][2] = 0.0; sv[k] = 0.0; }
    const float fx = b.flow[p * 2], fy = b.flow[p * 2 + 1];
    if (ok && b.h_colour != nullptr && finite_f(fx) && finite_f(fy)) {
        const double rx = (double) x - (double) fx, ry = (double) y - (double) fy;
        const double x0 = floor(rx), ax = rx - x0, y0 = floor(ry), by = ry - y0;
        // the tap loops stay loops, as in k_denoise_level: unrolled, the four taps' loads are hoisted together
#pragma unroll 1
        for (int j = 0; j < 2; ++j) {
#pragma unroll 1
            for (int i = 0; i < 2; ++i) {
                const double wt = (i ? ax : 1.0 - ax) * (j ? by : 1.0 - by);
                const double qx = x0 + (double) i, qy = y0 + (double) j;
                // decided on the doubles: a flow of 1e30 never reaches an integer conversion
                if (!(wt > 0.0) || !(qx >= 0.0 && qx <= (double) (W - 1) && qy >= 0.0 && qy <= (double) (H - 1))) continue;
                const int64_t q = (int64_t) qy * W + (int64_t) qx;
                const float len = b.h_length[q];
                if (!(len > 0.f)) continue;
                bool take = true;
                if constexpr (HI) { const float idq = b.h_ids[q]; take = take && finite_f(idq) && idq == idp; }
                if constexpr (HN) {
                    const float n0 = b.h_normal[q * 3], n1 = b.h_normal[q * 3 + 1], n2 = b.h_normal[q * 3 + 2];
                    const double d0 = (double) np[0] - (double) n0, d1 = (double) np[1] - (double) n1, d2 = (double) np[2] - (double) n2;
                    take = take && finite_f(n0) && finite_f(n1) && finite_f(n2) && ((d0 * d0 + d1 * d1) + d2 * d2) <= a.tau_normal2;
                }
                if (!take) continue;
                double hc[K][3], hv[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double *hp = b.h_colour + ((int64_t) k * a.n + q) * 3;
                    for (int ch = 0; ch < 3; ++ch) { hc[k][ch] = hp[ch]; take = take && finite_d(hc[k][ch]); }
                    hv[k] = 0.0;
                    if constexpr (HV) { hv[k] = b.h_variance[(int64_t) k * a.n + q]; take = take && finite_d(hv[k]); }
                }
                if (!take) continue;
                sw = sw + wt;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    for (int ch = 0; ch < 3; ++ch) sc[k][ch] = sc[k][ch] + wt * hc[k][ch];
                    if constexpr (HV) sv[k] = sv[k] + wt * hv[k];
                }
                sn = sn + wt * (double) len;
            }
        }
    }

    // 5. no history: the converted inputs; an invalid pixel starts no history (length 0), a valid one a new one (length 1)
    double alpha = 1.0;
    float length = ok ? 1.f : 0.f;
    if (sw > 0.0) {      // 6. (sw is a sum of weights > 0)
        const double hn = sn / sw;
        const double n1 = hn + 1.0, n = n1 < a.max_length ? n1 : a.max_length;
        const double r = 1.0 / n;
        alpha = r > a.alpha_min ? r : a.alpha_min;
        length = (float) n;
    }
    const double keep = 1.0 - alpha;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double *o = b.o_colour + ((int64_t) k * a.n + p) * 3;
        for (int ch = 0; ch < 3; ++ch) {
            const double r = sw > 0.0 ? keep * (sc[k][ch] / sw) + alpha * c[k][ch] : c[k][ch];
            o[ch] = r;
            if (b.o_colour_f32) b.o_colour_f32[((int64_t) k * a.n + p) * 3 + ch] = (float) r;
        }
        if constexpr (HV) b.o_variance[(int64_t) k * a.n + p] = sw > 0.0 ? (keep * keep) * (sv[k] / sw) + (alpha * alpha) * v[k] : v[k];
    }
    b.o_length[p] = length;
}

template <int K> void launch_temporal_k(const TemporalArgs &d, const TemporalKernelArgs &a, dim3 grid, hipStream_t s) {
    const int mask = (d.has_variance ? 1 : 0) | (d.has_normal ? 2 : 0) | (d.has_ids ? 4 : 0);
#define DTOF_TEMPORAL_CASE(M) case M: hipLaunchKernelGGL((k_temporal<K, ((M) & 1) != 0, ((M) & 2) != 0, ((M) & 4) != 0>), grid, dim3(kTemporalBlock), 0, s, a); break;
    switch (mask) {
        DTOF_TEMPORAL_CASE(0) DTOF_TEMPORAL_CASE(1) DTOF_TEMPORAL_CASE(2) DTOF_TEMPORAL_CASE(3)
        DTOF_TEMPORAL_CASE(4) DTOF_TEMPORAL_CASE(5) DTOF_TEMPORAL_CASE(6) DTOF_TEMPORAL_CASE(7)
    }
#undef DTOF_TEMPORAL_CASE
}

}  // namespace

void launch_temporal(const TemporalArgs &d, const TemporalDeviceBuffers &b, hipStream_t s) {
    TemporalKernelArgs a;
    a.b = b;
    if (!d.has_history) { a.b.h_colour = nullptr; a.b.h_variance = nullptr; a.b.h_normal = nullptr; a.b.h_ids = nullptr; a.b.h_length = nullptr; }
    a.n = (int64_t) d.width * d.height; a.width = d.width; a.height = d.height;
    a.alpha_min = d.alpha_min; a.max_length = d.max_length; a.tau_normal2 = d.tau_normal2;
    const dim3 grid((uint32_t) ((a.n + kTemporalBlock - 1) / kTemporalBlock));
    switch (d.n_planes) {
        case 1: launch_temporal_k<1>(d, a, grid, s); break;
        case 2: launch_temporal_k<2>(d, a, grid, s); break;
        case 3: launch_temporal_k<3>(d, a, grid, s); break;
        case 4: launch_temporal_k<4>(d, a, grid, s); break;
    }
}

}  // namespace dtof
