// dtof_denoise_args.h -- the argument checks and the parameter packing of the denoiser's two C-ABI entries (dtof_denoise_async, dtof_denoise).  Plain C++ with no
// HIP in it: the entries run it before their first HIP call, and tools/sanitize_denoise_args.sh compiles it with a main of its own under the host sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace dtof {

constexpr int kMaxDenoisePlanes = 4;     // colour planes filtered with one set of weights (the four films of a velocity map's traversal)
constexpr int kMaxDenoiseLevels = 6;     // a-trous levels: steps 1 .. 32
constexpr int32_t kMaxDenoiseExtent = 65535;   // width and height: the level kernel's tile rows are a 16-bit grid dimension

// What the kernels need beside their buffers.  The squares are formed ONCE on the host, in double, as tests/denoise_ref.py forms them.
struct DenoiseArgs {
    int32_t width, height, n_planes, levels;
    int32_t has_normal, has_position, has_variance;
    double sigma_normal2, sigma_position2, sigma_luminance;   // sigma_normal * sigma_normal, sigma_position * sigma_position, sigma_luminance
};

// the caller's buffers as byte ranges [p, p + bytes): device or host pointers, never dereferenced here
struct DenoiseBuffers {
    const void *colour, *variance, *normal, *position;   // inputs; the last three may be null
    const void *out_colour, *out_variance;               // outputs; the last may be null
};

inline bool denoise_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every refusal of the two entries, in the order dtof.h lists them.  Returns an empty string and fills `out` when the call can run, the message otherwise; `out` is
// written only on success.  levels / sigmas are passed as read from the caller's dtof_denoise_params (params_null: the pointer itself was null).
inline std::string denoise_check(const DenoiseBuffers &b, int n_planes, int32_t width, int32_t height, bool params_null, int32_t levels, double sigma_normal,
                                 double sigma_position, double sigma_luminance, DenoiseArgs *out) {
    if (!b.colour || !b.out_colour || params_null) return "null argument";
    if (n_planes < 1 || n_planes > kMaxDenoisePlanes) return "between 1 and 4 colour planes can be denoised jointly";
    if (levels < 1 || levels > kMaxDenoiseLevels) return "levels must be between 1 and 6";
    if (width < 1 || height < 1) return "width and height must be at least 1";
    if (width > kMaxDenoiseExtent || height > kMaxDenoiseExtent) return "width and height must not exceed 65535";
    if (b.out_variance && !b.variance) return "an output variance needs an input variance";
    if (b.normal && (!std::isfinite(sigma_normal) || !(sigma_normal > 0))) return "sigma_normal must be finite and > 0";
    if (b.position && (!std::isfinite(sigma_position) || !(sigma_position > 0))) return "sigma_position must be finite and > 0";
    if (b.variance && (!std::isfinite(sigma_luminance) || !(sigma_luminance > 0))) return "sigma_luminance must be finite and > 0";
    // the exponent divides by the squares: one that underflows to 0 or overflows would turn 0 / 0 or inf / inf into a NaN weight
    if (b.normal && (!(sigma_normal * sigma_normal > 0) || !std::isfinite(sigma_normal * sigma_normal))) return "sigma_normal squared must be a finite double > 0";
    if (b.position && (!(sigma_position * sigma_position > 0) || !std::isfinite(sigma_position * sigma_position))) return "sigma_position squared must be a finite double > 0";
    const size_t n = (size_t) width * (size_t) height;
    const size_t colour_bytes = (size_t) n_planes * n * 3 * sizeof(float), variance_bytes = (size_t) n_planes * n * sizeof(double), guide_bytes = n * 3 * sizeof(float);
    const size_t out_colour_bytes = (size_t) n_planes * n * 3 * sizeof(double);
    if ((uintptr_t) b.colour % 4 || (uintptr_t) b.normal % 4 || (uintptr_t) b.position % 4 || (uintptr_t) b.variance % 8 || (uintptr_t) b.out_colour % 8 ||
        (uintptr_t) b.out_variance % 8)
        return "misaligned buffer";
    const void *outs[2] = { b.out_colour, b.out_variance };
    const size_t out_bytes[2] = { out_colour_bytes, variance_bytes };
    const void *ins[4] = { b.colour, b.variance, b.normal, b.position };
    const size_t in_bytes[4] = { colour_bytes, variance_bytes, guide_bytes, guide_bytes };
    for (int o = 0; o < 2; ++o)
        for (int i = 0; i < 4; ++i)
            if (denoise_ranges_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return "an output buffer overlaps an input buffer";
    if (denoise_ranges_overlap(b.out_colour, out_colour_bytes, b.out_variance, variance_bytes)) return "the two output buffers overlap";
    DenoiseArgs a;
    a.width = width; a.height = height; a.n_planes = n_planes; a.levels = levels;
    a.has_normal = b.normal ? 1 : 0; a.has_position = b.position ? 1 : 0; a.has_variance = b.variance ? 1 : 0;
    a.sigma_normal2 = b.normal ? sigma_normal * sigma_normal : 1.0;
    a.sigma_position2 = b.position ? sigma_position * sigma_position : 1.0;
    a.sigma_luminance = b.variance ? sigma_luminance : 1.0;
    *out = a;
    return std::string();
}

// doubles of scratch a call needs beside its inputs and outputs: two sets of working planes (colour 3 K, luminance and variance K each when a variance is given)
// and the per-pixel guide records (4 doubles each)
inline size_t denoise_scratch_doubles(const DenoiseArgs &a) {
    const size_t n = (size_t) a.width * (size_t) a.height;
    const size_t per_set = (size_t) a.n_planes * (a.has_variance ? 5 : 3) * n;
    return 2 * per_set + 4 * n;
}

}  // namespace dtof
