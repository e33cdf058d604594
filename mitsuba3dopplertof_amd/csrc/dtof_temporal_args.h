// dtof_temporal_args.h -- the argument checks and the parameter packing of the temporal stage's two C-ABI entries (dtof_denoise_temporal_async,
// dtof_denoise_temporal).  Plain C++ with no HIP in it, like dtof_denoise_args.h: the entries run it before their first HIP call, and tests/temporal_args_check.cpp
// drives it shape by shape on the host.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace dtof {

constexpr int kMaxTemporalPlanes = 4;            // colour planes blended with one set of tap weights (the four films of a velocity map's traversal)
constexpr int32_t kMaxTemporalExtent = 65535;    // width and height, as for the spatial stage behind it

// the caller's buffers (dtof_temporal_buffers): device or host pointers, never dereferenced here
struct TemporalBuffers {
    const void *colour, *variance, *normal, *ids, *flow;                  // the current frame; variance, normal, ids may be null
    const void *h_colour, *h_variance, *h_normal, *h_ids, *h_length;      // the history: all null (a first frame) or exactly those whose current buffer is present
    const void *o_colour, *o_variance, *o_length, *o_colour_f32;          // outputs; o_variance iff variance, o_colour_f32 optional
};

// What the kernel needs beside its buffers.  The square is formed ONCE on the host, in double, as tests/temporal_ref.py forms it.
struct TemporalArgs {
    int32_t width, height, n_planes;
    int32_t has_variance, has_normal, has_ids, has_history;
    double alpha_min, max_length, tau_normal2;   // tau_normal2 = tau_normal * tau_normal (1 without normals)
};

inline bool temporal_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Every refusal of the two entries, in the order dtof.h lists them.  Returns an empty string and fills `out` when the call can run, the message otherwise; `out` is
// written only on success.  alpha_min / max_length / tau_normal are passed as read from the caller's dtof_temporal_params (params_null: the pointer itself was null).
inline std::string temporal_check(const TemporalBuffers &b, int n_planes, int32_t width, int32_t height, bool params_null, double alpha_min, double max_length,
                                  double tau_normal, TemporalArgs *out) {
    if (n_planes < 1 || n_planes > kMaxTemporalPlanes) return "between 1 and 4 colour planes can be accumulated jointly";
    if (width < 1 || height < 1) return "width and height must be at least 1";
    if (width > kMaxTemporalExtent || height > kMaxTemporalExtent) return "width and height must not exceed 65535";
    if (!b.colour || !b.flow || !b.o_colour || !b.o_length || params_null) return "null argument";
    const bool history = b.h_colour || b.h_variance || b.h_normal || b.h_ids || b.h_length;
    if (history && (!b.h_colour || !b.h_length || (b.variance && !b.h_variance) || (b.normal && !b.h_normal) || (b.ids && !b.h_ids)))
        return "the history must be all null or hold every buffer of the current frame's";
    if ((b.h_variance && !b.variance) || (b.h_normal && !b.normal) || (b.h_ids && !b.ids)) return "a history buffer needs the current frame's buffer";
    if (b.o_variance && !b.variance) return "an output variance needs an input variance";
    if (b.variance && !b.o_variance) return "an input variance needs an output variance";
    const size_t n = (size_t) width * (size_t) height, k = (size_t) n_planes;
    const void *all[14] = { b.colour, b.variance, b.normal, b.ids, b.flow, b.h_colour, b.h_variance, b.h_normal, b.h_ids, b.h_length,
                            b.o_colour, b.o_variance, b.o_length, b.o_colour_f32 };
    const size_t word[14] = { 4, 8, 4, 4, 4, 8, 8, 4, 4, 4, 8, 8, 4, 4 };
    const size_t bytes[14] = { k * n * 3 * 4, k * n * 8, n * 3 * 4, n * 4, n * 2 * 4, k * n * 3 * 8, k * n * 8, n * 3 * 4, n * 4, n * 4,
                               k * n * 3 * 8, k * n * 8, n * 4, k * n * 3 * 4 };
    for (int i = 0; i < 14; ++i)
        if ((uintptr_t) all[i] % word[i]) return "misaligned buffer";
    for (int o = 10; o < 14; ++o) {
        for (int i = 0; i < 10; ++i)
            if (temporal_ranges_overlap(all[o], bytes[o], all[i], bytes[i])) return "an output buffer overlaps an input buffer";
        for (int i = o + 1; i < 14; ++i)
            if (temporal_ranges_overlap(all[o], bytes[o], all[i], bytes[i])) return "two output buffers overlap";
    }
    if (!std::isfinite(alpha_min) || !(alpha_min > 0) || !(alpha_min <= 1)) return "alpha_min must be in (0, 1]";
    if (!std::isfinite(max_length) || !(max_length >= 1)) return "max_length must be finite and >= 1";
    if (b.normal && (!std::isfinite(tau_normal) || !(tau_normal > 0))) return "tau_normal must be finite and > 0";
    if (b.normal && (!(tau_normal * tau_normal > 0) || !std::isfinite(tau_normal * tau_normal))) return "tau_normal squared must be a finite double > 0";
    TemporalArgs a;
    a.width = width; a.height = height; a.n_planes = n_planes;
    a.has_variance = b.variance ? 1 : 0; a.has_normal = b.normal ? 1 : 0; a.has_ids = b.ids ? 1 : 0; a.has_history = history ? 1 : 0;
    a.alpha_min = alpha_min; a.max_length = max_length; a.tau_normal2 = b.normal ? tau_normal * tau_normal : 1.0;
    *out = a;
    return std::string();
}

}  // namespace dtof
