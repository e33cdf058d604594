// dtof_denoise_inputs_args.h -- the argument checks and the parameter packing of dtof_denoise_inputs_async (the stage between the raw films of one traversal and the
// denoiser's arguments, dtof_denoise_inputs.hip), and the sigma_position the host forms from the stage's extent words.  Plain C++ with no HIP in it: the entry runs it
// before its first HIP call, and tools/sanitize_denoise_inputs_args.sh compiles it with a main of its own under the host sanitizers.
#pragma once
#include "dtof_denoise_args.h"
#include <cstring>

namespace dtof {

constexpr int kDenoiseInputsImage = 0, kDenoiseInputsTof = 1;   // DTOF_DENOISE_INPUTS_IMAGE / _TOF of include/dtof.h
constexpr int kDenoiseExtentWords = 8;                            // min x, y, z | max x, y, z (float32) | count of finite pixels (uint32) | 0
constexpr int64_t kMaxDenoiseInputsPixels = 0x7fffffff;           // the count of finite pixels is one 32-bit word

// What the kernel needs beside its buffers, passed by value.  The doubles are formed ONCE on the host, as Python forms them before numpy sees an array.
struct DenoiseInputsArgs {
    int32_t mode, n_planes;
    int64_t n_pixels;
    float n_passes;          // (float) n_passes: the divisor of the pass mean
    float exposure_time;     // (float) T: to_tof_image multiplies a float32 image; read in TOF mode only
    double n_samples;        // n_paths / n_pixels of the traversals
    double time2;            // T * T in double; read in TOF mode only
};

// the caller's buffers as addresses: device pointers, never dereferenced here
struct DenoiseInputsBuffers {
    const void *sum, *moments, *aovs;                          // inputs
    const void *colour, *variance, *normal, *position;         // outputs
    const void *extent;                                        // output, may be null: kDenoiseExtentWords words
};

// The one packing of the scalars, for arguments that passed the checks below (the entry) or the renders' own (dtof_render_denoised, dtof_render_velocity_map_denoised).
// IMAGE mode reads neither exposure_time nor time2: they are packed as 0 whatever was given.
inline DenoiseInputsArgs denoise_inputs_pack(int mode, int n_planes, int64_t n_pixels, uint32_t n_passes, double n_samples, double exposure_time) {
    const bool tof = mode == kDenoiseInputsTof;
    DenoiseInputsArgs a;
    a.mode = mode; a.n_planes = n_planes; a.n_pixels = n_pixels;
    a.n_passes = (float) n_passes; a.exposure_time = tof ? (float) exposure_time : 0.f;
    a.n_samples = n_samples; a.time2 = tof ? exposure_time * exposure_time : 0.0;
    return a;
}

// Every refusal of the entry.  Returns an empty string and fills `out` when the call can run, the message otherwise; `out` is written only on success.
inline std::string denoise_inputs_check(const DenoiseInputsBuffers &b, int mode, int n_planes, int64_t n_pixels, uint32_t n_passes, double n_samples,
                                        double exposure_time, DenoiseInputsArgs *out) {
    if (!b.sum || !b.moments || !b.aovs || !b.colour || !b.variance || !b.normal || !b.position) return "null argument";
    if (mode != kDenoiseInputsImage && mode != kDenoiseInputsTof) return "mode must be DTOF_DENOISE_INPUTS_IMAGE or DTOF_DENOISE_INPUTS_TOF";
    if (n_planes < 1 || n_planes > kMaxDenoisePlanes) return "between 1 and 4 colour planes can be denoised jointly";
    if (n_passes == 0) return "n_passes must be at least 1";
    if (!std::isfinite(n_samples) || !(n_samples > 0)) return "n_samples must be finite and > 0";
    if (mode == kDenoiseInputsTof) {
        if (!std::isfinite(exposure_time) || !(exposure_time > 0)) return "exposure_time must be finite and > 0";
        if (!std::isfinite(exposure_time * exposure_time) || !(exposure_time * exposure_time > 0)) return "exposure_time squared must be a finite double > 0";
    }
    if (n_pixels < 0) return "negative pixel count";
    if (n_pixels > kMaxDenoiseInputsPixels) return "too many pixels for one launch";
    if ((uintptr_t) b.sum % 4 || (uintptr_t) b.colour % 4 || (uintptr_t) b.normal % 4 || (uintptr_t) b.position % 4 || (uintptr_t) b.extent % 4 ||
        (uintptr_t) b.moments % 8 || (uintptr_t) b.aovs % 8 || (uintptr_t) b.variance % 8)
        return "misaligned buffer";
    const size_t n = (size_t) n_pixels, k = (size_t) n_planes;
    const void *ins[3] = { b.sum, b.moments, b.aovs };
    const size_t in_bytes[3] = { k * n * 3 * sizeof(float), n * 32 * sizeof(double), n * 32 * sizeof(double) };
    const void *outs[5] = { b.colour, b.variance, b.normal, b.position, b.extent };
    const size_t out_bytes[5] = { k * n * 3 * sizeof(float), k * n * sizeof(double), n * 3 * sizeof(float), n * 3 * sizeof(float), kDenoiseExtentWords * sizeof(uint32_t) };
    for (int o = 0; o < 5; ++o) {
        for (int i = 0; i < 3; ++i)
            if (denoise_ranges_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return "an output buffer overlaps an input buffer";
        for (int p = 0; p < o; ++p)
            if (denoise_ranges_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return "two output buffers overlap";
    }
    *out = denoise_inputs_pack(mode, n_planes, n_pixels, n_passes, n_samples, exposure_time);
    return std::string();
}

// Blocks of the extent reduction's first pass over n pixels (256 lanes each, grid-stride), and so the kDenoiseExtentWords-word records of scratch it needs
constexpr uint32_t kMaxDenoiseExtentBlocks = 1024;
inline uint32_t denoise_extent_blocks(int64_t n_pixels) {
    if (n_pixels <= 0) return 0;
    if (n_pixels >= (int64_t) kMaxDenoiseExtentBlocks * 256) return kMaxDenoiseExtentBlocks;   // (before the rounding up: no count overflows it)
    return (uint32_t) ((n_pixels + 255) / 256);
}

// The extent words the reduction leaves -> sigma_position as Denoiser.__call__ computes it from the position plane: extent = the largest per-axis
// (double) max - (double) min over the pixels whose three position words are finite, 0 when there is none; 1 % of it, or 1.0 when it is not above 0.
inline double denoise_extent_of(const uint32_t words[kDenoiseExtentWords]) {
    if (words[6] == 0) return 0.0;
    float v[6];
    std::memcpy(v, words, sizeof v);
    double extent = (double) v[3] - (double) v[0];
    for (int c = 1; c < 3; ++c) { const double d = (double) v[3 + c] - (double) v[c]; if (d > extent) extent = d; }
    return extent;
}
inline double denoise_sigma_position_of(const uint32_t words[kDenoiseExtentWords]) {
    const double extent = denoise_extent_of(words);
    return extent > 0 ? 0.01 * extent : 1.0;
}

}  // namespace dtof
