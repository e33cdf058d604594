// dtof_splat_choice.h -- which float32 splat kernel a batch takes, and with which shape.  Plain C++ with no HIP type: launch_splat (dtof_kernels.hip) asks this function
// and launches what it says, the frame path keeps the packed answer of its last frame (dtof_scene_last_splat), and tests/splat_choice_check.cpp tabulates it on the host.
#pragma once
#include <cstdint>
#include <cmath>
#include "dtof_scene.h"

namespace dtof {

enum SplatKernel : uint32_t { kSplatNone = 0, kSplatGeneric = 1, kSplatTent3 = 2, kSplatX8 = 3, kSplatPixel = 4, kSplatFused = 5 };
constexpr uint32_t kSplatBlock = 256;      // the block of k_splat_x8 / k_splat_tent3 (kBlock, dtof_device.h; launch_splat asserts it)
constexpr uint32_t kSplatSamplesPerLane = 8;   // k_splat_x8: samples a lane sums before the segment is reduced (kSplatPer)
constexpr uint32_t kSplatFillThreads = 131072u;   // k_splat_pixel: a pixel's samples are split into parts while the frame has fewer threads than this

struct SplatFacts {
    int32_t filter = FILTER_TENT; float radius = 1.f;      // FilterKind and the filter's radius
    uint32_t spp = 0, spp_log2 = 0xffffffffu;              // samples per pixel of the pass; log2 of it, 0xffffffff if it is no power of two
    uint32_t n_lanes = 0;                                  // lanes of the batch, a multiple of spp
    int splat_switch = 0;                                  // DTOF_SPLAT: 0 automatic, 1 dpp, 2 generic
};

struct SplatChoice {
    SplatKernel kernel = kSplatNone;
    uint32_t n = 0;            // the footprint is n x n pixels (1: the box filter)
    uint32_t seg = 0;          // tent3: lanes of a DPP segment; x8: seg8, the lanes that share a pixel's segment of 8 seg8 samples
    uint32_t parts = 0, chunk = 0;   // pixel: threads per pixel and samples per thread (the last part takes what is left)
    uint32_t lds = 0;          // x8: dynamic LDS bytes
    // one word: kernel (bits 0-2), min(n, 15) (3-6), log2 of seg or of parts (7-11), min(chunk, 0xfffff) (12-31)
    uint32_t packed() const {
        uint32_t p2 = kernel == kSplatPixel ? parts : seg, lg = 0;
        while (p2 > 1) { p2 >>= 1; ++lg; }
        return (uint32_t) kernel | ((n < 15u ? n : 15u) << 3) | (lg << 7) | ((chunk < 0xfffffu ? chunk : 0xfffffu) << 12);
    }
};
constexpr uint32_t kSplatFusedWord = (uint32_t) kSplatFused | (3u << 3);   // the first-bounce kernel splatted the frame's lanes itself: radius-1 tent, 3 x 3

inline SplatChoice splat_choice(const SplatFacts &f) {
    SplatChoice c;
    if (f.n_lanes == 0 || f.spp == 0) return c;
    const bool pow2 = f.spp_log2 != 0xffffffffu;
    const bool fast = f.filter == FILTER_TENT && f.radius <= 1.f && f.radius > .5f && pow2 && f.spp >= 2;
    // footprint of the filter in pixels (ImageBlock::put: the pixels within ceil(radius - 0.5) of the sample's): 1 (box), 3 or 5 take the
    // eight-samples-per-lane kernel when spp is a power of two >= 16
    const int reach = f.filter == FILTER_BOX ? 0 : (int) ceilf(f.radius - .5f);
    c.n = (uint32_t) (2 * reach + 1);
    // the Lanczos filter (default radius 3: a 7 x 7 footprint) always takes the per-lane kernel
    const bool narrow = (f.filter == FILTER_BOX || (reach >= 1 && reach <= 2)) && f.filter != FILTER_LANCZOS && f.splat_switch == 0;
    if (narrow && pow2 && f.spp >= 2 * kSplatSamplesPerLane) {
        const uint32_t seg8 = f.spp / kSplatSamplesPerLane < 64 ? f.spp / kSplatSamplesPerLane : 64;
        const uint32_t lds = (kSplatBlock / seg8) * c.n * c.n * 16u;
        if (lds <= 64u * 1024u) { c.kernel = kSplatX8; c.seg = seg8; c.lds = lds; return c; }
    }
    const bool small_pow2_tent = fast && f.spp < 2 * kSplatSamplesPerLane;   // 2, 4, 8 spp under the radius-1 tent: k_splat_tent3 (one DPP segment per pixel)
    if (narrow && !small_pow2_tent) {
        // any other sample count: one thread per pixel; enough threads to fill the chip (parts of a pixel's samples, each >= 8, when the frame is small)
        const uint32_t n_pixels = f.n_lanes / f.spp;
        uint32_t parts = 1;
        while ((uint64_t) n_pixels * parts < kSplatFillThreads && f.spp / (parts * 2) >= 8) parts *= 2;
        c.kernel = kSplatPixel; c.parts = parts; c.chunk = (f.spp + parts - 1) / parts;
        return c;
    }
    if (fast && f.splat_switch != 2) { c.kernel = kSplatTent3; c.seg = f.spp < 64 ? f.spp : 64; }
    else c.kernel = kSplatGeneric;
    return c;
}

}  // namespace dtof
