// dtof_pixel_list.h -- what the list form of a render request (RenderRequest::pixels, dtof_host.h) cannot be combined with.  Plain C++ with no HIP type: the frame path
// (check_pixel_list, dtof_render.hip) and the C ABI's entries (dtof_abi_films.hip) fill in the facts of their request, before any device call, and
// tests/pixel_list_check.cpp drives every refusal on the host.
#pragma once
#include <cstdint>
#include <string>

namespace dtof {

struct PixelListFacts {
    bool stripes = false, row_range = false, aov = false;       // what else the request names
    bool film32 = false, film64 = false, moments = false;       // the films it renders into
    bool lane_dump = false; uint64_t dump_begin = 0, dump_n = 0;   // a lane dump and its range of virtual lanes
    uint32_t spp = 0;                                           // samples per pixel of the call (the sampler's count already taken for 0)
    uint32_t samples_per_pass = 0xffffffffu;                    // the integrator's property; 0 and 0xffffffff: one pass
    uint32_t n_pixels = 0; uint64_t crop_pixels = 0;            // the list's length, the crop window's pixels
};

// the refusal's message, or the empty string for a request that can run
inline std::string pixel_list_refusal(const PixelListFacts &f) {
    if (f.stripes) return "a pixel list cannot be combined with stripes";
    if (f.row_range) return "a pixel list cannot be combined with a row range";
    if (f.aov) return "a pixel list cannot be combined with an aov request";
    if (f.film32) return "a pixel list renders into the float64 film or the moment film, not into the float32 film";
    if (!f.lane_dump && !f.film64 && !f.moments) return "a pixel list needs a float64 film or a moment film to render into";
    if (f.spp == 0) return "sample count must be positive";
    if (f.samples_per_pass != 0xffffffffu && f.samples_per_pass != 0 && f.samples_per_pass < f.spp)
        return "a pixel list needs one pass per render: samples_per_pass below the sample count is not supported with a list";
    if (f.n_pixels > f.crop_pixels) return "a pixel list cannot hold more pixels than the crop window";
    if (f.lane_dump && (f.dump_begin % f.spp != 0 || f.dump_n % f.spp != 0 || f.dump_begin + f.dump_n > (uint64_t) f.n_pixels * f.spp))
        return "the lane dump of a pixel list covers whole pixels of the list";
    return std::string();
}

}  // namespace dtof
