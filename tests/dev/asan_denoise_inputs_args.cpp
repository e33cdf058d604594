// Stand-alone driver of the argument checks and parameter packing of dtof_denoise_inputs_async and of the sigma_position formed from the extent words
// (csrc/dtof_denoise_inputs_args.h) for tools/sanitize_denoise_inputs_args.sh: host code only, built with -fsanitize=address,undefined.  Walks the bounds of every
// scalar with every subset of the optional buffers; prints what it counted and fails on any surprise.
#include "dtof_denoise_inputs_args.h"
#include <climits>
#include <cstdio>
#include <limits>
#include <vector>

using namespace dtof;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void words_of(uint32_t w[kDenoiseExtentWords], const float lo[3], const float hi[3], uint32_t count) {
    std::memcpy(w, lo, 12); std::memcpy(w + 3, hi, 12); w[6] = count; w[7] = 0;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int k = 2; const int64_t n = 30;
    std::vector<float> sum(k * n * 3, 1.f), colour(k * n * 3, 7.f), normal(n * 3, 7.f), position(n * 3, 7.f);
    std::vector<double> moments(n * 32, 1.0), aovs(n * 32, 1.0), variance(k * n, 7.0);
    std::vector<uint32_t> extent(kDenoiseExtentWords, 7u);
    const DenoiseInputsBuffers good { sum.data(), moments.data(), aovs.data(), colour.data(), variance.data(), normal.data(), position.data(), extent.data() };
    DenoiseInputsArgs a;
    EXPECT(denoise_inputs_check(good, kDenoiseInputsTof, k, n, 3, 12.0, 0.0015, &a).empty());
    EXPECT(a.mode == kDenoiseInputsTof && a.n_planes == k && a.n_pixels == n && a.n_passes == 3.f && a.exposure_time == (float) 0.0015 && a.n_samples == 12.0 &&
           a.time2 == 0.0015 * 0.0015);
    long refused = 0, accepted = 0;
    // every scalar at and around its bounds, with the optional buffer present and absent
    const int modes[] = { INT_MIN, -1, 0, 1, 2, INT_MAX }, planes[] = { INT_MIN, -1, 0, 1, 4, 5, INT_MAX };
    const int64_t pixels[] = { INT64_MIN, -1, 0, 1, 30 };      // counts the buffers above hold; larger ones follow with far-apart fake addresses
    const uint32_t passes[] = { 0u, 1u, 2u, 0xffffffffu };
    const double reals[] = { nan, -inf, -1.0, -0.0, 0.0, 4.9e-324, 1e-200, 0.0015, 1e200, 1.7e308, inf };
    for (int with_extent = 0; with_extent < 2; ++with_extent)
        for (int m : modes) for (int p : planes) for (int64_t px : pixels) for (uint32_t np : passes) for (double ns : reals) for (double t : reals) {
            DenoiseInputsBuffers b = good;
            if (!with_extent) b.extent = nullptr;
            if (p > k) { b.sum = (const void *) 0x10000000; b.colour = (const void *) 0x20000000; b.variance = (const void *) 0x30000000; }      // K beyond what the vectors hold
            DenoiseInputsArgs r; r.n_planes = -77;
            const std::string err = denoise_inputs_check(b, m, p, px, np, ns, t, &r);
            if (err.empty()) {
                ++accepted;
                EXPECT((m == 0 || m == 1) && p >= 1 && p <= 4 && px >= 0 && np >= 1 && ns > 0 && ns < inf);
                EXPECT(m == 0 || (t > 0 && t < inf && r.time2 > 0 && r.time2 < inf));
                EXPECT(m == 1 || (r.exposure_time == 0.f && r.time2 == 0.0));      // IMAGE mode reads neither: packed as 0 whatever was given
                EXPECT(r.n_planes == p && r.n_pixels == px && r.n_passes == (float) np && r.n_samples == ns);
                EXPECT(denoise_extent_blocks(px) <= kMaxDenoiseExtentBlocks && (int64_t) denoise_extent_blocks(px) * 256 >= (px < 1024 * 256 ? px : 1024 * 256));
            } else {
                ++refused;
                EXPECT(r.n_planes == -77);      // a refusal writes nothing
            }
        }
    // pixel counts up to and beyond the limit, with fake addresses far enough apart for every size
    const int64_t big[] = { 4097, 0x7ffffffe, 0x7fffffff, 0x80000000ll, INT64_MAX };
    for (int64_t px : big) {
        const DenoiseInputsBuffers b { (const void *) 0x1000000000ull, (const void *) 0x100000000000ull, (const void *) 0x200000000000ull, (const void *) 0x300000000000ull,
                                       (const void *) 0x400000000000ull, (const void *) 0x500000000000ull, (const void *) 0x600000000000ull, nullptr };
        DenoiseInputsArgs r; r.n_planes = -77;
        const std::string err = denoise_inputs_check(b, kDenoiseInputsImage, 4, px, 1, 1.0, nan, &r);
        if (px <= kMaxDenoiseInputsPixels) { ++accepted; EXPECT(err.empty() && r.n_pixels == px); } else { ++refused; EXPECT(err == "too many pixels for one launch" && r.n_planes == -77); }
        EXPECT(denoise_extent_blocks(px) == (px == 4097 ? 17u : kMaxDenoiseExtentBlocks));
    }
    EXPECT(denoise_extent_blocks(0) == 0 && denoise_extent_blocks(1) == 1 && denoise_extent_blocks(256) == 1 && denoise_extent_blocks(257) == 2 && denoise_extent_blocks(-5) == 0);
    // null pointers, misalignment, overlaps
    for (int which = 0; which < 7; ++which) {
        DenoiseInputsBuffers b = good;
        const void **p[7] = { &b.sum, &b.moments, &b.aovs, &b.colour, &b.variance, &b.normal, &b.position };
        *p[which] = nullptr;
        EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, k, n, 1, 1.0, 1.0, &a) == "null argument");
    }
    DenoiseInputsBuffers b = good; b.variance = (const char *) variance.data() + 4;
    EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, k, n, 1, 1.0, 1.0, &a) == "misaligned buffer");
    b = good; b.extent = (const char *) extent.data() + 2;
    EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, k, n, 1, 1.0, 1.0, &a) == "misaligned buffer");
    b = good; b.sum = (const char *) sum.data() + 1;
    EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, k, n, 1, 1.0, 1.0, &a) == "misaligned buffer");
    for (size_t shift = 0; shift < sum.size(); shift += 7) {
        b = good; b.colour = sum.data() + shift;      // the colour output begins inside the sum
        EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, k, n, 1, 1.0, 1.0, &a) == "an output buffer overlaps an input buffer");
    }
    for (size_t shift = 0; shift < position.size(); shift += 5) {
        b = good; b.normal = position.data() + shift;
        EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, k, n, 1, 1.0, 1.0, &a) == "two output buffers overlap");
    }
    b = good; b.extent = moments.data() + 3;
    EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, k, n, 1, 1.0, 1.0, &a) == "an output buffer overlaps an input buffer");
    b = good; b.colour = sum.data() + sum.size();      // adjacent is not overlapping
    EXPECT(denoise_inputs_check(b, kDenoiseInputsImage, 1, 1, 1, 1.0, 1.0, &a).empty());
    // sigma_position from the extent words
    uint32_t w[kDenoiseExtentWords];
    const float finf = std::numeric_limits<float>::infinity(), fmax = std::numeric_limits<float>::max();
    { const float lo[3] = { finf, finf, finf }, hi[3] = { -finf, -finf, -finf }; words_of(w, lo, hi, 0); EXPECT(denoise_extent_of(w) == 0.0 && denoise_sigma_position_of(w) == 1.0); }
    { const float lo[3] = { 1.5f, -2.f, 0.f }, hi[3] = { 1.5f, -2.f, 0.f }; words_of(w, lo, hi, 1); EXPECT(denoise_extent_of(w) == 0.0 && denoise_sigma_position_of(w) == 1.0); }
    { const float lo[3] = { 0.f, -0.f, 0.f }, hi[3] = { -0.f, 0.f, 0.f }; words_of(w, lo, hi, 9); EXPECT(denoise_sigma_position_of(w) == 1.0); }
    { const float lo[3] = { -1.f, 0.f, 2.f }, hi[3] = { 1.f, 5.f, 2.5f }; words_of(w, lo, hi, 7); EXPECT(denoise_extent_of(w) == 5.0 && denoise_sigma_position_of(w) == 0.01 * 5.0); }
    { const float lo[3] = { -fmax, 0.f, 0.f }, hi[3] = { fmax, 0.f, 0.f }; words_of(w, lo, hi, 2);      // the difference is formed in double: no overflow
      EXPECT(denoise_extent_of(w) == 2.0 * (double) fmax && denoise_sigma_position_of(w) == 0.01 * (2.0 * (double) fmax)); }
    { const float lo[3] = { 0.f, 0.f, 0.f }, hi[3] = { 1.4e-45f, 0.f, 0.f }; words_of(w, lo, hi, 2); EXPECT(denoise_sigma_position_of(w) > 0 && denoise_sigma_position_of(w) < 1e-45); }
    std::printf("ok accepted %ld refused %ld failures %d\n", accepted, refused, failures);
    return failures ? 1 : 0;
}
