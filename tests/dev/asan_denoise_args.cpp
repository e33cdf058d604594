// Stand-alone driver of the denoiser's argument checks and parameter packing (csrc/dtof_denoise_args.h) for tools/sanitize_denoise_args.sh: host code only, built with
// -fsanitize=address,undefined.  Walks the refusals of include/dtof.h and a grid of extreme arguments; prints what it counted and fails on any surprise.
#include "dtof_denoise_args.h"
#include <climits>
#include <cstdio>
#include <limits>
#include <vector>

using namespace dtof;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int k = 2, w = 6, h = 5;
    std::vector<float> colour(k * w * h * 3, 1.f), normal(w * h * 3, 1.f), position(w * h * 3, 1.f);
    std::vector<double> variance(k * w * h, 1.0), out(k * w * h * 3, 7.0), out_var(k * w * h, 7.0);
    const DenoiseBuffers good { colour.data(), variance.data(), normal.data(), position.data(), out.data(), out_var.data() };
    DenoiseArgs a;
    a.levels = -1;
    EXPECT(denoise_check(good, k, w, h, false, 5, 0.1, 1.0, 4.0, &a).empty());
    EXPECT(a.width == w && a.height == h && a.n_planes == k && a.levels == 5 && a.has_normal && a.has_position && a.has_variance);
    EXPECT(a.sigma_normal2 == 0.1 * 0.1 && a.sigma_position2 == 1.0 && a.sigma_luminance == 4.0);
    EXPECT(denoise_scratch_doubles(a) == (size_t) (2 * k * 5 + 4) * w * h);
    long refused = 0, accepted = 0;
    // every scalar at and around its bounds, with every subset of the optional buffers
    const int planes[] = { INT_MIN, -1, 0, 1, 4, 5, INT_MAX }, levels[] = { INT_MIN, 0, 1, 6, 7, INT_MAX }, extents[] = { INT_MIN, -1, 0, 1, 5, 65535, 65536, INT_MAX };
    const double sigmas[] = { nan, -inf, -1.0, -0.0, 0.0, 4.9e-324, 1e-200, 0.1, 1e200, 1.7e308, inf };
    for (int mask = 0; mask < 16; ++mask)
        for (int p : planes) for (int l : levels) for (int ww : extents) for (int hh : extents) for (double s : sigmas) {
            DenoiseBuffers b = good;
            if (!(mask & 1)) b.normal = nullptr;
            if (!(mask & 2)) b.position = nullptr;
            if (!(mask & 4)) b.variance = nullptr;
            if (!(mask & 8)) b.out_variance = nullptr;
            DenoiseArgs r; r.levels = -77;
            const std::string err = denoise_check(b, p, ww, hh, false, l, s, s, s, &r);
            if (err.empty()) {
                ++accepted;
                EXPECT(p >= 1 && p <= 4 && l >= 1 && l <= 6 && ww >= 1 && hh >= 1 && ww <= 65535 && hh <= 65535);
                EXPECT(!(mask & 8) || (mask & 4));
                EXPECT(!(mask & 7) || (s > 0 && s < inf));
                EXPECT(r.sigma_normal2 > 0 && r.sigma_normal2 < inf && r.sigma_position2 > 0 && r.sigma_position2 < inf && r.sigma_luminance > 0 && r.sigma_luminance < inf);
                EXPECT(denoise_scratch_doubles(r) >= (size_t) ww * hh * 10);
            } else {
                ++refused;
                EXPECT(r.levels == -77);      // a refusal writes nothing
            }
        }
    // null pointers, misalignment, overlaps
    DenoiseBuffers b = good; b.colour = nullptr;
    EXPECT(!denoise_check(b, k, w, h, false, 5, 0.1, 1.0, 4.0, &a).empty());
    b = good; b.out_colour = nullptr;
    EXPECT(!denoise_check(b, k, w, h, false, 5, 0.1, 1.0, 4.0, &a).empty());
    EXPECT(!denoise_check(good, k, w, h, true, 5, 0.1, 1.0, 4.0, &a).empty());
    b = good; b.out_colour = (const char *) out.data() + 4;
    EXPECT(denoise_check(b, k, w, h, false, 5, 0.1, 1.0, 4.0, &a) == "misaligned buffer");
    b = good; b.colour = (const char *) colour.data() + 1;
    EXPECT(denoise_check(b, k, w, h, false, 5, 0.1, 1.0, 4.0, &a) == "misaligned buffer");
    for (size_t shift = 0; shift < out.size(); shift += 7) {
        b = good; b.colour = (const float *) (out.data() + shift);      // the colour input begins inside the colour output
        EXPECT(denoise_check(b, k, w, h, false, 5, 0.1, 1.0, 4.0, &a) == "an output buffer overlaps an input buffer");
        b = good; b.out_variance = out.data() + shift;
        EXPECT(denoise_check(b, k, w, h, false, 5, 0.1, 1.0, 4.0, &a) == "the two output buffers overlap");
    }
    b = good; b.out_variance = variance.data();
    EXPECT(denoise_check(b, k, w, h, false, 5, 0.1, 1.0, 4.0, &a) == "an output buffer overlaps an input buffer");
    b = good; b.colour = (const float *) (out.data() + out.size());      // adjacent is not overlapping
    EXPECT(denoise_check(b, 1, 1, 1, false, 5, 0.1, 1.0, 4.0, &a).empty());
    EXPECT(!denoise_ranges_overlap(nullptr, 8, out.data(), 8) && !denoise_ranges_overlap(out.data(), 0, out.data(), 8));
    std::printf("ok accepted %ld refused %ld failures %d\n", accepted, refused, failures);
    return failures ? 1 : 0;
}
