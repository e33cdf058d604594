// Host check of the integer identities behind the sampling facts of k_shade (dtof_kernels.h: kFactPow2Strata, kFactStratifiedPairs, kFactWavePixel; tests/test_sampling_facts.py
// builds and runs it):
//   1. permute_kensler_pow2(index, n, seed) == permute_kensler(index, n, seed, make_fastdiv(n)) for every power of two n in [2, 4096], every index < n and <seeds> seeds,
//      0 and 0xffffffff among them; each form is also checked to be a permutation of [0, n) for the first seeds;
//   2. the shifts and masks generate_lane / next_time use under the facts equal the fdiv forms for every lane of a <width> x <height> frame of <spp> samples per pixel
//      (spp a power of two, time_correlate_number = path_correlate_number = 2).
// usage: sampling_facts_check <seeds> <width> <height> <spp>    prints "key value" lines
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dtof_math.h"

using dtof::FastDiv;
using dtof::fdiv;
using dtof::make_fastdiv;

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char **argv) {
    if (argc < 5) { fprintf(stderr, "usage: sampling_facts_check <seeds> <width> <height> <spp>\n"); return 2; }
    const uint32_t n_seeds = (uint32_t) strtoul(argv[1], nullptr, 10), W = (uint32_t) strtoul(argv[2], nullptr, 10), H = (uint32_t) strtoul(argv[3], nullptr, 10), spp = (uint32_t) strtoul(argv[4], nullptr, 10);
    uint32_t spp_log2 = 0; while ((1u << spp_log2) < spp) ++spp_log2;
    if (spp < 2 || (1u << spp_log2) != spp) { fprintf(stderr, "spp must be a power of two >= 2\n"); return 2; }

    // ---- 1. the straight-line Kensler form
    std::vector<uint32_t> seeds = { 0u, 0xffffffffu, 1u, 0x80000000u, 0x0000ffffu, 0xffff0000u };
    uint64_t st = 0x5a17ull;
    while (seeds.size() < n_seeds) seeds.push_back((uint32_t) splitmix(st));
    unsigned long long evaluated = 0, mismatches = 0, not_permutation = 0, sizes = 0;
    std::vector<uint8_t> seen;
    for (uint32_t n = 2; n <= 4096; n <<= 1, ++sizes) {
        const FastDiv dn = make_fastdiv(n);
        for (size_t s = 0; s < seeds.size(); ++s) {
            const bool permutation = s < 64;
            if (permutation) seen.assign(n, 0);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t a = dtof::permute_kensler(i, n, seeds[s], dn), b = dtof::permute_kensler_pow2(i, n, seeds[s]);
                ++evaluated;
                if (a != b) { if (mismatches++ < 10) fprintf(stderr, "kensler: n %u index %u seed %08x: %u != %u\n", n, i, seeds[s], a, b); }
                if (permutation && b < n) seen[b]++;
            }
            if (permutation) for (uint32_t i = 0; i < n; ++i) if (seen[i] != 1) { ++not_permutation; break; }
        }
    }
    printf("kensler_sizes %llu\nkensler_seeds %zu\nkensler_evaluated %llu\nkensler_mismatches %llu\nkensler_not_permutation %llu\n", sizes, seeds.size(), evaluated, mismatches, not_permutation);

    // ---- 2. the lane mappings: pixel and sample index (kFactWavePixel), pair and member (kFactStratifiedPairs)
    const FastDiv d_spp = make_fastdiv(spp), d_two = make_fastdiv(2u);
    unsigned long long lanes = 0, bad_pix = 0, bad_si = 0, bad_quo = 0, bad_rem = 0, bad_pair = 0, bad_wave = 0;
    const uint32_t n_lanes = W * H * spp;
    for (uint32_t lane = 0; lane < n_lanes; ++lane, ++lanes) {
        const uint32_t pix = fdiv(lane, d_spp), si = lane - pix * spp;               // generate_lane, the run-time forms
        const uint32_t quo = fdiv(si, d_two), rem = si - quo * 2u;                   // next_time: si / tcn, si % tcn
        const uint32_t pair = fdiv(lane, d_two);                                      // generate_lane: lane / pcn
        bad_pix += (lane >> spp_log2) != pix; bad_si += (lane & (spp - 1u)) != si;
        bad_quo += (si >> 1) != quo; bad_rem += (si & 1u) != rem; bad_pair += (lane >> 1) != pair;
        // the pixel of a 64-aligned wave's first lane is the pixel of every lane of it (spp a multiple of 64)
        if (spp >= 64) bad_wave += ((lane & ~63u) >> spp_log2) != pix;
    }
    printf("lanes %llu\nbad_pix %llu\nbad_si %llu\nbad_quo %llu\nbad_rem %llu\nbad_pair %llu\nbad_wave %llu\n", lanes, bad_pix, bad_si, bad_quo, bad_rem, bad_pair, bad_wave);
    return mismatches || not_permutation || bad_pix || bad_si || bad_quo || bad_rem || bad_pair || bad_wave ? 1 : 0;
}
