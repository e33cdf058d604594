// Host check of the stream jumps behind kFactPairSamples (dtof_math.h: pcg_jump<N>; k_shade; tests/test_pair_samples.py builds and runs it):
//   1. pcg_jump<N>(state, inc) is the state after N single steps of the generator, N = 1 .. 12, for <pairs> random (state, inc) pairs and for the all-zeros and
//      all-ones states with even, odd, zero and all-ones increments (the identity holds modulo 2^64 whatever the increment);
//   2. the states k_shade reads under the fact -- offsets 3, 4 (iteration 0: s2x, s2y) and 9, 10 (iteration 1) from the state generate_lane leaves -- and the floats
//      it makes of them are those of a plain walk of six pcg_next_f32 draws per iteration; so are the states of the jumps-only loop (three steps at once, one draw,
//      the output of the next state, two steps at once), which must leave an iteration in the state after six steps.
// usage: pair_samples_check <pairs>    prints "key value" lines
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "dtof_math.h"

using dtof::kPcgMult;
using dtof::pcg_jump;
using dtof::pcg_jump6;
using dtof::pcg_next_f32;
using dtof::pcg_output_f32;

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static unsigned long long g_jump_checked = 0, g_jump_bad = 0;
template <int N> static void check_jump(uint64_t state, uint64_t inc) {
    uint64_t s = state;
    for (int i = 0; i < N; ++i) s = s * kPcgMult + inc;
    const uint64_t j = pcg_jump<N>(state, inc);
    ++g_jump_checked;
    if (j != s && g_jump_bad++ < 10) fprintf(stderr, "pcg_jump<%d>(%016llx, %016llx) = %016llx, %d steps give %016llx\n", N, (unsigned long long) state, (unsigned long long) inc, (unsigned long long) j, N, (unsigned long long) s);
}
template <int N> struct JumpsUpTo { static void run(uint64_t state, uint64_t inc) { JumpsUpTo<N - 1>::run(state, inc); check_jump<N>(state, inc); } };
template <> struct JumpsUpTo<0> { static void run(uint64_t, uint64_t) {} };

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: pair_samples_check <pairs>\n"); return 2; }
    const unsigned long long n_pairs = strtoull(argv[1], nullptr, 10);
    uint64_t rs = 0x9a17ull;

    // ---- 1. N steps at once
    const uint64_t edge[] = { 0ull, ~0ull };
    const uint64_t edge_inc[] = { 0ull, 1ull, 2ull, ~0ull, ~0ull - 1ull, 0xda3e39cb94b95bdbull };
    unsigned long long edge_cases = 0;
    for (uint64_t st : edge) for (uint64_t inc : edge_inc) { JumpsUpTo<12>::run(st, inc); ++edge_cases; }
    for (unsigned long long i = 0; i < n_pairs; ++i) { const uint64_t st = splitmix(rs), inc = splitmix(rs); JumpsUpTo<12>::run(st, i & 1u ? inc | 1u : inc); }
    unsigned long long jump6_bad = 0;
    for (int i = 0; i < 1000; ++i) { const uint64_t st = splitmix(rs), inc = splitmix(rs) | 1u; jump6_bad += pcg_jump<6>(st, inc) != pcg_jump6(st, inc); }
    printf("jump_pairs %llu\njump_edge_cases %llu\njump_checked %llu\njump_mismatches %llu\njump6_mismatches %llu\n", n_pairs, edge_cases, g_jump_checked, g_jump_bad, jump6_bad);

    // ---- 2. the offsets the kernel reads
    unsigned long long streams = 0, bad_state = 0, bad_draw = 0, bad_loop_state = 0, bad_loop_draw = 0;
    for (unsigned long long i = 0; i < n_pairs; ++i, ++streams) {
        const uint64_t s0 = i < 2 ? edge[i] : splitmix(rs), inc = splitmix(rs) | 1u;   // a PCG stream's increment is odd (pcg_seed)
        // the plain walk: six draws per iteration, three iterations
        uint64_t before[19]; float draw[18]; uint64_t s = s0;
        for (int k = 0; k < 18; ++k) { before[k] = s; draw[k] = pcg_next_f32(s, inc); }
        before[18] = s;
        // the pair's prologue: the even lane takes iteration 0's state, the odd lane iteration 1's, each steps once for s2y
        // (ONE jump whose two constants the parity selects, as k_shade writes it; it is pcg_jump<9> and pcg_jump<3>)
        constexpr uint64_t m3 = dtof::pcg_pow(3), g3 = dtof::pcg_geom(3), m9 = dtof::pcg_pow(9), g9 = dtof::pcg_geom(9);
        for (int odd = 0; odd < 2; ++odd) {
            const uint64_t sx = s0 * (odd ? m9 : m3) + inc * (odd ? g9 : g3), sy = sx * kPcgMult + inc;
            bad_state += sx != (odd ? pcg_jump<9>(s0, inc) : pcg_jump<3>(s0, inc));
            const int at = odd ? 9 : 3;
            bad_state += sx != before[at]; bad_state += sy != before[at + 1];
            bad_draw += fbits(pcg_output_f32(sx)) != fbits(draw[at]); bad_draw += fbits(pcg_output_f32(sy)) != fbits(draw[at + 1]);
        }
        // the jumps-only loop: per sampling iteration three steps at once, s2x drawn, s2y the output of the state that follows, two steps at once
        uint64_t ls = s0;
        for (int it = 0; it < 2; ++it) {
            ls = pcg_jump<3>(ls, inc);
            const float s2x = pcg_next_f32(ls, inc), s2y = pcg_output_f32(ls);
            bad_loop_draw += fbits(s2x) != fbits(draw[6 * it + 3]); bad_loop_draw += fbits(s2y) != fbits(draw[6 * it + 4]);
            ls = pcg_jump<2>(ls, inc);
            bad_loop_state += ls != before[6 * (it + 1)];
        }
    }
    printf("streams %llu\nbad_state %llu\nbad_draw %llu\nbad_loop_state %llu\nbad_loop_draw %llu\n", streams, bad_state, bad_draw, bad_loop_state, bad_loop_draw);
    return g_jump_bad || jump6_bad || bad_state || bad_draw || bad_loop_state || bad_loop_draw ? 1 : 0;
}
