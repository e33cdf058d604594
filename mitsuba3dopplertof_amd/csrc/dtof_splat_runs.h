// dtof_splat_runs.h -- what the double-accumulating splat kernels (dtof_film64.hip, dtof_moments.hip) share: the runs of lanes with one footprint anchor and their
// wave reduction, so that a run issues ONE atomic per cell and sum instead of one per lane.  Device code only; included by those two files.
#pragma once
#include "dtof_device.h"

namespace dtof {

constexpr int kRunCells = 5;   // footprints up to 5 x 5 pixels (radius <= 2.5) are reduced per run of lanes; wider ones take one atomic per lane and cell

// The lanes of a wave are cut into RUNS of consecutive lanes that share a footprint anchor (the samples of a pixel are consecutive lanes and almost always share it;
// a run ends at the wave's end, at a lane of another pixel, or at a sample whose position rounded into the next pixel).  dist: the lane's distance from the head of
// its run; steps: bit s set = some lane of the wave has dist >= 2^s (wave-uniform).  -> in the LAST lane of every run the sum of v over the run, added up as a
// Hillis-Steele tree: after step s a lane holds the sum of the min(2^(s+1), dist + 1) values that end at it.
DTOF_D double run_sum(double v, uint32_t dist, uint32_t steps) {
#pragma unroll
    for (uint32_t s = 0; s < 6; ++s)
        if ((steps >> s) & 1u) {
            const double up = __shfl_up(v, 1u << s);
            if (dist >= (1u << s)) v = v + up;
        }
    return v;
}

// a[j] of a small register array for a wave-uniform j, without indexing the registers
template <int N> DTOF_D float pick(const float (&a)[N], int j) {
    float v = a[0];
#pragma unroll
    for (int m = 1; m < N; ++m) v = j == m ? a[m] : v;
    return v;
}

DTOF_D void add_f64(double *p, double v) { if (v != 0.0) atomicAdd(p, v); }   // x + (+-0) = x, and the film starts at +0: skipping a zero changes no bit

// The runs of a wave.  Every lane of the wave calls this (the shuffles and ballots are wave-wide); a thread without a lane is a run of its own.
struct Runs { uint32_t dist, steps; bool last; };
DTOF_D Runs find_runs(int ax, int ay, bool valid) {
    // a lane heads a run if it is the wave's first, has no sample, follows a lane without one or a lane with another anchor
    const uint32_t wl = __lane_id();
    const int pax = __shfl_up(ax, 1), pay = __shfl_up(ay, 1), pvalid = __shfl_up((int) valid, 1);
    const bool head = wl == 0 || !valid || !pvalid || pax != ax || pay != ay;
    const unsigned long long heads = __ballot(head);   // bit 0 is always set
    const uint32_t run_first = 63u - (uint32_t) __builtin_clzll(heads & (~0ull >> (63u - wl)));
    Runs r;
    r.dist = wl - run_first;
    r.last = wl == 63u || ((heads >> (wl + 1u)) & 1ull);
    r.steps = 0;
#pragma unroll
    for (uint32_t s = 0; s < 6; ++s) r.steps |= __ballot(r.dist >= (1u << s)) != 0ull ? 1u << s : 0u;
    return r;
}

}  // namespace dtof
