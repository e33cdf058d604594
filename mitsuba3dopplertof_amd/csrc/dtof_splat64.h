// dtof_splat64.h -- what the double-accumulating splat kernels (k_splat_f64 of dtof_film64.hip, k_splat_moments_f64 of dtof_moments.hip, k_aov of dtof_aov.hip) share:
// ImageBlock::put (src/render/imageblock.cpp:414-531) with a double accumulator, up to the planes a kernel adds per cell.
//   footprint   the anchor, the extent and the filter offsets of a lane's splat (footprint_of), and the term a value contributes to a cell (term)
//   wide walk   footprints wider than 5 x 5 (the Lanczos filter's 7 x 7): every in-bounds cell of the lane's own footprint, one atomic per lane, cell and plane
//   run walk    the runs of lanes with one footprint anchor (find_runs), their ten weights in registers (run_cells_of) and the cells of the run's footprint
//               (walk_runs); a kernel sums each plane's terms over the run (run_sum) and the run's last lane issues ONE atomic per cell and plane (add_f64)
// Both walks hand every cell to a callable of the kernel, which adds the kernel's planes.  Device code only; included by those three files.
#pragma once
#include "dtof_device.h"

namespace dtof {

constexpr int kRunCells = 5;   // footprints up to 5 x 5 pixels (radius <= 2.5) are reduced per run of lanes; wider ones take one atomic per lane and cell

// Value j of a few registers for a wave-uniform j.  Scalars and a chain of selects, not an indexed array: with the many selects of the moment film the optimiser turned
// the chains over a private array back into an indexed load, and the array into LDS and scratch.  All three kernels stay free of both with this form
// (profiles/splat64_family_resource_usage.txt).
DTOF_D float sel(int j, float a0, float a1, float a2, float a3) { float v = a0; v = j == 1 ? a1 : v; v = j == 2 ? a2 : v; return j == 3 ? a3 : v; }
DTOF_D float sel(int j, float a0, float a1, float a2, float a3, float a4) { const float v = sel(j, a0, a1, a2, a3); return j == 4 ? a4 : v; }
DTOF_D float sel(int j, float a0, float a1, float a2, float a3, float a4, float a5) { const float v = sel(j, a0, a1, a2, a3, a4); return j == 5 ? a5 : v; }

// The footprint of a lane in film coordinates (splat_lane, dtof_device.h): cnt x cnt cells from (ax, ay); cell (xs, ys) weighs filter(relx + xs) * filter(rely + ys).
// The box filter splats at the lane's OWN pixel -- read from global_lane, so a render of a pixel list lands where its list says -- and adds the value itself.
struct Footprint { int ax, ay, cnt; float relx, rely; bool box; };
DTOF_D Footprint footprint_of(const RenderParams &rp, uint32_t i, bool valid, const float2 *pos) {
    Footprint f;
    f.box = rp.filter == FILTER_BOX;
    const int n = f.box ? 0 : (int) ceilf(rp.filter_radius - .5f);
    f.cnt = 2 * n + 1; f.relx = 0.f; f.rely = 0.f;
    const float2 p = valid ? pos[i] : make_float2(0.f, 0.f);
    if (f.box) {
        const uint32_t pix = fdiv(global_lane(rp, rp.lane_base + (valid ? i : 0u)), rp.d_spp);
        f.ay = (int) fdiv(pix, rp.d_w); f.ax = (int) (pix - (uint32_t) rp.crop_w * (uint32_t) f.ay);
    } else {
        const int pix = (int) floorf(p.x) - n, piy = (int) floorf(p.y) - n;
        f.relx = (float) pix + .5f - p.x; f.rely = (float) piy + .5f - p.y;
        f.ax = pix - rp.crop_x; f.ay = piy - rp.crop_y;
    }
    return f;
}
// Every term is a float32 product converted to double; the box filter adds the value itself (value * 1.f is the same float)
DTOF_D double term(float v, float w, bool box) { return (double) (box ? v : v * w); }
DTOF_D void add_f64(double *p, double v) { if (v != 0.0) atomicAdd(p, v); }   // x + (+-0) = x, and the film starts at +0: skipping a zero changes no bit

// The wide walk, for a lane that has a sample: cell(pixel, w) for every cell of the lane's footprint inside the film, pixel = y * crop_w + x, w = wx * wy
template <typename Cell> DTOF_D void walk_wide(const RenderParams &rp, const Footprint &f, Cell &&cell) {
#pragma unroll 1
    for (int ys = 0; ys < f.cnt; ++ys) {
        const float wy = filter_weight(rp, f.rely + (float) ys);
#pragma unroll 1
        for (int xs = 0; xs < f.cnt; ++xs) {
            const float w = filter_weight(rp, f.relx + (float) xs) * wy;
            const int x = f.ax + xs, y = f.ay + ys;
            if ((unsigned) x < (unsigned) rp.crop_w && (unsigned) y < (unsigned) rp.crop_h) cell((size_t) y * rp.crop_w + x, w);
        }
    }
}

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

// What the run walk of a lane needs, computed once per lane (k_aov walks once per plane): the lane's place in its run, whether it is the lane that writes the run's
// sums, and the column and row weights of its own sample (0 beyond cnt and for the box filter)
struct RunCells { uint32_t dist, steps; bool writes; float wx0, wx1, wx2, wx3, wx4, wy0, wy1, wy2, wy3, wy4; };
DTOF_D RunCells run_cells_of(const RenderParams &rp, const Footprint &f, bool valid) {
    static_assert(kRunCells == 5, "five column and five row weights are kept in registers");
    const Runs runs = find_runs(f.ax, f.ay, valid);
    RunCells c;
    c.dist = runs.dist; c.steps = runs.steps; c.writes = valid && runs.last;
#define DTOF_W(rel, k) (k < f.cnt && !f.box ? filter_weight(rp, rel + (float) k) : 0.f)
    c.wx0 = DTOF_W(f.relx, 0); c.wx1 = DTOF_W(f.relx, 1); c.wx2 = DTOF_W(f.relx, 2); c.wx3 = DTOF_W(f.relx, 3); c.wx4 = DTOF_W(f.relx, 4);
    c.wy0 = DTOF_W(f.rely, 0); c.wy1 = DTOF_W(f.rely, 1); c.wy2 = DTOF_W(f.rely, 2); c.wy3 = DTOF_W(f.rely, 3); c.wy4 = DTOF_W(f.rely, 4);
#undef DTOF_W
    return c;
}
// The run walk, for EVERY lane of the wave (the caller's run_sum is wave-wide): cell(w, write, pixel) for every cell of the footprint.  w is the lane's own weight
// wx * wy (0 for the box filter, whose term() does not read it); write: this lane adds the run's sums to the film -- the run's last lane, the cell inside the film,
// the same cell for every lane of the run; pixel = y * crop_w + x, 0 for a lane that does not write.  The loops stay rolled (25 cells times a kernel's sums unrolled
// would be far beyond the instruction cache): their counters are scalars, sel() turns into selects on them.
template <typename Cell> DTOF_D void walk_runs(const RenderParams &rp, const Footprint &f, const RunCells &c, Cell &&cell) {
#pragma unroll 1
    for (int ys = 0; ys < f.cnt; ++ys) {
        const float wys = sel(ys, c.wy0, c.wy1, c.wy2, c.wy3, c.wy4);
        const int y = f.ay + ys;
        const bool row = c.writes && (unsigned) y < (unsigned) rp.crop_h;
        const size_t row_first = (size_t) (row ? y : 0) * rp.crop_w;
#pragma unroll 1
        for (int xs = 0; xs < f.cnt; ++xs) {
            const int x = f.ax + xs;
            const bool write = row && (unsigned) x < (unsigned) rp.crop_w;
            cell(sel(xs, c.wx0, c.wx1, c.wx2, c.wx3, c.wx4) * wys, write, write ? row_first + (size_t) x : 0);
        }
    }
}

}  // namespace dtof
