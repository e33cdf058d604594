// dtof_adaptive.hip -- the selection step of adaptive sampling: which pixels does the next pass render?  From the moment sums of every pixel (dtof_moments.h) and its
// nominal sample count, a per-pixel error metric in double (dtof_adaptive.h has the definition, tests/adaptive_ref.py the same text in numpy), the flag metric > tol, and
// the ASCENDING list of the flagged pixels, which is what makes a run reproducible.
//   flags    one thread per pixel; the wave's ballot goes to memory, the block's popcount to the first scan level
//   scan     exclusive prefix sums of 256 counts per block, the blocks' totals being the next level; levels until one block takes a level (its total is the list's
//            length), then the prefixes are added back down level by level (nothing to add for a film of one level).  Every launch reads what an earlier launch finished: no block waits on another block inside a kernel.
//   scatter  a flagged pixel's slot is its block's prefix + the popcounts of the waves before its own + the popcount of the lanes before it in its wave's ballot
// Compiled with -ffp-contract=off like every kernel here; double division and square root are correctly rounded.
#include "dtof_adaptive.h"
#include "dtof_develop.h"
#include <vector>

namespace dtof {

namespace {
constexpr uint32_t kWave = 64, kWavesPerBlock = kAdaptiveBlock / kWave;
static_assert(kAdaptiveBlock % kWave == 0, "a block is whole waves");

// numpy's maximum: the first operand if it is the larger one or a NaN, else the second (so a NaN of either side comes through)
__device__ __forceinline__ double np_max(double x, double y) { return (x >= y || x != x) ? x : y; }
__device__ __forceinline__ bool finite_(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

struct PixelVerdict { double metric; bool selected; };

__device__ __forceinline__ PixelVerdict judge(const AdaptiveArgs &a, const double *S, int64_t ps, uint32_t cnt) {
    const double Wd = develop_weight(S[0]), n = (double) cnt;
    PixelVerdict v;
    if (a.mode == kAdaptiveImage) {
        double metric = 0.0;
        for (int k = 0; k < a.n_variants; ++k) {
            const double mean = S[(1 + 6 * k + 1) * ps] / Wd, m2 = S[(1 + 6 * k + 4) * ps] / Wd;
            const double var = m2 - mean * mean;
            const double se = sqrt(np_max(var, 0.0) / n);
            const double q = se / np_max(fabs(mean), a.floor);
            metric = k == 0 ? q : np_max(metric, q);
        }
        if (cnt == 0) metric = 0.0;
        v.metric = metric; v.selected = cnt != 0 && metric > a.tol;
        return v;
    }
    double best = __builtin_nan(""); bool any = false, selected = false;
    for (int p = 0; p < a.n_pairs; ++p) {
        const int h = a.hom[p], t = a.het[p];
        const double av = S[(1 + 6 * h + 1) * ps] / Wd, m2h = S[(1 + 6 * h + 4) * ps] / Wd, var_h = m2h - av * av;
        const double bv = S[(1 + 6 * t + 1) * ps] / Wd, m2t = S[(1 + 6 * t + 4) * ps] / Wd, var_t = m2t - bv * bv;
        const double cov = S[a.cross[p] * ps] / Wd - av * bv;
        const double r = bv / av;
        const double var_r = ((var_t - (2.0 * r) * cov) + (r * r) * var_h) / ((av * av) * n);
        const double slope = ((0.5 * 3e8) / (a.w_g_mhz * 1e6)) / (a.exposure_time * ((r - 1.0) * (r - 1.0)));
        const double se = sqrt(np_max(var_r, 0.0)) * slope;
        const bool valid = av != 0.0 && r > -1.0 && r < 0.999;
        if (valid && finite_(se)) {
            selected |= se > a.tol;
            if (!any || se > best) best = se;
            any = true;
        } else {
            selected |= var_h > 0.0 || var_t > 0.0;
        }
    }
    v.metric = best; v.selected = selected;
    return v;
}

// ballots[wave] and block_counts[block]; the wave index is global (i / 64)
__global__ __launch_bounds__(kAdaptiveBlock) void k_adaptive_flags(AdaptiveArgs a, const double *S, uint32_t n, const uint32_t *count, double *metric,
                                                                   unsigned long long *ballots, uint32_t *block_counts) {
    __shared__ uint32_t wave_count[kWavesPerBlock];
    const uint32_t i = blockIdx.x * kAdaptiveBlock + threadIdx.x;
    bool sel = false;
    if (i < n) {
        const PixelVerdict v = judge(a, S + (int64_t) i * a.pixel_stride, a.plane_stride, count[i]);
        if (metric) metric[i] = v.metric;
        sel = v.selected;
    }
    const unsigned long long mask = __ballot(sel);
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) {
        if (blockIdx.x * kAdaptiveBlock + wave * kWave < n) ballots[(size_t) blockIdx.x * kWavesPerBlock + wave] = mask;
        wave_count[wave] = (uint32_t) __popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < kWavesPerBlock; ++w) c += wave_count[w];
        block_counts[blockIdx.x] = c;
    }
}

// exclusive prefix sums of in[block * 256 .. + 256) (beyond m: 0) into out; the block's total to totals[block]
__global__ __launch_bounds__(kAdaptiveBlock) void k_adaptive_scan(const uint32_t *in, uint32_t *out, uint32_t *totals, uint32_t m) {
    __shared__ uint32_t buf[kAdaptiveBlock];
    const uint32_t i = blockIdx.x * kAdaptiveBlock + threadIdx.x;
    const uint32_t own = i < m ? in[i] : 0u;
    buf[threadIdx.x] = own;
    __syncthreads();
    for (uint32_t d = 1; d < kAdaptiveBlock; d <<= 1) {   // Hillis-Steele: inclusive sums
        const uint32_t add = threadIdx.x >= d ? buf[threadIdx.x - d] : 0u;
        __syncthreads();
        buf[threadIdx.x] += add;
        __syncthreads();
    }
    if (i < m) out[i] = buf[threadIdx.x] - own;
    if (threadIdx.x == kAdaptiveBlock - 1) totals[blockIdx.x] = buf[threadIdx.x];
}
// a level's prefixes become global: out[i] += upper[i / 256]
__global__ __launch_bounds__(kAdaptiveBlock) void k_adaptive_add(uint32_t *out, const uint32_t *upper, uint32_t m) {
    const uint32_t i = blockIdx.x * kAdaptiveBlock + threadIdx.x;
    if (i < m) out[i] += upper[blockIdx.x];
}

__global__ __launch_bounds__(kAdaptiveBlock) void k_adaptive_scatter(uint32_t n, uint32_t spp, const unsigned long long *ballots, const uint32_t *block_prefix,
                                                                     uint32_t *count, uint32_t *out_pixels) {
    const uint32_t i = blockIdx.x * kAdaptiveBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const unsigned long long *b = ballots + (size_t) blockIdx.x * kWavesPerBlock;
    const unsigned long long mine = b[wave];
    if (!((mine >> lane) & 1ull)) return;
    uint32_t slot = block_prefix[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) slot += (uint32_t) __popcll(b[w]);   // the waves before this one hold pixels below n: their ballots were written
    slot += (uint32_t) __popcll(mine & ((1ull << lane) - 1ull));
    out_pixels[slot] = i;   // slot < the number of flagged pixels <= n
    count[i] += spp;
}

uint32_t blocks_of(uint32_t m) { return (m + kAdaptiveBlock - 1) / kAdaptiveBlock; }
// the scan levels of n pixels: level 0 holds the flag kernel's block counts, level l + 1 the totals of level l's scan blocks; the last level is the one ONE scan block
// takes (at most 256 counts), and that block's total is the list's length -- one level for films up to 65 536 pixels, two up to 2^24
std::vector<uint32_t> level_sizes(uint32_t n) {
    std::vector<uint32_t> m { blocks_of(n) };
    while (blocks_of(m.back()) > 1) m.push_back(blocks_of(m.back()));
    return m;
}
}  // namespace

size_t adaptive_scratch_words(uint32_t n) {
    if (n == 0) return 0;
    size_t words = 2 * (size_t) blocks_of(n) * kWavesPerBlock;   // the ballots, 64 bits each
    for (uint32_t m : level_sizes(n)) words += 2 * (size_t) m;    // counts and prefixes of every level
    return words + 2;                                             // the total of the last level (8-byte aligned start of the counts)
}

void launch_adaptive_metric(const AdaptiveArgs &a, const double *S, uint32_t n, const uint32_t *count, double *metric, uint32_t *scratch, hipStream_t s) {
    if (n == 0) return;
    const uint32_t blocks = blocks_of(n);
    hipLaunchKernelGGL(k_adaptive_flags, dim3(blocks), dim3(kAdaptiveBlock), 0, s, a, S, n, count, metric, (unsigned long long *) scratch,
                       scratch + 2 * (size_t) blocks * kWavesPerBlock);
}

void launch_adaptive_select(const AdaptiveArgs &a, const double *S, uint32_t n, uint32_t *count, uint32_t *out_pixels, uint32_t *out_n, double *metric,
                            uint32_t *scratch, hipStream_t s) {
    if (n == 0) { (void) hipMemsetAsync(out_n, 0, sizeof(uint32_t), s); return; }
    const std::vector<uint32_t> m = level_sizes(n);
    unsigned long long *ballots = (unsigned long long *) scratch;
    uint32_t *w = scratch + 2 * (size_t) m[0] * kWavesPerBlock;
    std::vector<uint32_t *> counts(m.size()), prefix(m.size());
    for (size_t l = 0; l < m.size(); ++l) { counts[l] = w; w += m[l]; prefix[l] = w; w += m[l]; }
    hipLaunchKernelGGL(k_adaptive_flags, dim3(m[0]), dim3(kAdaptiveBlock), 0, s, a, S, n, count, metric, ballots, counts[0]);
    // level l's scan: blocks_of(m[l]) blocks, whose totals are level l + 1's counts (the last level is one block: its total is the list's length)
    for (size_t l = 0; l < m.size(); ++l)
        hipLaunchKernelGGL(k_adaptive_scan, dim3(blocks_of(m[l])), dim3(kAdaptiveBlock), 0, s, counts[l], prefix[l], l + 1 < m.size() ? counts[l + 1] : out_n, m[l]);
    for (size_t l = m.size() - 1; l-- > 0;)
        hipLaunchKernelGGL(k_adaptive_add, dim3(blocks_of(m[l])), dim3(kAdaptiveBlock), 0, s, prefix[l], prefix[l + 1], m[l]);
    hipLaunchKernelGGL(k_adaptive_scatter, dim3(m[0]), dim3(kAdaptiveBlock), 0, s, n, a.spp, ballots, prefix[0], count, out_pixels);
}

}  // namespace dtof
