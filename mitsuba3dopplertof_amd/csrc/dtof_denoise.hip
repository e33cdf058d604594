// dtof_denoise.hip -- joint variance-guided a-trous denoiser behind the films: the edge-avoiding wavelet filter of Dammertz et al. 2010 with the
// variance-normalised luminance term of SVGF's spatial pass, over up to four colour planes that share ONE set of weights (the four films of a velocity map, so the
// heterodyne / homodyne ratio of a pixel stays a ratio of identically weighted neighbourhoods).  tests/denoise_ref.py is the definition in numpy; every operation
// below is the double operation it names, in its order, and the file is compiled with -ffp-contract=off like every kernel here.
//   k_denoise_pack   : inputs -> one guide record per pixel (normal, position as the float32 they came as, validity) and double planes (colour, variance, luminance)
//   k_denoise_level  : one level, step s = 2^l, from one set of planes into the other; the last level writes the caller's outputs itself
// A level never reads what it writes.  No atomics, no scratch (profiles/denoise_resource_usage.txt).
#include "dtof_denoise.h"
#include <cfloat>

namespace dtof {

namespace {

constexpr int kPackBlock = 256;
constexpr int kTileX = 64;              // pixels of a tile row, contiguous in x: one wave reads one row
constexpr int kTileEntries = 1152;      // LDS entries of a tile and its halo: (64 + 4 * 16) x (4 + 4) = 1024 up to step 16, (64 + 4 * 32) x (2 + 4) = 1152 at step 32

// normal and position stay the float32 they came as (the conversion to double is exact wherever it happens); valid: every word of the pixel is finite
struct DenoiseGuide { float n[3]; float x[3]; uint32_t valid; uint32_t pad; };
static_assert(sizeof(DenoiseGuide) == 32, "two 16-byte loads per record");

struct PackArgs {
    const float *colour, *normal, *position; const double *variance;
    DenoiseGuide *guides; double *col, *var, *lum;
    int64_t n; int32_t n_planes;
};

struct LevelArgs {
    const DenoiseGuide *guides; const double *col_in, *var_in, *lum_in;
    double *col_out, *var_out, *lum_out;       // var_out / lum_out may be null (the last level: no luminance, the variance only if asked for)
    int64_t pix_stride, chan_stride;           // of col_out: 1, n for the working planes; 3, 1 for the caller's [K][H][W][3]
    int64_t n; int32_t width, height, step, tiles_y;
    double sigma_normal2, sigma_position2, sigma_luminance;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }     // false for a NaN
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= DBL_MAX; }
__device__ __forceinline__ double luminance(double r, double g, double b) { return (0.2126 * r + 0.7152 * g) + 0.0722 * b; }
__device__ __forceinline__ double b3(int i) { return i == 0 ? 0.375 : (i == 1 || i == -1) ? 0.25 : 0.0625; }   // (1/16, 1/4, 3/8, 1/4, 1/16)

__global__ __launch_bounds__(kPackBlock) void k_denoise_pack(PackArgs a) {
    const int64_t p = (int64_t) blockIdx.x * kPackBlock + threadIdx.x;
    if (p >= a.n) return;
    DenoiseGuide g;
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        g.n[c] = a.normal ? a.normal[p * 3 + c] : 0.f;
        g.x[c] = a.position ? a.position[p * 3 + c] : 0.f;
        ok = ok && finite_f(g.n[c]) && finite_f(g.x[c]);
    }
    for (int32_t k = 0; k < a.n_planes; ++k) {
        const float *cf = a.colour + ((int64_t) k * a.n + p) * 3;
        const double r = (double) cf[0], gr = (double) cf[1], b = (double) cf[2];
        ok = ok && finite_d(r) && finite_d(gr) && finite_d(b);
        a.col[((int64_t) k * 3 + 0) * a.n + p] = r; a.col[((int64_t) k * 3 + 1) * a.n + p] = gr; a.col[((int64_t) k * 3 + 2) * a.n + p] = b;
        if (a.variance) {
            const double v = a.variance[(int64_t) k * a.n + p];
            ok = ok && finite_d(v);
            a.var[(int64_t) k * a.n + p] = v;
            a.lum[(int64_t) k * a.n + p] = luminance(r, gr, b);
        }
    }
    g.valid = ok ? 1u : 0u; g.pad = 0u;
    a.guides[p] = g;
}

// One level.  TILED: a block of 64 x blockDim.y lanes owns 64 pixels of blockDim.y rows of the level's LATTICE (rows y0 + m * step), stages what the weights need
// of those pixels and their halo -- 2 * step columns each side, two lattice rows above and below -- in LDS with loads contiguous in x, and takes every tap's weight
// inputs from there; entries outside the image are staged as invalid, so one test skips both.  Columns are unit-stride arrays (one per word), so the wave's 64
// neighbouring entries of a ds_read_b64 fall into 64 different bank pairs.  Colours and variances of the taps come from memory, contiguous across the wave.
// !TILED (only in a build with -DDTOF_DENOISE_NAIVE): 64 x 4 pixels per block, every tap's record read from memory.
template <int K, bool HN, bool HX, bool HV, bool TILED>
__global__ __launch_bounds__(256) void k_denoise_level(LevelArgs a) {
    __shared__ float s_n[TILED && HN ? 3 * kTileEntries : 1];
    __shared__ float s_x[TILED && HX ? 3 * kTileEntries : 1];
    __shared__ double s_l[TILED && HV ? K * kTileEntries : 1];
    __shared__ uint32_t s_valid[TILED ? kTileEntries : 1];

    const int32_t s = a.step, W = a.width, H = a.height;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int32_t x = (int32_t) blockIdx.x * kTileX + tx;
    int32_t y, lw = 0, lc = 0;
    if constexpr (TILED) {
        const int32_t rows = (int32_t) blockDim.y;
        const int32_t r = (int32_t) blockIdx.y / a.tiles_y, m0 = ((int32_t) blockIdx.y % a.tiles_y) * rows;    // residue of the lattice, first lattice row of the tile
        lw = kTileX + 4 * s;
        const int32_t entries = lw * (rows + 4), x_lo = (int32_t) blockIdx.x * kTileX - 2 * s;
        for (int32_t e = ty * kTileX + tx; e < entries; e += kTileX * rows) {
            const int32_t ly = e / lw, lx = e - ly * lw;
            const int32_t qx = x_lo + lx, m = m0 - 2 + ly;
            const int64_t qy = (int64_t) r + (int64_t) m * s;
            const bool inside = qx >= 0 && qx < W && m >= 0 && qy < H;
            const int64_t q = inside ? qy * W + qx : 0;
            const DenoiseGuide g = a.guides[q];
            s_valid[e] = inside ? g.valid : 0u;
            if constexpr (HN) { s_n[e] = g.n[0]; s_n[kTileEntries + e] = g.n[1]; s_n[2 * kTileEntries + e] = g.n[2]; }
            if constexpr (HX) { s_x[e] = g.x[0]; s_x[kTileEntries + e] = g.x[1]; s_x[2 * kTileEntries + e] = g.x[2]; }
            if constexpr (HV) {
#pragma unroll
                for (int k = 0; k < K; ++k) s_l[k * kTileEntries + e] = a.lum_in[(int64_t) k * a.n + q];
            }
        }
        __syncthreads();
        y = r + (m0 + ty) * s;
        lc = (ty + 2) * lw + tx + 2 * s;
    } else {
        y = (int32_t) blockIdx.y * 4 + ty;
    }
    if (x >= W || y >= H) return;
    const int64_t p = (int64_t) y * W + x;

    bool valid_p;
    double np[3] = { 0, 0, 0 }, xp[3] = { 0, 0, 0 }, lp[K], den[K];
    if constexpr (TILED) {
        valid_p = s_valid[lc] != 0u;
        if constexpr (HN) for (int c = 0; c < 3; ++c) np[c] = (double) s_n[c * kTileEntries + lc];
        if constexpr (HX) for (int c = 0; c < 3; ++c) xp[c] = (double) s_x[c * kTileEntries + lc];
    } else {
        const DenoiseGuide g = a.guides[p];
        valid_p = g.valid != 0u;
        for (int c = 0; c < 3; ++c) { np[c] = (double) g.n[c]; xp[c] = (double) g.x[c]; }
    }
    if (!valid_p) {   // an invalid centre passes through unchanged, at every level
#pragma unroll
        for (int k = 0; k < K; ++k) {
            for (int c = 0; c < 3; ++c) a.col_out[(int64_t) k * 3 * a.n + p * a.pix_stride + c * a.chan_stride] = a.col_in[((int64_t) k * 3 + c) * a.n + p];
            if constexpr (HV) {
                if (a.var_out) a.var_out[(int64_t) k * a.n + p] = a.var_in[(int64_t) k * a.n + p];
                if (a.lum_out) a.lum_out[(int64_t) k * a.n + p] = a.lum_in[(int64_t) k * a.n + p];
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        lp[k] = 0.0; den[k] = 0.0;
        if constexpr (HV) {
            if constexpr (TILED) lp[k] = s_l[k * kTileEntries + lc]; else lp[k] = a.lum_in[(int64_t) k * a.n + p];
            const double v = a.var_in[(int64_t) k * a.n + p];
            den[k] = a.sigma_luminance * sqrt(v > 0.0 ? v : 0.0);     // the variance at the CENTRE
        }
    }

    double sum_w = 0.0, acc[K][3], acc_v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { acc[k][0] = acc[k][1] = acc[k][2] = 0.0; acc_v[k] = 0.0; }
    // the tap loops stay loops: unrolled, the 25 taps' loads are hoisted together and the K = 4 kernels run out of registers
#pragma unroll 1
    for (int j = -2; j <= 2; ++j) {
        const int64_t qy = (int64_t) y + (int64_t) j * s;
        if (qy < 0 || qy >= H) continue;           // (the staged entry says so too; this keeps q in range for the colour loads)
#pragma unroll 1
        for (int i = -2; i <= 2; ++i) {
            const int64_t qx = (int64_t) x + (int64_t) i * s;
            if (qx < 0 || qx >= W) continue;
            const int64_t q = qy * W + qx;
            double nq[3] = { 0, 0, 0 }, xq[3] = { 0, 0, 0 }, lq[K];
            if constexpr (TILED) {
                const int32_t lt = lc + j * lw + i * s;
                if (s_valid[lt] == 0u) continue;
                if constexpr (HN) for (int c = 0; c < 3; ++c) nq[c] = (double) s_n[c * kTileEntries + lt];
                if constexpr (HX) for (int c = 0; c < 3; ++c) xq[c] = (double) s_x[c * kTileEntries + lt];
#pragma unroll
                for (int k = 0; k < K; ++k) { if constexpr (HV) lq[k] = s_l[k * kTileEntries + lt]; else lq[k] = 0.0; }
            } else {
                const DenoiseGuide g = a.guides[q];
                if (g.valid == 0u) continue;
                for (int c = 0; c < 3; ++c) { nq[c] = (double) g.n[c]; xq[c] = (double) g.x[c]; }
#pragma unroll
                for (int k = 0; k < K; ++k) { if constexpr (HV) lq[k] = a.lum_in[(int64_t) k * a.n + q]; else lq[k] = 0.0; }
            }
            double dn = 0.0, dx = 0.0, dl = 0.0;
            if constexpr (HN) {
                const double d0 = np[0] - nq[0], d1 = np[1] - nq[1], d2 = np[2] - nq[2];
                dn = ((d0 * d0 + d1 * d1) + d2 * d2) / a.sigma_normal2;
            }
            if constexpr (HX) {
                const double d0 = xp[0] - xq[0], d1 = xp[1] - xq[1], d2 = xp[2] - xq[2];
                dx = ((d0 * d0 + d1 * d1) + d2 * d2) / a.sigma_position2;
            }
            if constexpr (HV) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    // no epsilon: under a zero (or negative) variance only an equal luminance passes, so the term is exactly scale-invariant
                    const double d = den[k] > 0.0 ? fabs(lp[k] - lq[k]) / den[k] : (lp[k] == lq[k] ? 0.0 : (double) INFINITY);
                    dl = d > dl ? d : dl;
                }
            }
            const double w = (b3(i) * b3(j)) * exp(-((dn + dx) + dl));    // ONE weight per tap, for every plane and for the variance
            sum_w = sum_w + w;
            const double w2 = w * w;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                for (int c = 0; c < 3; ++c) acc[k][c] = acc[k][c] + w * a.col_in[((int64_t) k * 3 + c) * a.n + q];
                if constexpr (HV) acc_v[k] = acc_v[k] + w2 * a.var_in[(int64_t) k * a.n + q];
            }
        }
    }
    // the centre tap always takes part: sum_w >= 9 / 64
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double r = acc[k][0] / sum_w, g = acc[k][1] / sum_w, b = acc[k][2] / sum_w;
        double *o = a.col_out + (int64_t) k * 3 * a.n + p * a.pix_stride;
        o[0] = r; o[a.chan_stride] = g; o[2 * a.chan_stride] = b;
        if constexpr (HV) {
            if (a.var_out) a.var_out[(int64_t) k * a.n + p] = acc_v[k] / (sum_w * sum_w);
            if (a.lum_out) a.lum_out[(int64_t) k * a.n + p] = luminance(r, g, b);
        }
    }
}

template <int K, bool TILED> void launch_level_k(const DenoiseArgs &d, const LevelArgs &a, dim3 grid, dim3 block, hipStream_t s) {
    const int mask = (d.has_normal ? 1 : 0) | (d.has_position ? 2 : 0) | (d.has_variance ? 4 : 0);
#define DTOF_DENOISE_CASE(M) case M: hipLaunchKernelGGL((k_denoise_level<K, ((M) & 1) != 0, ((M) & 2) != 0, ((M) & 4) != 0, TILED>), grid, block, 0, s, a); break;
    switch (mask) {
        DTOF_DENOISE_CASE(0) DTOF_DENOISE_CASE(1) DTOF_DENOISE_CASE(2) DTOF_DENOISE_CASE(3)
        DTOF_DENOISE_CASE(4) DTOF_DENOISE_CASE(5) DTOF_DENOISE_CASE(6) DTOF_DENOISE_CASE(7)
    }
#undef DTOF_DENOISE_CASE
}
template <bool TILED> void launch_level(const DenoiseArgs &d, const LevelArgs &a, dim3 grid, dim3 block, hipStream_t s) {
    switch (d.n_planes) {
        case 1: launch_level_k<1, TILED>(d, a, grid, block, s); break;
        case 2: launch_level_k<2, TILED>(d, a, grid, block, s); break;
        case 3: launch_level_k<3, TILED>(d, a, grid, block, s); break;
        case 4: launch_level_k<4, TILED>(d, a, grid, block, s); break;
    }
}

}  // namespace

void launch_denoise(const DenoiseArgs &d, const float *colour, const double *variance, const float *normal, const float *position, double *out_colour,
                    double *out_variance, double *scratch, hipStream_t s) {
    const int64_t n = (int64_t) d.width * d.height;
    const int64_t K = d.n_planes;
    const bool hv = d.has_variance != 0;
    // scratch: the guide records, then two sets of planes: colour [3 K][n], and with a variance: variance [K][n], luminance [K][n]
    DenoiseGuide *guides = (DenoiseGuide *) scratch;
    double *set[2]; set[0] = scratch + 4 * n; set[1] = set[0] + K * (hv ? 5 : 3) * n;
    auto col = [&](int i) { return set[i]; };
    auto var = [&](int i) { return hv ? set[i] + 3 * K * n : nullptr; };
    auto lum = [&](int i) { return hv ? set[i] + 4 * K * n : nullptr; };

    PackArgs pa;
    pa.colour = colour; pa.normal = normal; pa.position = position; pa.variance = variance;
    pa.guides = guides; pa.col = col(0); pa.var = var(0); pa.lum = lum(0); pa.n = n; pa.n_planes = d.n_planes;
    hipLaunchKernelGGL(k_denoise_pack, dim3((uint32_t) ((n + kPackBlock - 1) / kPackBlock)), dim3(kPackBlock), 0, s, pa);

    for (int32_t l = 0; l < d.levels; ++l) {
        const int in = l & 1, out = in ^ 1;
        const bool last = l == d.levels - 1;
        LevelArgs a;
        a.guides = guides; a.col_in = col(in); a.var_in = var(in); a.lum_in = lum(in);
        a.col_out = last ? out_colour : col(out); a.var_out = last ? out_variance : var(out); a.lum_out = last ? nullptr : lum(out);
        a.pix_stride = last ? 3 : 1; a.chan_stride = last ? 1 : n;
        a.n = n; a.width = d.width; a.height = d.height; a.step = 1 << l;
        a.sigma_normal2 = d.sigma_normal2; a.sigma_position2 = d.sigma_position2; a.sigma_luminance = d.sigma_luminance;
        const uint32_t tiles_x = (uint32_t) ((d.width + kTileX - 1) / kTileX);
#ifdef DTOF_DENOISE_NAIVE      // the A/B build: one lane per pixel
        a.tiles_y = 0;
        launch_level<false>(d, a, dim3(tiles_x, (uint32_t) ((d.height + 3) / 4)), dim3(kTileX, 4), s);
#else
        // rows of a tile: 4 up to step 16, 2 at step 32, so that the tile and its halo stay within kTileEntries; a lattice has min(step, height) residues of
        // at most ceil(height / step) rows each
        const int32_t rows = a.step <= 16 ? 4 : 2;
        const int32_t lattice_rows = (d.height + a.step - 1) / a.step, residues = a.step < d.height ? a.step : d.height;
        a.tiles_y = (lattice_rows + rows - 1) / rows;
        launch_level<true>(d, a, dim3(tiles_x, (uint32_t) (residues * a.tiles_y)), dim3(kTileX, rows), s);
#endif
    }
}

}  // namespace dtof
