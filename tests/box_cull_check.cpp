// Host check of the slab test of the TLAS / BLAS walks (mitsuba3dopplertof_amd/csrc/dtof_box_cull.h: slab_ray, box_hit -- the functions the kernels call, compiled for
// the host) against its contract (tests/test_box_cull.py builds and runs it, three times: with the reciprocal as 1.f / x and moved one ulp either way):
//
//     whenever the ray passes through the UNPADDED box within [0, maxt], box_hit on the padded box returns true.
//
// Input: a file of records of 14 floats -- o[3], d[3], time, maxt, the box's lo[3], hi[3] -- the rays of families B, F and E of tests/tree_sweep.py with the bounds of the
// meshes and triangles they hit, and the issue's own cases.  Each box is padded as the host pads it (scene_build.cpp: Box::pad) and tested as it is (float nodes) and
// rounded outwards to half floats (half_toward: DNode16).  "Passes through" is the slab test in long double, where a comparison BETWEEN TWO AXES, with 0 or with maxt has
// to hold with a margin of 2^-40 of its operands (one axis' near and far plane of a flat box coincide: that comparison is an identity).
// The PARENT columns restate the test as it was before the contract held (exact zeros nudged only, tn <= tf): they count what the check would have found there.
// usage: box_cull_check <records> ; prints "key value" lines
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cfloat>
#include <vector>
#include <algorithm>
#include "dtof_box_cull.h"
#include "dtof_half.h"

using dtof::SlabRay;

static float half_to_float(uint16_t h) {
    const uint32_t s = h >> 15, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    const float mag = e == 0 ? ldexpf((float) m, -24) : ldexpf((float) (m | 0x400u), (int) e - 25);
    return s ? -mag : mag;
}
static void pad(float *lo, float *hi) {   // Box::pad
    for (int i = 0; i < 3; ++i) {
        const float e = std::max(std::max(std::fabs(lo[i]), std::fabs(hi[i])), hi[i] - lo[i]) * 1e-5f + 1e-6f;
        lo[i] -= e; hi[i] += e;
    }
}
static bool parent_box_hit(const float *bmin, const float *bmax, const float *o, const float *d, float tbest) {
    float id[3], noid[3], t0[3], t1[3];
    for (int k = 0; k < 3; ++k) {
        id[k] = dtof::slab_rcp(d[k] == 0.f ? 1e-30f : d[k]); noid[k] = -(o[k] * id[k]);
        t0[k] = fmaf(bmin[k], id[k], noid[k]); t1[k] = fmaf(bmax[k], id[k], noid[k]);
    }
    const float tn = fmaxf(fmaxf(fminf(t0[0], t1[0]), fminf(t0[1], t1[1])), fmaxf(fminf(t0[2], t1[2]), 0.f));
    const float tf = fminf(fminf(fmaxf(t0[0], t1[0]), fmaxf(t0[1], t1[1])), fminf(fmaxf(t0[2], t1[2]), tbest));
    return tn <= tf;
}
// the ray meets the box [lo, hi] within [0, maxt], every comparison between different quantities with a margin
static bool passes_through(const float *o, const float *d, float maxt, const float *lo, const float *hi) {
    long double nr[3], fr[3];
    for (int k = 0; k < 3; ++k) {
        if (d[k] == 0.f) {
            const long double m = ldexpl(std::max(fabsl((long double) o[k]), std::max(fabsl((long double) lo[k]), fabsl((long double) hi[k]))), -40);
            const bool inside = ((long double) lo[k] + m <= (long double) o[k] && (long double) o[k] <= (long double) hi[k] - m) || (lo[k] == hi[k] && o[k] == lo[k]);
            if (!inside) return false;
            nr[k] = -INFINITY; fr[k] = INFINITY;
            continue;
        }
        const long double a = ((long double) lo[k] - (long double) o[k]) / (long double) d[k], b = ((long double) hi[k] - (long double) o[k]) / (long double) d[k];
        nr[k] = std::min(a, b); fr[k] = std::max(a, b);
    }
    auto below = [](long double a, long double b) {   // a <= b with a margin of 2^-40 of the operands
        if (std::isinf(a) || std::isinf(b)) return a <= b;
        return a + ldexpl(std::max(fabsl(a), fabsl(b)), -40) <= b;
    };
    for (int i = 0; i < 3; ++i) {
        if (!below(0.L, fr[i]) || !below(nr[i], (long double) maxt)) return false;
        for (int j = 0; j < 3; ++j) if (i != j && !below(nr[i], fr[j])) return false;
        if (!(nr[i] <= fr[i])) return false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> rec;
    float buf[14];
    while (fread(buf, sizeof(float), 14, f) == 14) rec.insert(rec.end(), buf, buf + 14);
    fclose(f);
    unsigned long long n = 0, through = 0, culled[2] = { 0, 0 }, parent_culled[2] = { 0, 0 }, hit_anyway[2] = { 0, 0 };
    for (size_t r = 0; r + 14 <= rec.size(); r += 14, ++n) {
        const float *o = &rec[r], *d = &rec[r + 3], maxt = rec[r + 7], *lo = &rec[r + 8], *hi = &rec[r + 11];
        const bool thru = passes_through(o, d, maxt, lo, hi);
        through += thru;
        float plo[3] = { lo[0], lo[1], lo[2] }, phi[3] = { hi[0], hi[1], hi[2] };
        pad(plo, phi);
        float hlo[3], hhi[3];
        for (int k = 0; k < 3; ++k) { hlo[k] = half_to_float(dtof::half_toward(plo[k], false)); hhi[k] = half_to_float(dtof::half_toward(phi[k], true)); }
        const SlabRay sr = dtof::slab_ray(o[0], o[1], o[2], d[0], d[1], d[2]);
        for (int form = 0; form < 2; ++form) {
            const float *bl = form ? hlo : plo, *bh = form ? hhi : phi;
            float tn;
            const bool hit = dtof::box_hit(bl, bh, sr, maxt, tn), parent = parent_box_hit(bl, bh, o, d, maxt);
            if (thru && !hit) {
                if (culled[form] < 5) fprintf(stderr, "CULLED (%s) o %a %a %a d %a %a %a maxt %a box %a %a %a .. %a %a %a\n", form ? "half" : "float", o[0], o[1], o[2], d[0], d[1], d[2], maxt,
                                              lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
                ++culled[form];
            }
            parent_culled[form] += thru && !parent;
            hit_anyway[form] += !thru && hit;
        }
    }
    printf("records %llu\nthrough %llu\nculled_float %llu\nculled_half %llu\nparent_culled_float %llu\nparent_culled_half %llu\nkept_beyond_float %llu\nkept_beyond_half %llu\n",
           n, through, culled[0], culled[1], parent_culled[0], parent_culled[1], hit_anyway[0], hit_anyway[1]);
    return 0;
}
