// Host check of trace_flat's certain-miss test (mitsuba3dopplertof_amd/csrc/dtof_flat_cull.h) against the rectangle test it skips (tests/test_flat_cull.py
// builds and runs it).  For every input (zx, zy, maxt, and the xy rows' results) it evaluates the kernel's arithmetic
//     t = -zx / zy,  u = fma(ldx, t, lox),  v = fma(ldy, t, loy),  hit = t >= 0 && t <= maxt && |u| <= 1 && |v| <= 1
// and counts the inputs the cull settles although `t >= 0 && t <= maxt` holds (whatever u and v are) or although `hit` holds.  Both must stay 0.
// usage: flat_cull_check <inputs> <seed>    prints "key value" lines
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cfloat>
#include "dtof_flat_cull.h"

using dtof::flat_certain_miss;
using dtof::flat_cull_far;

static uint64_t g_state;
static inline uint64_t next_u64() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float uni() { return (float) (next_u64() >> 40) * 0x1p-24f; }                 // [0, 1)
static inline float sgn_rand(float x) { return (next_u64() & 1) ? -x : x; }
static inline float logu(int lo, int hi) { return ldexpf(1.f + uni(), lo + (int) (next_u64() % (uint64_t) (hi - lo + 1))); }   // log-uniform magnitude in [2^lo, 2^(hi+1))
static inline float ulps(float x, int k) { return u2f(f2u(x) + (uint32_t) k); }               // k ulps away from x (same sign side; k < 0 towards 0)

static const float kSpecial[] = { 0.f, -0.f, INFINITY, -INFINITY, NAN, -NAN, FLT_MIN, -FLT_MIN, 0x1p-149f, -0x1p-149f, 0x1p-140f, 0x1p-127f, FLT_MAX, -FLT_MAX,
                                  1.f, -1.f, 0x1p-100f, -0x1p-100f, 0x1p-60f, 0x1p60f, 0x1p100f, -0x1p100f, 1e-30f, 1e30f, 3.40282346638528859812e+38f };
static const int kNSpecial = sizeof kSpecial / sizeof kSpecial[0];
static inline float special() { return kSpecial[next_u64() % kNSpecial]; }

struct Counts { uint64_t n = 0, culled = 0, in_range = 0, hits = 0, bad_range = 0, bad_hit = 0; };
static void check(float zx, float zy, float maxt, float lox, float loy, float ldx, float ldy, Counts &c) {
    const float t = -zx / zy;
    const float u = fmaf(ldx, t, lox), v = fmaf(ldy, t, loy);
    const bool range = t >= 0.f && t <= maxt;
    const bool hit = range && fabsf(u) <= 1.f && fabsf(v) <= 1.f;
    const bool cull = flat_certain_miss(zx, zy, flat_cull_far(maxt));
    ++c.n; c.culled += cull; c.in_range += range; c.hits += hit;
    if (cull && range) {
        if (c.bad_range < 5) fprintf(stderr, "UNSOUND zx=%a zy=%a maxt=%a t=%a\n", zx, zy, maxt, t);
        ++c.bad_range;
    }
    c.bad_hit += cull && hit;
}
// xy-row results that put u and v within an ulp of +-1 at the given t (where t is finite)
static void xy_near_one(float t, float &lo, float &ld) {
    ld = sgn_rand(logu(-4, 4));
    const float target = sgn_rand(ulps(1.f, (int) (next_u64() % 3) - 1));
    lo = std::isfinite(t) ? target - ld * t : target;
    if (!std::isfinite(lo)) lo = target;
}

static float pick_maxt() {
    switch (next_u64() % 6) {
        case 0: return special();
        case 1: return 3.40282346638528859812e+38f;      // kLargest: closest-hit rays
        case 2: return logu(-149, -126);                 // denormals / tiny
        default: return logu(-20, 20);
    }
}

int main(int argc, char **argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000000ull;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    Counts kinds[6];
    for (uint64_t i = 0; i < n; ++i) {
        const int kind = (int) (i % 6);
        float zx, zy, maxt = pick_maxt(), lox, loy, ldx, ldy;
        switch (kind) {
            case 0:   // any bit pattern
                zx = u2f((uint32_t) next_u64()); zy = u2f((uint32_t) next_u64()); maxt = (next_u64() & 3) ? maxt : u2f((uint32_t) next_u64());
                break;
            case 1:   // log-uniform magnitudes over the whole range, both signs
                zx = sgn_rand(logu(-149, 127)); zy = sgn_rand(logu(-149, 127));
                break;
            case 2:   // special values against ordinary ones
                zx = (next_u64() & 1) ? special() : sgn_rand(logu(-30, 30));
                zy = (next_u64() & 1) ? special() : sgn_rand(logu(-30, 30));
                break;
            case 3: {   // quotient within a few ulps of maxt
                zy = sgn_rand(logu(-40, 40));
                const float target = std::isfinite(maxt) && maxt > 0.f ? ulps(maxt, (int) (next_u64() % 9) - 4) : maxt;
                zx = ulps(-target * zy, (int) (next_u64() % 5) - 2);
                break;
            }
            case 4: {   // quotient within a few ulps of 0: tiny positive / negative, +-0, denormal quotients
                zy = sgn_rand((next_u64() & 1) ? logu(-20, 20) : logu(60, 127));
                const float q = (next_u64() & 3) ? sgn_rand(logu(-149, -90)) : sgn_rand(0.f);
                zx = ulps(-q * zy, (int) (next_u64() % 5) - 2);
                break;
            }
            default:   // zy near 0 (denormal, +-0, tiny)
                zy = (next_u64() & 3) ? sgn_rand(logu(-149, -100)) : sgn_rand(0.f);
                zx = (next_u64() & 1) ? sgn_rand(logu(-149, 10)) : special();
                break;
        }
        const float t = -zx / zy;
        xy_near_one(t, lox, ldx); xy_near_one(t, loy, ldy);
        check(zx, zy, maxt, lox, loy, ldx, ldy, kinds[kind]);
    }
    Counts all;
    for (const Counts &c : kinds) { all.n += c.n; all.culled += c.culled; all.in_range += c.in_range; all.hits += c.hits; all.bad_range += c.bad_range; all.bad_hit += c.bad_hit; }
    printf("inputs %llu\nculled %llu\nin_range %llu\nhits %llu\nunsound_range %llu\nunsound_hit %llu\n", (unsigned long long) all.n, (unsigned long long) all.culled,
           (unsigned long long) all.in_range, (unsigned long long) all.hits, (unsigned long long) all.bad_range, (unsigned long long) all.bad_hit);
    for (int k = 0; k < 6; ++k) printf("kind%d %llu %llu %llu %llu\n", k, (unsigned long long) kinds[k].n, (unsigned long long) kinds[k].culled, (unsigned long long) kinds[k].in_range,
                                       (unsigned long long) kinds[k].bad_range);

    // C2-like shadow rays: the five walls of a room [-1, 1]^3 open towards +z (the plane of each wall as a rectangle's z row: local z = signed distance, scaled by a
    // random factor as an object-space scale would), a point light in front of the open side, shading points on the walls lifted off their plane along the normal
    // the way spawn_ray_to offsets them; maxt = the distance to the light (1 - ShadowEpsilon).  Counts the wall tests the cull settles.
    const float nrm[5][3] = { { 0, 0, 1 }, { 1, 0, 0 }, { -1, 0, 0 }, { 0, 1, 0 }, { 0, -1, 0 } };   // inner normals: back, left, right, floor, ceiling
    const float light[3] = { 0.f, 0.f, 3.9f };
    uint64_t room_tests = 0, room_culled = 0, room_bad = 0;
    for (uint64_t i = 0; i < n / 20; ++i) {
        const int w = (int) (next_u64() % 5);
        float p[3] = { 2.f * uni() - 1.f, 2.f * uni() - 1.f, 2.f * uni() - 1.f };
        for (int k = 0; k < 3; ++k) if (nrm[w][k] != 0.f) p[k] = -nrm[w][k];   // on wall w
        float dv[3] = { light[0] - p[0], light[1] - p[1], light[2] - p[2] };
        const float dist = sqrtf(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
        const float eps = (1.f + 1.f) * 1500.f * 0x1p-24f;
        for (int k = 0; k < 3; ++k) { dv[k] /= dist; p[k] += nrm[w][k] * eps; }
        const float maxt = dist * (1.f - 1500.f * 0x1p-24f * 10.f);
        for (int v = 0; v < 5; ++v) {   // the z row of wall v: n . x + 1 (zero on the wall, positive inside), times a scale
            const float s = 0.5f + uni();
            const float z0 = nrm[v][0] * s, z1 = nrm[v][1] * s, z2 = nrm[v][2] * s, z3 = s;
            const float zx = fmaf(z2, p[2], fmaf(z1, p[1], fmaf(z0, p[0], z3))), zy = fmaf(z2, dv[2], fmaf(z1, dv[1], z0 * dv[0]));
            const float t = -zx / zy;
            const bool range = t >= 0.f && t <= maxt, cull = flat_certain_miss(zx, zy, flat_cull_far(maxt));
            ++room_tests; room_culled += cull; room_bad += cull && range;
        }
    }
    printf("room_tests %llu\nroom_culled %llu\nroom_unsound %llu\n", (unsigned long long) room_tests, (unsigned long long) room_culled, (unsigned long long) room_bad);
    return 0;
}
