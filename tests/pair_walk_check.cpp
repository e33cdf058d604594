// pair_walk_check.cpp -- the merge of trace_flat's pair form (mitsuba3dopplertof_amd/csrc/dtof_pair_walk.h) against the walk it replaces, exhaustively: five rectangles,
// the wall at index 2, every rectangle's t from a small set that holds equal values across the two halves and with the wall, t == maxt, a value above maxt, NaN and a
// rectangle whose t is the smallest of all but whose u / v miss.  The two lanes of a pair share the four plain rectangles and have a wall t of their own (their
// times differ), so a case is six choices; maxt is finite, infinite or NaN.  Host only (tests/test_pair_walk.py compiles and runs it).
#include "dtof_pair_walk.h"
#include <math.h>
#include <stdio.h>
#include <string.h>

using namespace dtof;

struct Cand { float t, u, v; bool uv_ok; };

static bool hit_of(const Cand &c, float maxt) { return (int) (c.t >= 0.f) & (int) (c.t <= maxt) & (int) c.uv_ok; }   // trace_flat's `hit`

// the walk of a kernel without the form: 0, 1, 2, 3, 4 in ascending order, strict <
static FlatBest walk(const Cand *c, float maxt) {
    FlatBest b{ maxt, 0.f, 0.f, 0xffffffffu };
    for (uint32_t k = 0; k < 5; ++k) flat_best_take(b, hit_of(c[k], maxt), c[k].t, c[k].u, c[k].v, k);
    return b;
}
// one lane of the pair form: the halves as the even and the odd lane walk them, the wall with this lane's own candidate on the lower state, then the merge
static FlatBest pair_form(const Cand *c, float maxt) {
    FlatBest lower{ maxt, 0.f, 0.f, 0xffffffffu }, upper = lower;
    for (uint32_t s = 0; s < 2; ++s) {
        flat_best_take(lower, hit_of(c[s], maxt), c[s].t, c[s].u, c[s].v, s);
        flat_best_take(upper, hit_of(c[3 + s], maxt), c[3 + s].t, c[3 + s].u, c[3 + s].v, 3 + s);
    }
    FlatBest b = lower;
    flat_best_take(b, hit_of(c[2], maxt), c[2].t, c[2].u, c[2].v, 2);
    pair_merge_upper(b, upper);
    return b;
}
static bool same(const FlatBest &a, const FlatBest &b) { return memcmp(&a.t, &b.t, 4) == 0 && memcmp(&a.u, &b.u, 4) == 0 && memcmp(&a.v, &b.v, 4) == 0 && a.obj == b.obj; }

int main() {
    const float maxts[3] = { 3.f, INFINITY, NAN };
    const int K = 7;   // per rectangle: u / v miss at the smallest t | NaN | 1 | 2 | maxt (3) | above maxt | -1
    unsigned long long cases = 0, mismatches = 0, upper_wins = 0, wall_wins = 0, lower_wins = 0, none = 0, ties_across = 0, ties_wall = 0, lanes_differ = 0, at_maxt = 0;
    for (int mi = 0; mi < 3; ++mi) {
        const float maxt = maxts[mi];
        int pick[6];   // rectangles 0, 1, 3, 4, the even lane's wall, the odd lane's wall
        for (int code = 0; code < K * K * K * K * K * K; ++code) {
            for (int j = 0, c = code; j < 6; ++j, c /= K) pick[j] = c % K;
            auto cand = [&](int p, int k) {
                const float ts[K] = { 0.5f, NAN, 1.f, 2.f, 3.f, 3.5f, -1.f };
                return Cand{ ts[p], 0.125f * (float) (k + 1), -0.0625f * (float) (k + 1), p != 0 };   // u, v name the rectangle they came from
            };
            FlatBest got[2], want[2];
            for (int lane = 0; lane < 2; ++lane) {
                const Cand c[5] = { cand(pick[0], 0), cand(pick[1], 1), cand(pick[4 + lane], 2), cand(pick[2], 3), cand(pick[3], 4) };
                want[lane] = walk(c, maxt); got[lane] = pair_form(c, maxt);
                ++cases;
                if (!same(got[lane], want[lane])) {
                    if (mismatches++ < 5) fprintf(stderr, "maxt %g picks %d %d %d %d wall %d: walk obj %d t %g, pair form obj %d t %g\n", maxt, pick[0], pick[1], pick[2], pick[3], pick[4 + lane],
                                                  (int) want[lane].obj, want[lane].t, (int) got[lane].obj, got[lane].t);
                }
                const uint32_t o = want[lane].obj;
                if (o == 0xffffffffu) ++none; else if (o < 2) ++lower_wins; else if (o == 2) ++wall_wins; else ++upper_wins;
                // equal accepted t in both halves, and between the wall and a half
                bool lo_t[K] = { false }, hi_t[K] = { false };
                for (int j = 0; j < 2; ++j) { if (hit_of(c[j], maxt) && c[j].t < maxt) lo_t[pick[j]] = true; if (hit_of(c[3 + j], maxt) && c[3 + j].t < maxt) hi_t[pick[2 + j]] = true; }
                for (int p = 0; p < K; ++p) {
                    if (lo_t[p] && hi_t[p]) ++ties_across;
                    if ((lo_t[p] || hi_t[p]) && pick[4 + lane] == p) ++ties_wall;
                }
                for (int j = 0; j < 5; ++j) if (c[j].t == maxt && c[j].uv_ok) { ++at_maxt; break; }
            }
            if (!same(want[0], want[1])) ++lanes_differ;
        }
    }
    printf("cases %llu\nmismatches %llu\nnone %llu\nlower_wins %llu\nwall_wins %llu\nupper_wins %llu\nties_across %llu\nties_wall %llu\nlanes_differ %llu\nat_maxt %llu\n",
           cases, mismatches, none, lower_wins, wall_wins, upper_wins, ties_across, ties_wall, lanes_differ, at_maxt);
    return mismatches ? 1 : 0;
}
