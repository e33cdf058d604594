// math_sweep -- the float32 building blocks of dtof_math.h, swept on the device against exact references (tests/test_math_sweep_gpu.py and
// tests/test_math_sweep_cpu.py build and run it; `make -C mitsuba3dopplertof_amd/csrc sweep` compiles it with exactly the kernels' $(HIPFLAGS)).
//
// usage: math_sweep list
//        math_sweep <case> [--cpu] [--oracle liboracle.so] [--seed S] [--extra d1,d2,...] [--candidate]
//        math_sweep accuracy --oracle liboracle.so
// A case is a struct below: operands (up to six 32-bit words), an input generator that is a pure function of (element index, element count, seed) and
// runs on the device (nothing is uploaded; the host regenerates the operands when it compares), the __host__ __device__ function under test, and a host
// reference.  Results come back in chunks of 2^24 elements and are compared by min(16, OMP_NUM_THREADS or hardware threads) host threads while the device
// works on the next chunk.  Equality is by bit pattern; two NaNs are equal (sign and payload are not part of the contract); -0 and +0 differ.
// --cpu runs the HOST compilation of the function under test over a thinned index space and never touches the HIP runtime; the restated transcendentals
// then take the oracle's orc_* exports as their reference (--oracle).  Output: "key value..." lines; exit status 0 whenever the run reached its end.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <thread>
#include <vector>
#include "dtof_math.h"
#include "dtof_sampling.h"   // kInvTwoPiF
#ifdef DTOF_SWEEP_CANDIDATE
#include "candidates/div_unscaled.h"
#endif

using namespace dtof;

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fprintf(stderr, "math_sweep: %s failed: %s (%s:%d)\n", #call, hipGetErrorString(e_), __FILE__, __LINE__); exit(3); } } while (0)

struct In { uint32_t v[6]; };
struct Out { uint32_t v[3]; };
constexpr uint32_t kChunk = 1u << 24;
constexpr int kMaxWords = 4;   // up to three result words and the operand checksum

// ---------------------------------------------------------------------------------------------------------------- generator helpers (host == device, integer only)
DTOF_HD uint64_t mix64(uint64_t i, uint64_t seed) {   // splitmix64 finaliser of a counter
    uint64_t z = (i + 1) * 0x9e3779b97f4a7c15ull + seed * 0xd1342543de82ef95ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
DTOF_HD uint32_t ilog2_u64(uint64_t n) { return 63u - (uint32_t) __builtin_clzll(n); }   // n >= 1
// every bit pattern when n = 2^32; for a thinned run of n = 2^k elements the high k bits count up and the low bits are zero (even i: +-0, inf, the quiet NaN,
// powers of two stay in) or random (odd i)
DTOF_HD uint32_t sweep_u32(uint64_t i, uint64_t n, uint64_t seed) {
    const uint32_t k = ilog2_u64(n);
    if (k >= 32) return (uint32_t) i;
    const uint32_t sh = 32 - k, low = (i & 1) ? (uint32_t) mix64(i, seed) & ((1u << sh) - 1) : 0u;
    return (uint32_t) (i << sh) | low;
}
// a normal float with a random sign and fraction and an exponent uniform in [lo, hi]
DTOF_HD uint32_t rand_normal(uint64_t h, int lo, int hi) {
    const uint32_t e = (uint32_t) (lo + 127 + (int) ((h >> 24) % (uint64_t) (hi - lo + 1)));
    return ((uint32_t) (h >> 63) << 31) | (e << 23) | ((uint32_t) h & 0x007fffffu);
}
DTOF_HD uint32_t ulp_step(uint32_t u, int k) { return u + (uint32_t) k; }   // k ulps away from zero (k < 0: towards it); callers keep clear of the ends
DTOF_HD uint32_t kind_of(uint64_t i, uint64_t n, uint32_t kinds) { return (uint32_t) ((i * kinds) >> ilog2_u64(n)); }   // n a power of two <= 2^35, kinds <= 8
DTOF_HD uint32_t in_checksum(const In &in) {
    uint32_t c = 0x811c9dc5u;
    for (int k = 0; k < 6; ++k) c = (c ^ in.v[k]) * 0x01000193u;
    return c;
}
// sixteen special values: zeros, infinities, NaNs (quiet and signalling pattern), the smallest and largest denormal, the smallest normal, +-FLT_MAX, +-1, 1 - ulp
DTOF_HD uint32_t special_bits(uint32_t k) {
    switch (k & 15) { case 0: return 0x00000000u; case 1: return 0x80000000u; case 2: return 0x7f800000u; case 3: return 0xff800000u; case 4: return 0x7fc00000u;
        case 5: return 0xffc00000u; case 6: return 0x00000001u; case 7: return 0x80000001u; case 8: return 0x007fffffu; case 9: return 0x00800000u;
        case 10: return 0x7f7fffffu; case 11: return 0xff7fffffu; case 12: return 0x3f800000u; case 13: return 0xbf800000u; case 14: return 0x7f800001u; default: return 0x3f7fffffu; }
}

DTOF_HD uint32_t bits_or_special(uint64_t h) { return (h >> 60) == 0 ? special_bits((uint32_t) (h >> 40)) : (uint32_t) h; }   // random bit pattern, one in 16 a special value
// ---------------------------------------------------------------------------------------------------------------- host-side classification
static inline bool is_nan_bits(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }
static inline bool is_inf_bits(uint32_t u) { return (u & 0x7fffffffu) == 0x7f800000u; }
static inline bool is_den_bits(uint32_t u) { return (u & 0x7f800000u) == 0 && (u & 0x007fffffu) != 0; }
static inline bool same_bits(uint32_t a, uint32_t b) { return a == b || (is_nan_bits(a) && is_nan_bits(b)); }
static inline float hf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t hu(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

enum { CL_DENORM_IN, CL_DENORM_OUT, CL_OVERFLOW, CL_NAN_IN, CL_INF_IN, CL_ZERO_IN, CL_NAN_OUT, CL_EXACT, CL_UP, CL_DOWN, CL_TIE, CL_COUNT };
static const char *kClassName[CL_COUNT] = { "denormal_in", "denormal_out", "overflow", "nan_in", "inf_in", "zero_in", "nan_out", "exact", "rounded_up", "rounded_down", "tie" };
#define M(x) (1u << (x))
constexpr uint32_t kFloatIn = M(CL_DENORM_IN) | M(CL_NAN_IN) | M(CL_INF_IN) | M(CL_ZERO_IN);
constexpr uint32_t kRounding = M(CL_EXACT) | M(CL_UP) | M(CL_DOWN);
enum { R_NONE = -1, R_EXACT = CL_EXACT, R_UP = CL_UP, R_DOWN = CL_DOWN, R_TIE = CL_TIE };

// the rounding class of the float r against the exact value s + err (|err| far below an ulp of s): where the exact value lies relative to r
static int round_class(double s, double err, float r) {
    if (!std::isfinite(s) || !std::isfinite(r)) return R_NONE;
    const double d = (s - (double) r) + err;          // exact value minus result
    if (d == 0.0) return R_EXACT;
    const float r2 = nextafterf(r, d > 0 ? INFINITY : -INFINITY);
    if (std::isfinite(r2)) {
        const double mid = 0.5 * ((double) r + (double) r2);
        if ((s - mid) + err == 0.0) return R_TIE;
    }
    return d > 0 ? R_DOWN : R_UP;                     // the result is below / above the exact value
}
// a / b: the residual a - q b is one rounding of an exactly representable product and a sum, its sign is exact
static int div_class(float a, float b, float q) {
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(q) || b == 0.f) return R_NONE;
    const double res = fma(-(double) q, (double) b, (double) a);
    if (res == 0.0) return R_EXACT;
    const bool above = (res > 0) == (b > 0);          // exact quotient above q
    const float q2 = nextafterf(q, above ? INFINITY : -INFINITY);
    if (std::isfinite(q2) && fma(-0.5 * ((double) q + (double) q2), (double) b, (double) a) == 0.0) return R_TIE;
    return above ? R_DOWN : R_UP;
}

struct Mismatch { uint64_t index; In in; Out got, ref; };
struct Tally {
    uint64_t inputs = 0, mismatches = 0, excluded = 0, excluded_mismatches = 0, gen_mismatches = 0;
    uint64_t cls[CL_COUNT] = {}, kind_n[8] = {}, kind_bad[8] = {};
    uint64_t cand[5][2] = {};                         // candidate slot: operand class -> inputs, mismatches
    uint64_t safe[2] = {};                            // candidate slot: inputs and mismatches inside the window the class table claims to be safe
    // candidate slot, operand pairs with normal operands that break exactly ONE condition of the window: inputs, mismatches, and over the mismatches the range of
    // the exponent that condition bounds (b, b, a, a - b, a - b)
    uint64_t only[5][2] = {};
    int only_exp[5][2] = { { 999, -999 }, { 999, -999 }, { 999, -999 }, { 999, -999 }, { 999, -999 } };
    std::vector<Mismatch> first;
    void note(const Mismatch &m) { if (first.size() < 8) first.push_back(m); }
    void merge(const Tally &o) {
        inputs += o.inputs; mismatches += o.mismatches; excluded += o.excluded; excluded_mismatches += o.excluded_mismatches; gen_mismatches += o.gen_mismatches;
        for (int k = 0; k < CL_COUNT; ++k) cls[k] += o.cls[k];
        for (int k = 0; k < 8; ++k) { kind_n[k] += o.kind_n[k]; kind_bad[k] += o.kind_bad[k]; }
        for (int k = 0; k < 5; ++k) { cand[k][0] += o.cand[k][0]; cand[k][1] += o.cand[k][1]; }
        safe[0] += o.safe[0]; safe[1] += o.safe[1];
        for (int k = 0; k < 5; ++k) {
            only[k][0] += o.only[k][0]; only[k][1] += o.only[k][1];
            only_exp[k][0] = std::min(only_exp[k][0], o.only_exp[k][0]); only_exp[k][1] = std::max(only_exp[k][1], o.only_exp[k][1]);
        }
        for (const Mismatch &m : o.first) first.push_back(m);
        std::sort(first.begin(), first.end(), [](const Mismatch &a, const Mismatch &b) { return a.index < b.index; });
        if (first.size() > 8) first.resize(8);
    }
};

// the oracle's exports (--oracle; the reference of the restated transcendentals under --cpu)
static struct Orc {
    float (*expf_)(float) = nullptr; float (*logf_)(float) = nullptr; float (*tanf_)(float) = nullptr; float (*erff_)(float) = nullptr; float (*erfinvf_)(float) = nullptr;
    float (*acos_)(float) = nullptr; float (*atan2f_)(float, float) = nullptr; void (*sincos_)(float, float *, float *) = nullptr;
    bool loaded = false;
} g_orc;
static bool g_cpu = false, g_candidate = false;
static void load_oracle(const char *path) {
    void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "math_sweep: cannot load %s: %s\n", path, dlerror()); exit(2); }
    auto sym = [&](const char *n) { void *p = dlsym(h, n); if (!p) { fprintf(stderr, "math_sweep: %s lacks %s\n", path, n); exit(2); } return p; };
    g_orc.expf_ = (float (*)(float)) sym("orc_expf"); g_orc.logf_ = (float (*)(float)) sym("orc_logf"); g_orc.tanf_ = (float (*)(float)) sym("orc_tanf");
    g_orc.erff_ = (float (*)(float)) sym("orc_erff"); g_orc.erfinvf_ = (float (*)(float)) sym("orc_erfinvf"); g_orc.acos_ = (float (*)(float)) sym("orc_acos");
    g_orc.atan2f_ = (float (*)(float, float)) sym("orc_atan2f"); g_orc.sincos_ = (void (*)(float, float *, float *)) sym("orc_sincos");
    g_orc.loaded = true;
}
static void need_oracle() { if (!g_orc.loaded) { fprintf(stderr, "math_sweep: this case needs --oracle under --cpu\n"); exit(2); } }

// ---------------------------------------------------------------------------------------------------------------- the cases
// Every case: NOUT result words, N_GPU / N_CPU elements, CHECK_GEN (the generator does arithmetic: the device returns a checksum of its operands and the host
// compares it with its own), CLASSES (the class counts the case promises to be non-zero), KINDS (generator regions, each promised non-zero),
// gen, fut (the function under test), ref (host), excluded, rounding.
struct CaseBase {
    static constexpr int NOUT = 1, KINDS = 1, NIN = 1;
    static constexpr bool CHECK_GEN = false, FLOAT_IN = true, FLOAT_OUT = true, HAS_CAND = false;
    static constexpr uint64_t N_GPU = 1ull << 32, N_CPU = 1ull << 28;
    static constexpr uint32_t CLASSES = 0;
    static const char *exclusion() { return nullptr; }
    static bool excluded(const In &) { return false; }
    static int rounding(const In &, const Out &) { return R_NONE; }
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) { in.v[0] = sweep_u32(i, n, seed); }
};

// ---- A. IEEE primitives as the device compiles them; reference: double precision, rounded once
struct CaseRcp : CaseBase {
    static constexpr uint32_t CLASSES = kFloatIn | kRounding | M(CL_DENORM_OUT) | M(CL_OVERFLOW);   // no ties: 2^150 / odd is no float
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(rcp(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { o.v[0] = hu((float) (1.0 / (double) hf(in.v[0]))); }
    static int rounding(const In &in, const Out &r) { return div_class(1.f, hf(in.v[0]), hf(r.v[0])); }
};
struct CaseSqrt : CaseBase {
    static constexpr uint32_t CLASSES = kFloatIn | kRounding | M(CL_NAN_OUT);
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(sqrtf(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { o.v[0] = hu((float) sqrt((double) hf(in.v[0]))); }
    static int rounding(const In &in, const Out &r) {   // x - q^2 is exact in double (48-bit product, nearby operands) up to one harmless rounding: its sign is exact
        const float x = hf(in.v[0]), q = hf(r.v[0]);
        if (!(x > 0.f) || !std::isfinite(x)) return R_NONE;
        const double res = fma(-(double) q, (double) q, (double) x);
        return res == 0.0 ? R_EXACT : res > 0 ? R_DOWN : R_UP;
    }
};
struct CaseRsqrt : CaseBase {   // two roundings, in that order
    static constexpr uint32_t CLASSES = kFloatIn | kRounding | M(CL_NAN_OUT) | M(CL_OVERFLOW);
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(rsqrt_(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { const float t = (float) (1.0 / (double) hf(in.v[0])); o.v[0] = hu((float) sqrt((double) t)); }
    static int rounding(const In &in, const Out &r) {
        const float t = (float) (1.0 / (double) hf(in.v[0])), q = hf(r.v[0]);
        if (!(t > 0.f) || !std::isfinite(t)) return R_NONE;
        const double res = fma(-(double) q, (double) q, (double) t);
        return res == 0.0 ? R_EXACT : res > 0 ? R_DOWN : R_UP;
    }
};
struct CaseSafeSqrt : CaseBase {
    static constexpr uint32_t CLASSES = kFloatIn | kRounding;
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(safe_sqrt(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { const float x = hf(in.v[0]); o.v[0] = hu((float) sqrt((double) (x > 0.f ? x : 0.f))); }   // fmax_(NaN, 0) = 0
    static int rounding(const In &in, const Out &r) { return CaseSqrt::rounding(in, r); }
};
struct CaseSignf : CaseBase {
    static constexpr uint32_t CLASSES = kFloatIn;
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(signf(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { o.v[0] = hu(std::signbit(hf(in.v[0])) ? -1.f : 1.f); }
};
struct CaseTrunc : CaseBase {
    static constexpr uint32_t CLASSES = kFloatIn;
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(truncf(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { o.v[0] = hu((float) trunc((double) hf(in.v[0]))); }
};
struct CaseFloor : CaseBase {
    static constexpr uint32_t CLASSES = kFloatIn;
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(floorf(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { o.v[0] = hu((float) floor((double) hf(in.v[0]))); }
};
struct CaseF2I : CaseBase {     // (int32_t) x for |x| < 2^31; everything else is undefined in C++ and excluded
    static constexpr bool FLOAT_OUT = false;
    static constexpr uint32_t CLASSES = M(CL_DENORM_IN) | M(CL_ZERO_IN);
    static const char *exclusion() { return "float -> int conversion of a value outside int32 (|x| >= 2^31, inf, NaN)"; }
    static bool excluded(const In &in) { return (in.v[0] & 0x7fffffffu) >= 0x4f000000u; }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = (uint32_t) (int32_t) u2f(in.v[0]); }
    static void ref(const In &in, Out &o) { o.v[0] = (uint32_t) (int32_t) (int64_t) trunc((double) hf(in.v[0])); }
};
struct CaseI2F : CaseBase {
    static constexpr bool FLOAT_IN = false;
    static constexpr uint32_t CLASSES = kRounding | M(CL_TIE);
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u((float) (int32_t) in.v[0]); }
    static void ref(const In &in, Out &o) { o.v[0] = hu((float) (double) (int32_t) in.v[0]); }
    static int rounding(const In &in, const Out &r) { return round_class((double) (int32_t) in.v[0], 0.0, hf(r.v[0])); }
};
struct CaseU2F : CaseBase {
    static constexpr bool FLOAT_IN = false;
    static constexpr uint32_t CLASSES = kRounding | M(CL_TIE);
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u((float) in.v[0]); }
    static void ref(const In &in, Out &o) { o.v[0] = hu((float) (double) in.v[0]); }
    static int rounding(const In &in, const Out &r) { return round_class((double) in.v[0], 0.0, hf(r.v[0])); }
};

// a / b on 2^32 pairs.  kinds: 0 every pair of exponents (denormal range included) x fraction patterns x signs; 1 quotients that are denormal, next to the smallest
// normal, next to the largest float; 2 a within an ulp of q b for a float q; 3 ... for a q halfway between two floats (near-ties); 4 1 / det-like operands, both
// in [2^-40, 2^40]; 5-7 uniformly random bit patterns
DTOF_HD uint32_t frac_pattern(uint32_t sel, uint64_t h) {
    switch (sel & 7) { case 0: return 0; case 1: return 1; case 2: return 0x7fffffu; case 3: return 0x400000u; case 4: return 0x555555u; case 5: return 0x2aaaaau;
        default: return (uint32_t) (h >> (sel & 1 ? 7 : 31)) & 0x7fffffu; }
}
struct CaseDiv : CaseBase {
    static constexpr int KINDS = 8, NIN = 2;
    static constexpr bool CHECK_GEN = true;
#ifdef DTOF_SWEEP_CANDIDATE
    static constexpr bool HAS_CAND = true;
    DTOF_HD static void cand(const In &in, Out &o) { o.v[0] = f2u(div_unscaled(u2f(in.v[0]), u2f(in.v[1]))); }
#endif
    static constexpr uint32_t CLASSES = kFloatIn | kRounding | M(CL_DENORM_OUT) | M(CL_OVERFLOW) | M(CL_NAN_OUT) | M(CL_TIE);
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) {
        const uint64_t h = mix64(i, seed), h2 = mix64(h, 17);
        const uint32_t kind = kind_of(i, n, 8);
        uint32_t a, b;
        if (kind == 0) {
            a = ((uint32_t) (i >> 22 & 1) << 31) | ((uint32_t) (i & 255) << 23) | frac_pattern((uint32_t) (i >> 16), h);
            b = ((uint32_t) (i >> 23 & 1) << 31) | ((uint32_t) (i >> 8 & 255) << 23) | frac_pattern((uint32_t) (i >> 19), h2);
        } else if (kind <= 3) {
            uint32_t q;
            if (kind == 1) {
                const uint32_t sel = (uint32_t) (h2 >> 40) & 3;
                b = rand_normal(h, sel == 2 ? -60 : 0, sel == 2 ? -1 : 60);
                q = sel == 0 ? 1u + (uint32_t) ((h2 >> 8) % 0x7fffffu) : sel == 1 ? 0x00800000u + (uint32_t) (h2 >> 8 & 7) - 4u : sel == 2 ? 0x7f7fffffu - (uint32_t) (h2 >> 8 & 3)
                                                                                                                                 : 0x00800000u - (uint32_t) (h2 >> 8 & 0xffff);
            } else {
                b = rand_normal(h, -30, 30);
                q = rand_normal(h2, -30, 30);
            }
            // the float nearest q b (kind 3: (q + half an ulp) b, computed as q b + (ulp(q) / 2) b) and its two neighbours
            float p = u2f(q) * u2f(b);
            if (kind == 3) p = fmaf(u2f((q & 0x7f800000u) - (24u << 23)), u2f(b), p);
            a = ulp_step(f2u(p), (int) ((h2 >> 44) % 3) - 1);
        } else if (kind == 4) {
            a = rand_normal(h, -40, 39); b = rand_normal(h2, -40, 39);
        } else { a = bits_or_special(h); b = bits_or_special(h2); }
        in.v[0] = a; in.v[1] = b;
    }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(u2f(in.v[0]) / u2f(in.v[1])); }
    static void ref(const In &in, Out &o) { o.v[0] = hu((float) ((double) hf(in.v[0]) / (double) hf(in.v[1]))); }
    static int rounding(const In &in, const Out &r) { return div_class(hf(in.v[0]), hf(in.v[1]), hf(r.v[0])); }
};

// fmaf / lerp_ / dot / cross: the reference is the host compilation of the same function -- fused exactly where fmaf is written and nowhere else.
// kinds: 0 random bit patterns, 1 random operands of moderate exponent, 2-3 cancellation-heavy operands
struct CaseFma : CaseBase {
    static constexpr int KINDS = 4, NIN = 3;
    static constexpr bool CHECK_GEN = true;
    static constexpr uint64_t N_GPU = 1ull << 30, N_CPU = 1ull << 26;
    static constexpr uint32_t CLASSES = kFloatIn | kRounding | M(CL_DENORM_OUT) | M(CL_OVERFLOW) | M(CL_NAN_OUT) | M(CL_TIE);
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) {
        const uint64_t h = mix64(i, seed), h2 = mix64(h, 17), h3 = mix64(h, 29);
        const uint32_t kind = kind_of(i, n, 4);
        if (kind == 0) { in.v[0] = bits_or_special(h); in.v[1] = bits_or_special(h2); in.v[2] = bits_or_special(h3); return; }
        const int span = kind == 3 ? 60 : 20;
        in.v[0] = rand_normal(h, -span, span); in.v[1] = rand_normal(h2, -span, span); in.v[2] = rand_normal(h3, -20, 20);
        // a b within a few ulps of -c (kind 3: over the whole exponent range, so that the residual is often denormal; half of them with the low fraction bits of
        // a and b cleared, which makes a b a float or a tie between two floats)
        if (kind == 1 && (h3 & (1ull << 51))) {   // a 12-bit times a 13-bit significand plus nothing: a b is a float or exactly halfway between two
            in.v[0] &= ~0xfffu; in.v[1] &= ~0x7ffu; in.v[2] = (uint32_t) (h3 >> 52 & 1) << 31;
        }
        if (kind >= 2) {
            if (h3 & (1ull << 50)) { in.v[0] &= ~0xfffu; in.v[1] &= ~0x7ffu; }
            in.v[2] = ulp_step(f2u(-(u2f(in.v[0]) * u2f(in.v[1]))), (int) ((h3 >> 40) % 7) - 3);
        }
    }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(fmaf(u2f(in.v[0]), u2f(in.v[1]), u2f(in.v[2]))); }
    static void ref(const In &in, Out &o) { o.v[0] = hu(fmaf(hf(in.v[0]), hf(in.v[1]), hf(in.v[2]))); }   // the C library's, correctly rounded
    static int rounding(const In &in, const Out &r) {
        const double p = (double) hf(in.v[0]) * (double) hf(in.v[1]), c = hf(in.v[2]), s = p + c;   // p is exact; two-sum for the error of s
        const double bb = s - p, err = (p - (s - bb)) + (c - bb);
        return round_class(s, err, hf(r.v[0]));
    }
};
struct CaseLerp : CaseBase {
    static constexpr int KINDS = 4, NIN = 3;
    static constexpr bool CHECK_GEN = true;
    static constexpr uint64_t N_GPU = 1ull << 30, N_CPU = 1ull << 26;
    static constexpr uint32_t CLASSES = kFloatIn | M(CL_DENORM_OUT) | M(CL_OVERFLOW) | M(CL_NAN_OUT);
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) {
        const uint64_t h = mix64(i, seed), h2 = mix64(h, 17), h3 = mix64(h, 29);
        const uint32_t kind = kind_of(i, n, 4);
        if (kind == 0) { in.v[0] = bits_or_special(h); in.v[1] = bits_or_special(h2); in.v[2] = bits_or_special(h3); return; }
        in.v[0] = rand_normal(h, -20, 20); in.v[1] = rand_normal(h2, -20, 20);
        in.v[2] = f2u(u2f(((uint32_t) h3 >> 9) | 0x3f800000u) - 1.f);                                   // t in [0, 1)
        if (kind >= 2) {   // t = 2^-k: b t within a few ulps of -(a - a t)
            const uint32_t k = 1 + (uint32_t) (h3 >> 40) % (kind == 3 ? 100 : 10);
            if (kind == 3) in.v[0] = rand_normal(h, -126, -60);                                        // ... and the inner term denormal or nearly so
            const float t = u2f((127u - (k > 60 ? 60 : k)) << 23), a = u2f(in.v[0]);
            in.v[2] = f2u(t);
            in.v[1] = ulp_step(f2u(-fmaf(-a, t, a) * u2f((127u + (k > 60 ? 60 : k)) << 23)), (int) ((h3 >> 50) % 5) - 2);
        }
    }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(lerp_(u2f(in.v[0]), u2f(in.v[1]), u2f(in.v[2]))); }
    static void ref(const In &in, Out &o) { fut(in, o); }
};
DTOF_HD V3 v3_of(const In &in, int at) { return mk(u2f(in.v[at]), u2f(in.v[at + 1]), u2f(in.v[at + 2])); }
struct CaseDot : CaseBase {
    static constexpr int KINDS = 4, NIN = 6;
    static constexpr bool CHECK_GEN = true;
    static constexpr uint64_t N_GPU = 1ull << 30, N_CPU = 1ull << 26;
    static constexpr uint32_t CLASSES = kFloatIn | M(CL_DENORM_OUT) | M(CL_OVERFLOW) | M(CL_NAN_OUT);
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) {
        const uint32_t kind = kind_of(i, n, 4);
        const uint64_t h = mix64(i, seed);
        for (int k = 0; k < 6; ++k) { const uint64_t hk = mix64(h, 3 + k); in.v[k] = kind == 0 ? bits_or_special(hk) : rand_normal(hk, kind == 3 ? -63 : -10, kind == 3 ? -40 : 10); }
        if (kind >= 2) {   // a.z = 2^k, b.z within a few ulps of -(a.x b.x + a.y b.y) 2^-k: the outer fmaf cancels
            const uint32_t k = (uint32_t) (h >> 40) % 8;
            const float inner = fmaf(u2f(in.v[1]), u2f(in.v[4]), u2f(in.v[0]) * u2f(in.v[3]));
            in.v[2] = (127u + k) << 23;
            in.v[5] = ulp_step(f2u(-inner * u2f((127u - k) << 23)), (int) ((h >> 50) % 5) - 2);
        }
    }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(dot(v3_of(in, 0), v3_of(in, 3))); }
    static void ref(const In &in, Out &o) { fut(in, o); }
};
struct CaseCross : CaseBase {
    static constexpr int NOUT = 3, KINDS = 4, NIN = 6;
    static constexpr bool CHECK_GEN = true;
    static constexpr uint64_t N_GPU = 1ull << 30, N_CPU = 1ull << 26;
    static constexpr uint32_t CLASSES = kFloatIn | M(CL_DENORM_OUT) | M(CL_OVERFLOW) | M(CL_NAN_OUT);
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) {
        const uint32_t kind = kind_of(i, n, 4);
        const uint64_t h = mix64(i, seed);
        for (int k = 0; k < 6; ++k) { const uint64_t hk = mix64(h, 3 + k); in.v[k] = kind == 0 ? bits_or_special(hk) : rand_normal(hk, kind == 3 ? -63 : -10, kind == 3 ? -40 : 10); }
        if (kind >= 2) {   // b = 2^k a with every component moved by a few ulps: nearly parallel, every component cancels
            const uint32_t k = (uint32_t) (h >> 40) % 8;
            for (int c = 0; c < 3; ++c) in.v[3 + c] = ulp_step(f2u(u2f(in.v[c]) * u2f((127u + k) << 23)), (int) ((h >> (44 + 4 * c)) % 5) - 2);
        }
    }
    DTOF_HD static void fut(const In &in, Out &o) { const V3 c = cross(v3_of(in, 0), v3_of(in, 3)); o.v[0] = f2u(c.x); o.v[1] = f2u(c.y); o.v[2] = f2u(c.z); }
    static void ref(const In &in, Out &o) { fut(in, o); }
};

// ---- B. hand-made exact routines; reference: the definition
struct CaseFmod2Pi : CaseBase {
    static constexpr uint32_t CLASSES = kFloatIn | M(CL_DENORM_OUT) | M(CL_NAN_OUT) | M(CL_EXACT);
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(fmod_pos(u2f(in.v[0]), 2.f * kPi, kInvTwoPiF)); }
    static void ref(const In &in, Out &o) { o.v[0] = hu(fmodf(hf(in.v[0]), 2.f * kPi)); }
    static int rounding(const In &in, const Out &r) { return std::isfinite(hf(in.v[0])) && hf(r.v[0]) == hf(in.v[0]) ? R_EXACT : R_NONE; }   // |x| < y: x itself
};
// fmod_pos(x, y, 1 / y) for y in [2^-20, 2^20].  kinds: 0 any x, 1 |x| < 2^22 y, 2 x within a few ulps of a multiple k y (k up to 2^22 + 3: across the end of
// the fast branch), 3 |x| within a few ulps of 2^22 y
struct CaseFmodXY : CaseBase {
    static constexpr int KINDS = 4, NIN = 2;
    static constexpr bool CHECK_GEN = true;
    static constexpr uint64_t N_GPU = 1ull << 30, N_CPU = 1ull << 26;
    static constexpr uint32_t CLASSES = kFloatIn | M(CL_NAN_OUT) | M(CL_DENORM_OUT);
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) {
        const uint64_t h = mix64(i, seed), h2 = mix64(h, 17);
        const uint32_t kind = kind_of(i, n, 4);
        const uint32_t y = rand_normal(h, -20, 19) & 0x7fffffffu;
        uint32_t x;
        if (kind == 0) x = bits_or_special(h2);
        else if (kind == 1) x = f2u(u2f(rand_normal(h2, -30, 21)) * u2f(y));
        else if (kind == 2) x = ulp_step(f2u((float) (uint32_t) ((h2 >> 8) % ((h2 & 1) ? 4194308u : 16u)) * u2f(y)), (int) ((h2 >> 40) % 5) - 2) ^ ((uint32_t) (h2 >> 63) << 31);
        else x = ulp_step(f2u(4194304.f * u2f(y)), (int) ((h2 >> 40) % 9) - 4) ^ ((uint32_t) (h2 >> 63) << 31);
        in.v[0] = x; in.v[1] = y;
    }
    DTOF_HD static void fut(const In &in, Out &o) { const float y = u2f(in.v[1]); o.v[0] = f2u(fmod_pos(u2f(in.v[0]), y, 1.0f / y)); }
    static void ref(const In &in, Out &o) { o.v[0] = hu(fmodf(hf(in.v[0]), hf(in.v[1]))); }
};
struct CasePcgJump6 : CaseBase {
    static constexpr int NOUT = 2, NIN = 4;
    static constexpr bool FLOAT_IN = false, FLOAT_OUT = false;
    static constexpr uint64_t N_GPU = 1ull << 30, N_CPU = 1ull << 26;
    DTOF_HD static void gen(uint64_t i, uint64_t, uint64_t seed, In &in) {
        const uint64_t s = mix64(i, seed), inc = mix64(s, 5);
        in.v[0] = (uint32_t) s; in.v[1] = (uint32_t) (s >> 32); in.v[2] = (uint32_t) inc; in.v[3] = (uint32_t) (inc >> 32);
    }
    DTOF_HD static void fut(const In &in, Out &o) {
        const uint64_t r = pcg_jump6((uint64_t) in.v[0] | (uint64_t) in.v[1] << 32, (uint64_t) in.v[2] | (uint64_t) in.v[3] << 32);
        o.v[0] = (uint32_t) r; o.v[1] = (uint32_t) (r >> 32);
    }
    static void ref(const In &in, Out &o) {
        uint64_t s = (uint64_t) in.v[0] | (uint64_t) in.v[1] << 32; const uint64_t inc = (uint64_t) in.v[2] | (uint64_t) in.v[3] << 32;
        for (int k = 0; k < 6; ++k) pcg_next_u32(s, inc);
        o.v[0] = (uint32_t) s; o.v[1] = (uint32_t) (s >> 32);
    }
};
struct CasePcgOutput : CasePcgJump6 {
    static constexpr int NOUT = 1;
    static constexpr bool FLOAT_OUT = true;
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(pcg_output_f32((uint64_t) in.v[0] | (uint64_t) in.v[1] << 32)); }
    static void ref(const In &in, Out &o) { uint64_t s = (uint64_t) in.v[0] | (uint64_t) in.v[1] << 32; o.v[0] = hu(pcg_next_f32(s, (uint64_t) in.v[2] | (uint64_t) in.v[3] << 32)); }
};
// mulsign / mulsign_neg: every a for b in {+-0, +-1, +-NaN, +-inf}; the definition: a with its sign flipped when b is negative (mulsign_neg: when it is not)
struct CaseMulsign : CaseBase {
    static constexpr int NIN = 2;
    static constexpr uint64_t N_GPU = 8ull << 32, N_CPU = 8ull << 25;
    static constexpr uint32_t CLASSES = kFloatIn;
    DTOF_HD static uint32_t b_of(uint32_t k) { const uint32_t m = k >> 1 == 0 ? 0u : k >> 1 == 1 ? 0x3f800000u : k >> 1 == 2 ? 0x7fc00000u : 0x7f800000u; return m | (k & 1) << 31; }
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) { const uint64_t per = n >> 3; in.v[0] = sweep_u32(i & (per - 1), per, seed); in.v[1] = b_of((uint32_t) (i >> ilog2_u64(per))); }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(mulsign(u2f(in.v[0]), u2f(in.v[1]))); }
    static void ref(const In &in, Out &o) { o.v[0] = (in.v[1] >> 31) ? in.v[0] ^ 0x80000000u : in.v[0]; }
};
struct CaseMulsignNeg : CaseMulsign {
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(mulsign_neg(u2f(in.v[0]), u2f(in.v[1]))); }
    static void ref(const In &in, Out &o) { o.v[0] = (in.v[1] >> 31) ? in.v[0] : in.v[0] ^ 0x80000000u; }
};

// ---- C. restated transcendentals: the device against the host compilation of the same function (under --cpu: the host against the oracle's export)
// The one exclusion: inputs whose float -> int conversion inside the function leaves int32 (undefined in C++; x86 gives INT_MIN, the GPU saturates).
static bool octant_conversion_out_of_range(uint32_t u) { const float q = fabsf(hf(u)) * 1.2732395447351626862f; return !(q < 2147483648.f); }   // NaN included
#define TRANSCENDENTAL(NAME, FN, ORC, EXCL_REASON, EXCL_EXPR, CLS)                                                                                  \
    struct NAME : CaseBase {                                                                                                                          \
        static constexpr uint64_t N_CPU = 1ull << 26;                                                                                                 \
        static constexpr uint32_t CLASSES = (CLS);                                                                                                    \
        static const char *exclusion() { return EXCL_REASON; }                                                                                        \
        static bool excluded(const In &in) { const uint32_t u = in.v[0]; (void) u; return EXCL_EXPR; }                                                \
        DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(FN(u2f(in.v[0]))); }                                                             \
        static void ref(const In &in, Out &o) { if (g_cpu) { need_oracle(); o.v[0] = hu(g_orc.ORC(hf(in.v[0]))); } else fut(in, o); }                  \
    }
static const char kExclOctant[] = "float -> int conversion of a value outside int32, unreachable from every caller: |x| 4/pi >= 2^31 or NaN";
static const char kExclNan[] = "float -> int conversion of a value outside int32, unreachable from every caller: x is NaN";
TRANSCENDENTAL(CaseExp, exp_, expf_, kExclNan, is_nan_bits(u), M(CL_DENORM_IN) | M(CL_INF_IN) | M(CL_ZERO_IN) | M(CL_DENORM_OUT) | M(CL_OVERFLOW));
TRANSCENDENTAL(CaseLog, log_, logf_, nullptr, false, kFloatIn | M(CL_NAN_OUT));
TRANSCENDENTAL(CaseTan, tan_, tanf_, kExclOctant, octant_conversion_out_of_range(u), M(CL_DENORM_IN) | M(CL_ZERO_IN));
TRANSCENDENTAL(CaseErf, erf_, erff_, kExclNan, is_nan_bits(u), M(CL_DENORM_IN) | M(CL_INF_IN) | M(CL_ZERO_IN) | M(CL_DENORM_OUT));
TRANSCENDENTAL(CaseErfinv, erfinv_, erfinvf_, nullptr, false, kFloatIn | M(CL_NAN_OUT));
TRANSCENDENTAL(CaseAcos, acos_, acos_, nullptr, false, kFloatIn | M(CL_NAN_OUT));
struct CaseCos : CaseBase {
    static constexpr uint64_t N_CPU = 1ull << 26;
    static constexpr uint32_t CLASSES = M(CL_DENORM_IN) | M(CL_ZERO_IN);
    static const char *exclusion() { return kExclOctant; }
    static bool excluded(const In &in) { return octant_conversion_out_of_range(in.v[0]); }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(cos_(u2f(in.v[0]))); }
    static void ref(const In &in, Out &o) { if (g_cpu) { need_oracle(); float s, c; g_orc.sincos_(hf(in.v[0]), &s, &c); o.v[0] = hu(c); } else fut(in, o); }
};
struct CaseSincos : CaseCos {
    static constexpr int NOUT = 2;
    DTOF_HD static void fut(const In &in, Out &o) { float s, c; sincos_(u2f(in.v[0]), s, c); o.v[0] = f2u(s); o.v[1] = f2u(c); }
    static void ref(const In &in, Out &o) { if (g_cpu) { need_oracle(); float s, c; g_orc.sincos_(hf(in.v[0]), &s, &c); o.v[0] = hu(s); o.v[1] = hu(c); } else fut(in, o); }
};
// atan2_(y, x) on 2^32 pairs.  kinds: 0 every combination of 16 special values (signs, zeros, denormals, infinities, NaNs, extremes) in both operands; 1 |y| = |x|;
// 2 |y| within two ulps of |x| (the octant boundary); 3 one operand zero, denormal or tiny against a random other (the axes); 4-7 random bit patterns
struct CaseAtan2 : CaseBase {
    static constexpr int KINDS = 8, NIN = 2;
    static constexpr uint64_t N_CPU = 1ull << 26;
    static constexpr uint32_t CLASSES = kFloatIn | M(CL_NAN_OUT) | M(CL_DENORM_OUT);
    DTOF_HD static void gen(uint64_t i, uint64_t n, uint64_t seed, In &in) {
        const uint64_t h = mix64(i, seed), h2 = mix64(h, 17);
        const uint32_t kind = kind_of(i, n, 8);
        uint32_t y = (uint32_t) h, x = (uint32_t) h2;
        if (kind == 0) { y = special_bits((uint32_t) i); x = special_bits((uint32_t) (i >> 4)); }
        else if (kind == 1) x = (y & 0x7fffffffu) | (x & 0x80000000u);
        else if (kind == 2) { y = rand_normal(h, -100, 100); x = ulp_step(y & 0x7fffffffu, (int) ((h2 >> 40) % 5) - 2) | (x & 0x80000000u); }
        else if (kind == 3) { const uint32_t tiny = (h2 >> 40 & 1) ? (uint32_t) (h2 >> 8) & 0x807fffffu : special_bits((uint32_t) (h2 >> 8)); if (h2 >> 41 & 1) y = tiny; else x = tiny; }
        in.v[0] = y; in.v[1] = x;
    }
    DTOF_HD static void fut(const In &in, Out &o) { o.v[0] = f2u(atan2_(u2f(in.v[0]), u2f(in.v[1]))); }
    static void ref(const In &in, Out &o) { if (g_cpu) { need_oracle(); o.v[0] = hu(g_orc.atan2f_(hf(in.v[0]), hf(in.v[1]))); } else fut(in, o); }
};
// the device's f64 division and square root against the host's on 2^24 inputs (what a device-side double reference would rest on)
struct CaseF64DivSqrt : CaseBase {
    static constexpr int NOUT = 3, NIN = 4;
    static constexpr bool FLOAT_IN = false, FLOAT_OUT = false;
    static constexpr uint64_t N_GPU = 1ull << 24, N_CPU = 1ull << 24;
    DTOF_HD static double d_of(uint32_t lo, uint32_t hi) { const uint64_t u = (uint64_t) lo | (uint64_t) hi << 32; double d; __builtin_memcpy(&d, &u, 8); return d; }
    DTOF_HD static void gen(uint64_t i, uint64_t, uint64_t seed, In &in) {   // half random bit patterns, half floats widened (the operands a float reference would feed)
        const uint64_t h = mix64(i, seed), h2 = mix64(h, 17);
        uint64_t a = h, b = h2;
        if (i & 1) { const double da = (double) u2f((uint32_t) h), db = (double) u2f((uint32_t) h2); __builtin_memcpy(&a, &da, 8); __builtin_memcpy(&b, &db, 8); }
        in.v[0] = (uint32_t) a; in.v[1] = (uint32_t) (a >> 32); in.v[2] = (uint32_t) b; in.v[3] = (uint32_t) (b >> 32);
    }
    DTOF_HD static void fut(const In &in, Out &o) {   // the quotient and the root rounded once to float, and the low word of the double quotient
        const double a = d_of(in.v[0], in.v[1]), b = d_of(in.v[2], in.v[3]), q = a / b;
        uint64_t qu; __builtin_memcpy(&qu, &q, 8);
        const float qf = (float) q, rf = (float) sqrt(a);   // NaNs in canonical form: the comparison of this case is by integer
        o.v[0] = qf == qf ? f2u(qf) : 0x7fc00000u; o.v[1] = rf == rf ? f2u(rf) : 0x7fc00000u; o.v[2] = q == q ? (uint32_t) qu : 0u;
    }
    static void ref(const In &in, Out &o) { fut(in, o); }   // host compilation: x86 IEEE double
};

// ---------------------------------------------------------------------------------------------------------------- generic runner
template <class C, bool CAND>
__global__ void __launch_bounds__(256) k_sweep(uint64_t base, uint32_t n, uint64_t total, uint64_t seed, uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    In in = {}; Out o = {};
    C::gen(base + j, total, seed, in);
    if constexpr (CAND) C::cand(in, o); else C::fut(in, o);
#pragma unroll
    for (int k = 0; k < C::NOUT; ++k) out[(size_t) k * n + j] = o.v[k];
    if (C::CHECK_GEN) out[(size_t) C::NOUT * n + j] = in_checksum(in);
}

static int host_threads() {
    int t = 0;
    if (const char *e = getenv("OMP_NUM_THREADS")) t = atoi(e);
    if (t <= 0) t = (int) std::thread::hardware_concurrency();
    return std::max(1, std::min(16, t));
}
static inline int exp_of(uint32_t u) { return (int) (u >> 23 & 255) - 127; }

template <class C>
static void host_range(uint64_t lo, uint64_t hi, uint64_t chunk_base, uint32_t chunk_n, uint64_t total, uint64_t seed, const uint32_t *dev, Tally &t) {
    for (uint64_t i = lo; i < hi; ++i) {
        In in = {}; Out got = {}, ref = {};
        C::gen(i, total, seed, in);
        if (dev) {
            const size_t j = (size_t) (i - chunk_base);
            for (int k = 0; k < C::NOUT; ++k) got.v[k] = dev[(size_t) k * chunk_n + j];
            if (C::CHECK_GEN && dev[(size_t) C::NOUT * chunk_n + j] != in_checksum(in)) { ++t.gen_mismatches; continue; }
        } else C::fut(in, got);
        ++t.inputs;
        C::ref(in, ref);
        bool same = true;
        for (int k = 0; k < C::NOUT; ++k) same = same && (C::FLOAT_OUT ? same_bits(got.v[k], ref.v[k]) : got.v[k] == ref.v[k]);
        if (C::excluded(in)) { ++t.excluded; t.excluded_mismatches += !same; continue; }
        const uint32_t kind = C::KINDS > 1 ? kind_of(i, total, C::KINDS) : 0;
        ++t.kind_n[kind];
        if (C::FLOAT_IN) {
            bool den = false, nan = false, inf = false, zero = false, fin = true;
            for (int k = 0; k < C::NIN; ++k) {
                const uint32_t u = in.v[k];
                den |= is_den_bits(u); nan |= is_nan_bits(u); inf |= is_inf_bits(u); zero |= (u << 1) == 0; fin &= (u & 0x7f800000u) != 0x7f800000u;
            }
            t.cls[CL_DENORM_IN] += den; t.cls[CL_NAN_IN] += nan; t.cls[CL_INF_IN] += inf; t.cls[CL_ZERO_IN] += zero;
            if (C::FLOAT_OUT) for (int k = 0; k < C::NOUT; ++k) { t.cls[CL_OVERFLOW] += fin && is_inf_bits(ref.v[k]); t.cls[CL_NAN_OUT] += !nan && is_nan_bits(ref.v[k]); }
        }
        if (C::FLOAT_OUT) for (int k = 0; k < C::NOUT; ++k) t.cls[CL_DENORM_OUT] += is_den_bits(ref.v[k]);
        const int rc = C::rounding(in, ref);
        if (rc >= 0) ++t.cls[rc];
        if (g_candidate) {   // operand classes of the candidate slot (two float operands, one result)
            const uint32_t a = in.v[0], b = in.v[1], q = ref.v[0];
            const bool special = (a & 0x7f800000u) == 0x7f800000u || (b & 0x7f800000u) == 0x7f800000u || (a << 1) == 0 || (b << 1) == 0;
            const int eq = exp_of(q);
            const int oc = special ? 4 : (is_den_bits(a) || is_den_bits(b)) ? 1 : (is_den_bits(q) || (q << 1) == 0) ? 2 : (eq >= 126 || eq <= -125) ? 3 : 0;
            ++t.cand[oc][0]; t.cand[oc][1] += !same;
#ifdef DTOF_SWEEP_CANDIDATE
            if (!special && !is_den_bits(a) && !is_den_bits(b)) {
                const int ea = exp_of(a), eb = exp_of(b), v = div_unscaled_violations(ea, eb);
                if (v == 0) { ++t.safe[0]; t.safe[1] += !same; }
                for (int k = 0; k < 5; ++k) if (v == (1 << k)) {
                    const int e = k < 2 ? eb : k == 2 ? ea : ea - eb;
                    ++t.only[k][0]; t.only[k][1] += !same;
                    if (!same) { t.only_exp[k][0] = std::min(t.only_exp[k][0], e); t.only_exp[k][1] = std::max(t.only_exp[k][1], e); }
                }
            }
#endif
        }
        if (!same) { ++t.mismatches; ++t.kind_bad[kind]; Mismatch m; m.index = i; m.in = in; m.got = got; m.ref = ref; t.note(m); }
    }
}

template <class C>
static void compare_chunk(uint64_t base, uint32_t n, uint64_t total, uint64_t seed, const uint32_t *dev, Tally &tally, int threads) {
    std::vector<Tally> part((size_t) threads);
    std::vector<std::thread> pool;
    const uint64_t per = (n + (uint64_t) threads - 1) / (uint64_t) threads;
    for (int k = 0; k < threads; ++k) {
        const uint64_t lo = base + std::min<uint64_t>(n, per * (uint64_t) k), hi = base + std::min<uint64_t>(n, per * (uint64_t) (k + 1));
        pool.emplace_back([=, &part] { host_range<C>(lo, hi, base, n, total, seed, dev, part[(size_t) k]); });
    }
    for (std::thread &th : pool) th.join();
    for (const Tally &p : part) tally.merge(p);
}

struct Options { uint64_t seed = 1; std::vector<uint32_t> extra; };

template <class C, bool CAND>
static void launch_chunk(uint64_t base, uint32_t n, uint64_t total, uint64_t seed, uint32_t *d_out, uint32_t *h_out, hipStream_t s) {
    hipLaunchKernelGGL((k_sweep<C, CAND>), dim3((n + 255u) / 256u), dim3(256), 0, s, base, n, total, seed, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h_out, d_out, (size_t) (C::NOUT + (C::CHECK_GEN ? 1 : 0)) * n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
}

template <class C>
static void run_case(const char *name, const Options &opt, Tally &tally, uint64_t &total) {
    const int threads = host_threads();
    total = g_cpu ? C::N_CPU : C::N_GPU;
    if (g_cpu) {
        for (uint64_t base = 0; base < total; base += kChunk) compare_chunk<C>(base, (uint32_t) std::min<uint64_t>(kChunk, total - base), total, opt.seed, nullptr, tally, threads);
        return;
    }
    if (g_candidate && !C::HAS_CAND) { fprintf(stderr, "math_sweep: case %s carries no candidate (or the build lacks -DDTOF_SWEEP_CANDIDATE)\n", name); exit(2); }
    hipStream_t s; HIP_OK(hipStreamCreate(&s));
    uint32_t *d_out[2], *h_out[2];
    const size_t bytes = (size_t) kMaxWords * kChunk * sizeof(uint32_t);
    for (int k = 0; k < 2; ++k) { HIP_OK(hipMalloc((void **) &d_out[k], bytes)); HIP_OK(hipHostMalloc((void **) &h_out[k], bytes, hipHostMallocDefault)); }
    auto launch = [&](uint64_t base, int buf) {
        const uint32_t n = (uint32_t) std::min<uint64_t>(kChunk, total - base);
        if constexpr (C::HAS_CAND) { if (g_candidate) { launch_chunk<C, true>(base, n, total, opt.seed, d_out[buf], h_out[buf], s); return; } }
        launch_chunk<C, false>(base, n, total, opt.seed, d_out[buf], h_out[buf], s);
    };
    launch(0, 0);
    int buf = 0;
    for (uint64_t base = 0; base < total; base += kChunk, buf ^= 1) {
        HIP_OK(hipStreamSynchronize(s));                       // chunk `base` is in h_out[buf]
        if (base + kChunk < total) launch(base + kChunk, buf ^ 1);
        compare_chunk<C>(base, (uint32_t) std::min<uint64_t>(kChunk, total - base), total, opt.seed, h_out[buf], tally, threads);
    }
    for (int k = 0; k < 2; ++k) { HIP_OK(hipFree(d_out[k])); HIP_OK(hipHostFree(h_out[k])); }
    HIP_OK(hipStreamDestroy(s));
}

template <class C>
static int case_main(const char *name, const Options &opt) {
    const auto t0 = std::chrono::steady_clock::now();
    Tally t; uint64_t total = 0;
    run_case<C>(name, opt, t, total);
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("case %s\nmode %s\nthreads %d\n", name, g_cpu ? "cpu" : g_candidate ? "candidate" : "gpu", host_threads());
    printf("inputs %llu\n", (unsigned long long) t.inputs);
    printf("compared %llu\n", (unsigned long long) (t.inputs - t.excluded));
    printf("mismatches %llu\n", (unsigned long long) t.mismatches);
    printf("gen_mismatches %llu\n", (unsigned long long) t.gen_mismatches);
    printf("excluded %llu\nexcluded_mismatches %llu\n", (unsigned long long) t.excluded, (unsigned long long) t.excluded_mismatches);
    if (C::exclusion()) printf("# exclusion: %s\n", C::exclusion());
    for (int k = 0; k < CL_COUNT; ++k) if (C::CLASSES & M(k)) printf("class_%s %llu\n", kClassName[k], (unsigned long long) t.cls[k]);
    if (C::KINDS > 1) for (int k = 0; k < C::KINDS; ++k) printf("kind%d %llu %llu\n", k, (unsigned long long) t.kind_n[k], (unsigned long long) t.kind_bad[k]);
    for (const Mismatch &m : t.first) {
        printf("mismatch index %llu operands", (unsigned long long) m.index);
        for (int k = 0; k < C::NIN; ++k) printf(" 0x%08x", m.in.v[k]);
        if (C::FLOAT_IN) { printf(" ("); for (int k = 0; k < C::NIN; ++k) printf("%s%a", k ? ", " : "", hf(m.in.v[k])); printf(")"); }
        printf(" got"); for (int k = 0; k < C::NOUT; ++k) printf(" 0x%08x", m.got.v[k]);
        printf(" reference"); for (int k = 0; k < C::NOUT; ++k) printf(" 0x%08x", m.ref.v[k]);
        printf("\n");
    }
    if (g_candidate) {
        static const char *oc[5] = { "normal", "denormal_operand", "denormal_result", "near_overflow_or_underflow", "special" };
        for (int k = 0; k < 5; ++k) printf("cand_%s %llu %llu\n", oc[k], (unsigned long long) t.cand[k][0], (unsigned long long) t.cand[k][1]);
        printf("cand_safe_window %llu %llu\n", (unsigned long long) t.safe[0], (unsigned long long) t.safe[1]);
        static const char *on[5] = { "b_above_125", "b_below_m125", "a_below_m100", "a_minus_b_below_m100", "a_minus_b_above_125" };
        for (int k = 0; k < 5; ++k) printf("cand_only_%s %llu %llu %d %d\n", on[k], (unsigned long long) t.only[k][0], (unsigned long long) t.only[k][1], t.only_exp[k][0], t.only_exp[k][1]);
    }
    printf("wall_s %.2f\n", wall);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- fdiv: integer work, compared on the device
// q = fdiv(n, make_fastdiv(d)) is n / d exactly when q d <= n < (q + 1) d (64-bit products: the definition, no division involved)
DTOF_HD bool fdiv_is_quotient(uint32_t n, uint32_t d, uint32_t q) { const uint64_t p = (uint64_t) q * d; return p <= n && n - p < d; }
__global__ void __launch_bounds__(256) k_fdiv(FastDiv f, uint32_t d, uint32_t slot, unsigned long long *__restrict__ bad, unsigned long long *__restrict__ multiples, uint32_t *__restrict__ first_bad) {
    __shared__ unsigned int s_bad, s_mult, s_first;
    if (threadIdx.x == 0) { s_bad = 0; s_mult = 0; s_first = 0xffffffffu; }
    __syncthreads();
    unsigned int my_bad = 0, my_mult = 0, my_first = 0xffffffffu;
    const uint32_t stride = gridDim.x * 256u;                         // the launch makes stride divide 2^32
    uint32_t n = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t it = 0, its = (uint32_t) ((1ull << 32) / stride); it < its; ++it, n += stride) {
        const uint32_t q = fdiv(n, f);
        const bool ok = fdiv_is_quotient(n, d, q);
        if (!ok) { ++my_bad; my_first = n < my_first ? n : my_first; }
        my_mult += q * d == n;
    }
    if (my_bad) { atomicAdd(&s_bad, my_bad); atomicMin(&s_first, my_first); }
    atomicAdd(&s_mult, my_mult);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&multiples[slot], (unsigned long long) s_mult);
        if (s_bad) { atomicAdd(&bad[slot], (unsigned long long) s_bad); atomicMin(&first_bad[slot], s_first); }
    }
}
static const uint32_t kPrimes[] = { 4099u, 4999u, 7919u, 10007u, 65521u, 65537u, 99991u, 1000003u, 16777213u, 16777259u, 100000007u, 1000000007u,
                                    2147483629u, 2147483647u, 2147483659u, 3000000019u, 4294967279u, 4294967291u };
static std::vector<uint32_t> fdiv_divisors(const Options &opt) {
    std::vector<uint32_t> d;
    for (uint32_t k = 1; k <= 4096; ++k) d.push_back(k);
    for (uint32_t k = 1; k <= 31; ++k) { d.push_back((1u << k) - 1); d.push_back(1u << k); d.push_back((1u << k) + 1); }
    d.push_back(0xffffffffu);
    for (uint32_t p : kPrimes) d.push_back(p);
    for (uint32_t e : opt.extra) if (e) d.push_back(e);               // the divisors of the committed configurations (the test computes them)
    std::sort(d.begin(), d.end()); d.erase(std::unique(d.begin(), d.end()), d.end());
    return d;
}
static int fdiv_main(const Options &opt) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<uint32_t> divs = fdiv_divisors(opt);
    const size_t nd = divs.size();
    std::vector<unsigned long long> bad(nd, 0), mult(nd, 0);
    std::vector<uint32_t> first(nd, 0xffffffffu);
    uint64_t inputs = 0;
    if (g_cpu) {   // per divisor 2^16 values of n: the ends, multiples of d and their neighbours, and a stride through the rest
        const int threads = host_threads();
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t) pool.emplace_back([&, t] {
            for (size_t s = (size_t) t; s < nd; s += (size_t) threads) {
                const uint32_t d = divs[s]; const FastDiv f = make_fastdiv(d);
                for (uint32_t k = 0; k < 65536u; ++k) {
                    const uint64_t h = mix64(k, d);
                    const uint32_t n = k < 8 ? (k < 4 ? k : 0xfffffffbu + k) : (k & 3) == 0 ? k * 65521u + (uint32_t) h % 65521u
                                                                             : (uint32_t) ((h >> 20) % ((0xffffffffull / d) + 1)) * d + ((k & 3) - 2u);
                    const uint32_t q = fdiv(n, f);
                    if (!fdiv_is_quotient(n, d, q) || q != n / d) { ++bad[s]; first[s] = std::min(first[s], n); }
                    mult[s] += q * d == n;
                }
            }
        });
        for (std::thread &th : pool) th.join();
        inputs = (uint64_t) nd * 65536u;
    } else {
        unsigned long long *d_bad, *d_mult; uint32_t *d_first;
        HIP_OK(hipMalloc((void **) &d_bad, nd * 8)); HIP_OK(hipMalloc((void **) &d_mult, nd * 8)); HIP_OK(hipMalloc((void **) &d_first, nd * 4));
        HIP_OK(hipMemset(d_bad, 0, nd * 8)); HIP_OK(hipMemset(d_mult, 0, nd * 8)); HIP_OK(hipMemset(d_first, 0xff, nd * 4));
        for (size_t s = 0; s < nd; ++s) {
            hipLaunchKernelGGL(k_fdiv, dim3(4096), dim3(256), 0, 0, make_fastdiv(divs[s]), divs[s], (uint32_t) s, d_bad, d_mult, d_first);
            HIP_OK(hipGetLastError());
            if ((s & 255) == 255) HIP_OK(hipDeviceSynchronize());
        }
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(bad.data(), d_bad, nd * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(mult.data(), d_mult, nd * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(first.data(), d_first, nd * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_bad)); HIP_OK(hipFree(d_mult)); HIP_OK(hipFree(d_first));
        inputs = (uint64_t) nd << 32;
    }
    unsigned long long mismatches = 0, multiples = 0; int shown = 0;
    printf("case fdiv\nmode %s\ndivisors %zu\ninputs %llu\n", g_cpu ? "cpu" : "gpu", nd, (unsigned long long) inputs);
    for (size_t s = 0; s < nd; ++s) { mismatches += bad[s]; multiples += mult[s]; }
    printf("mismatches %llu\nclass_multiples %llu\n", mismatches, multiples);
    for (size_t s = 0; s < nd && shown < 8; ++s) if (bad[s]) {
        const uint32_t n = first[s], d = divs[s];
        printf("mismatch divisor %u first_n %u got %u reference %u count %llu\n", d, n, fdiv(n, make_fastdiv(d)), n / d, bad[s]); ++shown;
    }
    printf("wall_s %.2f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- permute_kensler
__global__ void __launch_bounds__(256) k_permute(uint32_t n, FastDiv dn, uint32_t total, uint32_t *__restrict__ out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= total) return;                                            // total = 64 n <= 2^24
    const uint32_t s = j / n, i = j - s * n;
    out[j] = permute_kensler(i, n, (uint32_t) mix64(s, n), dn);
}
static int permute_main() {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> ns;
    for (uint32_t n = 1; n <= 257; ++n) ns.push_back(n);
    ns.push_back(1000); ns.push_back(4096); ns.push_back(65537);
    uint32_t *d_out = nullptr; std::vector<uint32_t> got((size_t) 64 * 65537), seen;
    if (!g_cpu) HIP_OK(hipMalloc((void **) &d_out, got.size() * 4));
    unsigned long long inputs = 0, mismatches = 0, not_permutation = 0, moved = 0; int shown = 0;
    printf("case permute_kensler\nmode %s\n", g_cpu ? "cpu" : "gpu");
    for (uint32_t n : ns) {
        const uint32_t total = 64 * n; const FastDiv dn = make_fastdiv(n);
        if (!g_cpu) {
            hipLaunchKernelGGL(k_permute, dim3((total + 255u) / 256u), dim3(256), 0, 0, n, dn, total, d_out);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpy(got.data(), d_out, (size_t) total * 4, hipMemcpyDeviceToHost));
        }
        for (uint32_t s = 0; s < 64; ++s) {
            seen.assign(n, 0);
            const uint32_t seed = (uint32_t) mix64(s, n);
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t ref = permute_kensler(i, n, seed, dn), g = g_cpu ? ref : got[(size_t) s * n + i];
                ++inputs; moved += g != i;
                if (g != ref) { ++mismatches; if (shown++ < 8) printf("mismatch n %u seed 0x%08x index %u got %u reference %u\n", n, seed, i, g, ref); }
                if (g >= n || seen[g]++) { ++not_permutation; if (shown++ < 8) printf("mismatch n %u seed 0x%08x index %u value %u is out of range or repeated\n", n, seed, i, g); }
            }
        }
    }
    if (d_out) HIP_OK(hipFree(d_out));
    printf("sizes %zu\ninputs %llu\nmismatches %llu\nnot_permutation %llu\nclass_moved %llu\n", ns.size(), inputs, mismatches, not_permutation, moved);
    printf("wall_s %.2f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- accuracy: host (and oracle) against float64
static double ulp_of(double ref) { int e; frexp(ref, &e); return ldexp(1.0, std::max(e - 24, -149)); }
static double erfinv_f64(double x, double start) {   // Newton on erf, from the float result
    double y = start;
    for (int k = 0; k < 4; ++k) y -= (erf(y) - x) / (1.1283791670955126 * exp(-y * y));
    return y;
}
struct Acc { double ulp = 0, abs = 0; float at_ulp = 0, at_abs = 0; };
static void acc_add(Acc &a, float x, float got, double ref) {
    const double e = fabs((double) got - ref), u = e / ulp_of(ref);
    if (e > a.abs) { a.abs = e; a.at_abs = x; }
    if (u > a.ulp) { a.ulp = u; a.at_ulp = x; }
}
static void acc_print(const char *fn, const char *what, float lo, float hi, uint64_t n, const Acc &d, const Acc &o) {
    printf("acc %s %s %.9g %.9g %llu dtof_ulp %.3f dtof_abs %.4g orc_ulp %.3f orc_abs %.4g worst_x %a %a\n", fn, what, lo, hi, (unsigned long long) n, d.ulp, d.abs, o.ulp, o.abs, d.at_ulp, d.at_abs);
}
template <class F, class G, class R>
static void acc_unary(const char *fn, const char *what, float lo, float hi, F dtof_fn, G orc_fn, R ref_fn) {
    // every float of [lo, hi] when there are at most 2^24 of them on each side of zero, else an even stride through their bit patterns
    Acc d, o; uint64_t n = 0;
    auto side = [&](float a, float b, uint32_t sign) {   // 0 <= a <= b
        const uint32_t ua = hu(a), ub = hu(b), step = std::max(1u, (ub - ua) >> 24);
        for (uint64_t u = ua; u <= ub; u += step) { const float x = hf((uint32_t) u | sign); const double r = ref_fn((double) x, dtof_fn(x)); acc_add(d, x, dtof_fn(x), r); acc_add(o, x, orc_fn(x), r); ++n; }
    };
    if (lo < 0.f) side(hi < 0.f ? -hi : 0.f, -lo, 0x80000000u);
    if (hi >= 0.f) side(lo > 0.f ? lo : 0.f, hi, 0u);
    acc_print(fn, what, lo, hi, n, d, o);
}
static int accuracy_main() {
    need_oracle();
    auto orc_sin = [](float x) { float s, c; g_orc.sincos_(x, &s, &c); return s; };
    auto orc_cos = [](float x) { float s, c; g_orc.sincos_(x, &s, &c); return c; };
    auto my_sin = [](float x) { float s, c; sincos_(x, s, c); return s; };
    const float two_pi = 2.f * kPi;
    acc_unary("exp_", "normal_results", -87.3f, 88.72f, [](float x) { return exp_(x); }, g_orc.expf_, [](double x, float) { return exp(x); });
    acc_unary("log_", "normal_arguments", 1.17549435e-38f, 3.40282347e+38f, [](float x) { return log_(x); }, g_orc.logf_, [](double x, float) { return log(x); });
    acc_unary("tan_", "one_turn", 0.f, two_pi, [](float x) { return tan_(x); }, g_orc.tanf_, [](double x, float) { return tan(x); });
    acc_unary("tan_", "pm20", -20.f, 20.f, [](float x) { return tan_(x); }, g_orc.tanf_, [](double x, float) { return tan(x); });
    acc_unary("sin_", "pm20", -20.f, 20.f, my_sin, orc_sin, [](double x, float) { return sin(x); });
    acc_unary("cos_", "pm20", -20.f, 20.f, [](float x) { return cos_(x); }, orc_cos, [](double x, float) { return cos(x); });
    acc_unary("sin_", "one_turn", 0.f, two_pi, my_sin, orc_sin, [](double x, float) { return sin(x); });
    acc_unary("cos_", "one_turn", 0.f, two_pi, [](float x) { return cos_(x); }, orc_cos, [](double x, float) { return cos(x); });
    acc_unary("acos_", "domain", -1.f, 1.f, [](float x) { return acos_(x); }, g_orc.acos_, [](double x, float) { return acos(x); });
    acc_unary("erf_", "series", -0.99999994f, 0.99999994f, [](float x) { return erf_(x); }, g_orc.erff_, [](double x, float) { return erf(x); });
    acc_unary("erf_", "tail", 1.f, 6.f, [](float x) { return erf_(x); }, g_orc.erff_, [](double x, float) { return erf(x); });
    acc_unary("erfinv_", "open_interval", -0.999999f, 0.999999f, [](float x) { return erfinv_(x); }, g_orc.erfinvf_, [](double x, float start) { return erfinv_f64(x, (double) start); });
    {   // atan2_: 2^24 random directions, every quadrant, ratios log-uniform over 2^-40 .. 2^40
        Acc d, o; const uint64_t n = 1ull << 24;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t h = mix64(i, 3);
            const float y = hf(rand_normal(h, -20, 20)), x = hf(rand_normal(mix64(h, 17), -20, 20));
            const double r = atan2((double) y, (double) x);
            acc_add(d, y, atan2_(y, x), r); acc_add(o, y, g_orc.atan2f_(y, x), r);
        }
        acc_print("atan2_", "random_directions", -1.f, 1.f, n, d, o);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the table
struct Entry { const char *name; int (*run)(const char *, const Options &); };
#define GENERIC(NAME, TYPE) { NAME, [](const char *n, const Options &o) { return case_main<TYPE>(n, o); } }
static const Entry kCases[] = {
    GENERIC("rcp", CaseRcp), GENERIC("sqrtf", CaseSqrt), GENERIC("rsqrt_", CaseRsqrt), GENERIC("safe_sqrt", CaseSafeSqrt), GENERIC("signf", CaseSignf),
    GENERIC("truncf", CaseTrunc), GENERIC("floorf", CaseFloor), GENERIC("float_to_int32", CaseF2I), GENERIC("int32_to_float", CaseI2F), GENERIC("uint32_to_float", CaseU2F),
    GENERIC("div", CaseDiv), GENERIC("fmaf", CaseFma), GENERIC("lerp_", CaseLerp), GENERIC("dot", CaseDot), GENERIC("cross", CaseCross),
    GENERIC("fmod_pos_2pi", CaseFmod2Pi), GENERIC("fmod_pos_xy", CaseFmodXY),
    { "fdiv", [](const char *, const Options &o) { return fdiv_main(o); } },
    GENERIC("pcg_jump6", CasePcgJump6), GENERIC("pcg_output_f32", CasePcgOutput),
    { "permute_kensler", [](const char *, const Options &) { return permute_main(); } },
    GENERIC("mulsign", CaseMulsign), GENERIC("mulsign_neg", CaseMulsignNeg),
    GENERIC("exp_", CaseExp), GENERIC("log_", CaseLog), GENERIC("tan_", CaseTan), GENERIC("erf_", CaseErf), GENERIC("erfinv_", CaseErfinv), GENERIC("acos_", CaseAcos),
    GENERIC("cos_", CaseCos), GENERIC("sincos_", CaseSincos), GENERIC("atan2_", CaseAtan2), GENERIC("f64_div_sqrt", CaseF64DivSqrt),
};

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: math_sweep list | accuracy --oracle LIB | <case> [--cpu] [--oracle LIB] [--seed S] [--extra d1,d2,...] [--candidate]\n"); return 2; }
    Options opt;
    for (int k = 2; k < argc; ++k) {
        const std::string a = argv[k];
        if (a == "--cpu") g_cpu = true;
        else if (a == "--candidate") g_candidate = true;
        else if (a == "--oracle" && k + 1 < argc) load_oracle(argv[++k]);
        else if (a == "--seed" && k + 1 < argc) opt.seed = strtoull(argv[++k], nullptr, 0);
        else if (a == "--extra" && k + 1 < argc) { for (char *p = strtok(argv[++k], ","); p; p = strtok(nullptr, ",")) opt.extra.push_back((uint32_t) strtoul(p, nullptr, 0)); }
        else { fprintf(stderr, "math_sweep: unknown argument %s\n", a.c_str()); return 2; }
    }
    const std::string name = argv[1];
    if (name == "list") { for (const Entry &e : kCases) printf("%s\n", e.name); return 0; }
    if (name == "accuracy") { g_cpu = true; return accuracy_main(); }
    if (g_cpu && g_candidate) { fprintf(stderr, "math_sweep: a candidate uses device builtins and runs on the device only\n"); return 2; }
    for (const Entry &e : kCases) if (name == e.name) { const int r = e.run(e.name, opt); fflush(stdout); return r; }
    fprintf(stderr, "math_sweep: no case named %s\n", name.c_str());
    return 2;
}
