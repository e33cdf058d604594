// dtof_render.hip -- host orchestration of the wavefront renderer and the C ABI (include/dtof.h).
//
// Replaces, for the `dopplertofpath` + `correlated` path only, SamplingIntegrator::render
// (src/render/integrator.cpp:104-347, JIT branch :226-340): wavefront set-up, sampler seeding,
// lane->pixel mapping, the bounce loop and the film develop.  One host thread drives one HIP
// stream; the wavefront of W*H*spp lanes is cut into row-band batches (results are invariant to
// the cut because every lane's RNG streams are pure functions of its global lane index,
// sampler.cpp:115-134 / correlated.cpp:38-64).
#include "../../include/dtof.h"
#include "dtof_kernels.h"
#include "dtof_reconstruct.h"
#include "dtof_denoise.h"
#include "dtof_film64.h"
#include "dtof_moments.h"
#include "dtof_aov.h"
#include "dtof_flat_query.h"
#include "dtof_pair_setup.h"
#include "dtof_tree_query.h"
#include "dtof_scene.h"
#include "dtof_math.h"
#include <atomic>
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <string>
#include <memory>
#include <vector>

using namespace dtof;

namespace {

thread_local std::string g_last_error;

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
#define HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

template <typename F> int guarded(F &&f) {
    try { f(); return DTOF_OK; }
    catch (const HipError &e) { g_last_error = e.what(); return DTOF_ERR_HIP; }
    catch (const std::exception &e) { g_last_error = e.what(); return DTOF_ERR_INVALID; }
    catch (...) { g_last_error = "unknown error"; return DTOF_ERR_INVALID; }
}

template <typename T> struct DevBuf {
    T *p = nullptr; size_t n = 0;
    void ensure(size_t count) {
        if (count <= n) return;
        release();
        HIP_CHECK(hipMalloc((void **) &p, count * sizeof(T))); n = count;
    }
    void release() { if (p) { (void) hipFree(p); p = nullptr; n = 0; } }
    ~DevBuf() { release(); }
};

// per-iteration count slots of a batch (statistics + the queue counts of the previous iteration); reused cyclically beyond that.
// DTOF_STAT_SLOTS shrinks it so that the tests can exercise the wrap-around with short paths.
static const uint32_t kMaxIter = [] { const char *e = getenv("DTOF_STAT_SLOTS"); int v = e ? atoi(e) : 0; return (uint32_t) (v >= 2 ? v : 256); }();
// the stages a frame's launches are timed by (StageTimer, dtof_render_stats) and named after (roctx ranges)
enum Stage { kStageGenerate, kStageTrace, kStageShade, kStageShadow, kStageSplat, kStageFirst, kStageCount };

struct Workspace {
    DevBuf<float4> ray_a, ray_b, st_a, st_b, res, sh_a, sh_b, sh_c;
    DevBuf<uint4> hit, rng_a;
    DevBuf<uint32_t> hit_id, q0, q1, counts;
    DevBuf<float> hit_t;
    DevBuf<float2> pos, st_c;
    DevBuf<uint2> rng_b;
    DevBuf<LaneDebug> dbg;
    DevBuf<float4> valid;   // Queues::valid_out
    DevBuf<uint4> cand; DevBuf<uint32_t> defer_idx, defer_cnt;   // Queues::cand / defer_idx / defer_cnt
    uint32_t capacity = 0; int k = 0;
    void ensure(uint32_t cap, int n_offsets) {
        if (cap <= capacity && n_offsets <= k) return;
        capacity = std::max(cap, capacity); k = std::max(n_offsets, k);
        ray_a.ensure(capacity); ray_b.ensure(capacity); st_a.ensure(capacity); st_b.ensure(capacity);
        res.ensure((size_t) capacity * k); sh_a.ensure(capacity); sh_b.ensure(capacity); sh_c.ensure((size_t) capacity * k);
        hit.ensure(capacity); hit_t.ensure(capacity); rng_a.ensure(capacity); hit_id.ensure(capacity); q0.ensure(capacity); q1.ensure(capacity);
        counts.ensure(2 * (size_t) kMaxIter * segments_for(capacity) + 16); pos.ensure(capacity); rng_b.ensure(capacity); st_c.ensure(capacity);   // + the segment counter of the resident kernel
    }
    // the queues of a batch of up to `cap` lanes; valid_out only when asked for, the DEFER lists only for frames whose ray kernels run as a pair of launches
    Queues prepare(uint32_t cap, int n_offsets, bool want_valid, bool defer, uint32_t id_shift) {
        ensure(cap, n_offsets);
        if (want_valid) valid.ensure(capacity);
        if (defer) { cand.ensure(capacity); defer_idx.ensure(capacity); defer_cnt.ensure(segments_for(capacity)); }
        Queues q; memset(&q, 0, sizeof q);
        q.ray_a = ray_a.p; q.ray_b = ray_b.p; q.hit = hit.p; q.hit_t = hit_t.p; q.hit_id = hit_id.p; q.st_a = st_a.p; q.st_b = st_b.p; q.rng_a = rng_a.p; q.rng_b = rng_b.p; q.st_c = st_c.p;
        q.res = res.p; q.pos = pos.p; q.sh_a = sh_a.p; q.sh_b = sh_b.p; q.sh_c = sh_c.p; q.q[0] = q0.p; q.q[1] = q1.p;
        q.counts = counts.p; q.capacity = capacity; q.valid_out = valid.p;
        q.seg_counter = counts.p + 2 * (size_t) kMaxIter * segments_for(capacity);
        if (defer) { q.cand = cand.p; q.defer_idx = defer_idx.p; q.defer_cnt = defer_cnt.p; }
        q.id_shift = id_shift;
        return q;
    }
};

}  // namespace

struct dtof_scene {
    HostScene host;
    PluginParams pp;
    std::vector<uint8_t> blob;
    DevBuf<uint8_t> d_blob; bool uploaded = false;
    Workspace ws;
    DevBuf<float> d_film, d_rgb;
    DevBuf<double> d_film64;   // the library's own float64 film (dtof_render_variants_f64, dtof_render_velocity_map_f64)
    DevBuf<double> d_moments, d_moment_planes;   // the moment film (dtof_render_moments) or the aov film (dtof_render_aovs) of the call: cells of kMomentCell doubles per pixel, and the dense planes copied out
    DevBuf<double> d_denoise;   // dtof_denoise_async: the guide records and the two sets of working planes
    DevBuf<float> d_vm_sum, d_vm_tof; DevBuf<double> d_vm_maps;   // dtof_render_velocity_map: the passes' sum, the ToF images, the per-pair maps and the combined map
    // the caller's device film as declared with dtof_scene_set_film_layout (0 = not declared: colour planes only, W * H * 4 apart)
    int32_t film_planes = 0; uint64_t film_plane_stride = 0;
    DevBuf<unsigned long long> d_sums;       // [batch][2*kMaxIter] per-iteration totals (survivors, shadow rays)
    DevBuf<uint2> d_pass_rng;                // multi-pass renders: [lane][3] stream states between the passes
    uint32_t id_shift = 24;                  // Queues::id_shift of this scene
    hipStream_t stream = nullptr;                        // the library's own, or the caller's (dtof_scene_set_stream)
    hipStream_t own_stream = nullptr;                    // what ensure_device created and the destructor destroys
    std::atomic<bool> stop { false };
    uint64_t plan_facts_launches = 0;        // first-bounce launches that took a kernel compiled with plan facts, since the scene was loaded (dtof_scene_plan_facts_launches)
    uint32_t last_plan_facts = 0;            // ... and the FACTS mask of the one the last frame launched, 0 if it launched none (dtof_scene_last_plan_facts)
    // reusable statistics plumbing (creating events / pinned memory per call costs ~0.3 ms)
    std::vector<hipEvent_t> event_pool; size_t events_used = 0;
    // frames enqueued by dtof_render_rows_async and not collected yet: their events (frame, stages) and launch counters; no host synchronisation until dtof_async_collect
    struct DeferredFrame { hipEvent_t ev0, ev1; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[kStageCount]; dtof_render_stats counters; };
    std::vector<DeferredFrame> deferred;
    uint32_t *pinned_counts = nullptr; size_t pinned_words = 0;
    hipEvent_t take_event() {
        if (events_used == event_pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) throw std::runtime_error("hipEventCreate failed"); event_pool.push_back(e); }
        return event_pool[events_used++];
    }
    uint32_t *pinned(size_t words) {
        if (words > pinned_words) {
            if (pinned_counts) (void) hipHostFree(pinned_counts);
            pinned_counts = nullptr; pinned_words = 0;
            if (hipHostMalloc((void **) &pinned_counts, words * 4, hipHostMallocDefault) != hipSuccess) throw std::runtime_error("hipHostMalloc failed");
            pinned_words = words;
        }
        return pinned_counts;
    }
    ~dtof_scene() {
        if (own_stream) (void) hipStreamDestroy(own_stream);
        for (auto e : event_pool) (void) hipEventDestroy(e);
        if (pinned_counts) (void) hipHostFree(pinned_counts);
    }
};

struct dtof_sampler {
    uint32_t sample_count = 4, base_seed = 0; int32_t tcn = 2, pcn = 2;
    uint32_t seed = 0, wavefront = 0, spw = 1, sample_index = 0; bool seeded = false;
    DevBuf<uint2> rng, rng_time, rng_path; DevBuf<uint32_t> perm, dim; DevBuf<float> out; DevBuf<uint8_t> flags;
};

namespace {

void ensure_device(dtof_scene *sc) {
    if (!sc->own_stream) HIP_CHECK(hipStreamCreate(&sc->own_stream));
    if (!sc->stream) sc->stream = sc->own_stream;
    if (!sc->uploaded) {
        sc->d_blob.ensure(sc->blob.size());
        HIP_CHECK(hipMemcpy(sc->d_blob.p, sc->blob.data(), sc->blob.size(), hipMemcpyHostToDevice));
        sc->uploaded = true;
    }
}

// 4x4 float product with the fmadd chain of Dr.Jit's column-major matrix product
void m4_mul(const float *a, const float *b, float *out) {
    float r[16];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
        float s = a[4 * i] * b[j];
        for (int k = 1; k < 4; ++k) s = fmaf(a[4 * i + k], b[4 * k + j], s);
        r[4 * i + j] = s;
    }
    memcpy(out, r, sizeof r);
}
void m4_identity(float *m) { memset(m, 0, 64); m[0] = m[5] = m[10] = m[15] = 1.f; }

// sample_to_camera: inverse of perspective_projection (include/mitsuba/render/sensor.h:226-262) as
// PerspectiveCamera::update_camera_transforms builds it (src/sensors/perspective.cpp:172-198); the
// Transform class carries analytic inverses, so this is the reversed product of the factor inverses.
void sample_to_camera(const HostSensor &s, float *inv_out) {
    float fw = (float) s.film_w, fh = (float) s.film_h;
    float rel_sx = (float) s.crop_w / fw, rel_sy = (float) s.crop_h / fh;
    float rel_ox = (float) s.crop_x / fw, rel_oy = (float) s.crop_y / fh;
    float aspect = fw / fh, near_ = s.near_clip, far_ = s.far_clip;
    float tanv = (float) std::tan((double) (s.x_fov * .5f) * (M_PI / 180.0));
    float S1i[16], T1i[16], S2i[16], T2i[16], Pi[16], tmp[16];
    m4_identity(S1i); S1i[0] = rcp(1.f / rel_sx); S1i[5] = rcp(1.f / rel_sy);
    m4_identity(T1i); T1i[3] = rel_ox; T1i[7] = rel_oy;
    m4_identity(S2i); S2i[0] = rcp(-0.5f); S2i[5] = rcp(-0.5f * aspect);
    m4_identity(T2i); T2i[3] = 1.f; T2i[7] = 1.f / aspect;
    memset(Pi, 0, 64); Pi[0] = tanv; Pi[5] = tanv; Pi[15] = rcp(near_); Pi[11] = 1.f; Pi[14] = (near_ - far_) / (far_ * near_);
    if (s.orthographic) {   // orthographic_projection (sensor.h:266-299): the last factor is scale(1, 1, 1 / (far - near)) * translate(0, 0, -near) (transform.h:242-245)
        float OT[16], OS[16];
        m4_identity(OT); OT[11] = near_;
        m4_identity(OS); OS[0] = rcp(1.f); OS[5] = rcp(1.f); OS[10] = rcp(1.f / (far_ - near_));
        m4_mul(OT, OS, Pi);
    }
    m4_mul(T1i, S1i, tmp); m4_mul(S2i, tmp, tmp); m4_mul(T2i, tmp, tmp); m4_mul(Pi, tmp, inv_out);
}

// the film's reconstruction filter as the splat kernels see it
void set_filter(RenderParams &rp, int32_t filter, float radius, float stddev, float B, float C) {
    rp.filter = filter; rp.filter_radius = radius; rp.inv_radius = 1.f / radius;
    rp.filter_b = B; rp.filter_c = C;
    if (filter == FILTER_GAUSSIAN) {   // GaussianFilter ctor (src/rfilters/gaussian.cpp:60-89), non-CUDA branch
        static const double coeff[10] = { 9.992604880e-1, -4.977025247e-1, 1.222248550e-1, -1.932406282e-2, 2.136713061e-3,
                                          -1.679873860e-4, 9.202145248e-6, -3.329417433e-7, 7.128382794e-9, -6.821193280e-11 };
        double scale = 1;
        for (int i = 0; i < 10; ++i) { rp.gauss_coeff[i] = (float) (coeff[i] * scale); scale /= (double) stddev * (double) stddev; }
        rp.gauss_coeff[0] -= estrin10(radius * radius, rp.gauss_coeff);
    }
}
// spp = samples per wavefront (per pass); sample_count = Sampler::sample_count() of the whole render (0: the same)
// offsets / n_offsets: batched hetero_offset values at the integrator's own frequency; variants / n_variants: batched (hetero_frequency, hetero_offset) pairs.
// At most one of the two is given (n > 0); neither: the integrator's own pair.
RenderParams make_params(const dtof_scene *sc, uint32_t seed, uint32_t spp, const float *offsets, int n_offsets, uint32_t sample_count = 0,
                         const dtof_modulation *variants = nullptr, int n_variants = 0) {
    const HostSensor &se = sc->host.sensor; const PluginParams &pp = sc->pp;
    RenderParams rp; memset(&rp, 0, sizeof rp);
    sample_to_camera(se, rp.s2c);
    memcpy(rp.cam_to_world, se.to_world, 48);
    rp.near_clip = se.near_clip; rp.far_clip = se.far_clip; rp.shutter_open = se.shutter_open;
    rp.shutter_open_time = se.shutter_close - se.shutter_open;
    rp.orthographic = se.orthographic ? 1 : 0;
    rp.aperture_radius = se.thinlens ? se.aperture_radius : 0.f; rp.focus_distance = se.focus_distance;
    rp.crop_x = se.crop_x; rp.crop_y = se.crop_y; rp.crop_w = se.crop_w; rp.crop_h = se.crop_h;
    rp.scale_x = 1.f / (float) se.crop_w; rp.scale_y = 1.f / (float) se.crop_h;
    rp.offset_x = -(float) se.crop_x * rp.scale_x; rp.offset_y = -(float) se.crop_y * rp.scale_y;
    set_filter(rp, se.filter, se.filter_radius, se.filter_stddev, se.filter_b, se.filter_c);
    rp.base_seed = pp.base_seed; rp.seed = seed; rp.seed_value = pp.base_seed + seed;
    rp.spp = spp; rp.spp_log2 = 0xffffffffu;
    for (uint32_t b = 0; b < 32; ++b) if ((1u << b) == spp) rp.spp_log2 = b;
    rp.tcn = (uint32_t) pp.time_correlate_number; rp.pcn = (uint32_t) pp.path_correlate_number;
    rp.time_sampling = pp.time_sampling; rp.antithetic_shift = pp.antithetic_shift; rp.stratify = pp.stratify_each_interval;
    if (sample_count == 0) sample_count = spp;
    rp.sample_count = sample_count; rp.d_sample_count = make_fastdiv(sample_count);
    rp.n_stratum = sample_count / rp.tcn;                          // int n_stratum = m_sample_count / tcn (correlated.cpp:112)
    rp.inv_n_stratum = rp.n_stratum ? 1.0f / (float) (int) rp.n_stratum : 0.f;
    rp.inv_tcn = 1.0f / (float) pp.time_correlate_number;
    rp.d_spp = make_fastdiv(spp); rp.d_w = make_fastdiv((uint32_t) se.crop_w); rp.d_tcn = make_fastdiv(rp.tcn); rp.d_pcn = make_fastdiv(rp.pcn);
    rp.d_stratum = make_fastdiv(rp.n_stratum);
    for (uint32_t d : { spp, sample_count, (uint32_t) se.crop_w, rp.tcn, rp.pcn, rp.n_stratum })   // the kernels have no other division: fail loudly
        for (uint32_t n : { 0u, 1u, d - 1, d, d + 1, 2 * d - 1, 0x7fffffffu, 0xfffffffeu, 0xffffffffu })
            if (d && fdiv(n, make_fastdiv(d)) != n / d) throw std::runtime_error("internal error: fast division self-check failed");
    rp.n_passes = 1;
    // eval_modulation_weight's scalar prefactors are folded in double and rounded to float32 once
    // (they multiply JIT float32 arrays), dopplertofpath.cpp:62-69
    rp.T = pp.time;
    rp.w_g = (float) (2 * M_PI * (double) pp.w_g_mhz * 1e6);
    const auto w_d_of = [&](float hetero_frequency) { return (float) (2 * M_PI / (double) pp.time * (double) hetero_frequency); };
    const auto phase_of = [](float hetero_offset) { return (float) ((double) (hetero_offset * 2) * M_PI); };   // dopplertofpath.cpp:30-32
    for (int k = 0; k < kMaxOffsets; ++k) rp.w_d[k] = w_d_of(pp.hetero_frequency);
    rp.phi_coef = (float) ((2 * M_PI * (double) pp.w_g_mhz) / 300);
    rp.amp = (float) (0.5 * (double) pp.g_1);
    rp.g_1 = pp.g_1; rp.g_0 = pp.g_0;
    rp.wave_type = pp.wave_type; rp.low_pass = pp.low_frequency_component_only;
    if (n_variants > 0) {   // film k: the render of an integrator with hetero_frequency = f_k, hetero_offset = o_k (constructor roundings, dopplertofpath.cpp:26-32)
        if (n_variants > kMaxOffsets) throw std::runtime_error("at most 4 modulation variants can be batched per traversal");
        rp.n_offsets = n_variants;
        for (int k = 0; k < n_variants; ++k) { rp.w_d[k] = w_d_of(variants[k].hetero_frequency); rp.phase[k] = phase_of(variants[k].hetero_offset); }
    } else if (n_offsets <= 0) { rp.n_offsets = 1; rp.phase[0] = pp.phase_offset; }
    else {
        if (n_offsets > kMaxOffsets) throw std::runtime_error("at most 4 modulation offsets can be batched per traversal");
        rp.n_offsets = n_offsets;
        for (int k = 0; k < n_offsets; ++k) rp.phase[k] = phase_of(offsets[k]);
    }
    rp.path_correlation_depth = pp.path_correlation_depth; rp.max_depth = pp.max_depth; rp.rr_depth = pp.rr_depth;
    rp.integrator = pp.integrator;
    rp.sampler_kind = pp.sampler_kind; rp.jitter = pp.jitter; rp.inv_spp = 1.0f / (float) sample_count;   // dr::rcp(ScalarFloat(m_sample_count))
    if (pp.integrator != INTEGRATOR_DOPPLER && (n_offsets > 0 || n_variants > 0)) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");
    return rp;
}

// Optional roctx ranges around the stage launches (the counterpart of the reference's ScopedPhase / NVTX ranges,
// include/mitsuba/core/profiler.h): DTOF_ROCTX=1 loads the roctx library at run time, `rocprofv3 --marker-trace` then shows
// "dtof:generate|trace|shade|shadow|splat|first" ranges on the host timeline.  No link-time dependency.
struct Roctx {
    int (*push)(const char *) = nullptr; int (*pop)() = nullptr;
    Roctx() {
        const char *e = getenv("DTOF_ROCTX");
        if (!e || e[0] == '0') return;
        void *h = nullptr;   // rocprofv3 listens to the SDK's roctx; the older libroctx64 serves rocprof v1 / v2
        for (const char *name : { "librocprofiler-sdk-roctx.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so", "libroctx64.so", "/opt/rocm/lib/libroctx64.so" })
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) return;
        push = (int (*)(const char *)) dlsym(h, "roctxRangePushA"); pop = (int (*)()) dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr;
    }
};
static const Roctx &roctx() { static const Roctx r; return r; }
static const char *const kStageNames[kStageCount] = { "dtof:generate", "dtof:trace", "dtof:shade", "dtof:shadow", "dtof:splat", "dtof:first" };

struct StageTimer {
    bool on; dtof_scene *sc; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[kStageCount];
    StageTimer(bool enabled, dtof_scene *scene) : on(enabled), sc(scene) { if (sc->deferred.empty()) sc->events_used = 0; }   // the events of uncollected frames stay taken
    int begin(Stage stage, hipStream_t s) {
        if (roctx().push) roctx().push(kStageNames[stage]);
        if (!on) return -1;
        hipEvent_t a = sc->take_event(), b = sc->take_event();
        ev[stage].emplace_back(a, b); HIP_CHECK(hipEventRecord(a, s));
        return (int) ev[stage].size() - 1;
    }
    void end(Stage stage, int idx, hipStream_t s) {
        if (on) HIP_CHECK(hipEventRecord(ev[stage][idx].second, s));
        if (roctx().push) roctx().pop();
        static const bool sync_each = [] { const char *e = getenv("DTOF_SYNC_LAUNCHES"); return e && e[0] == '1'; }();   // debugging: which stage of a frame never finishes?
        if (sync_each) { fprintf(stderr, "[dtof] %s enqueued ...", kStageNames[stage]); fflush(stderr); HIP_CHECK(hipStreamSynchronize(s)); fprintf(stderr, " done\n"); fflush(stderr); }
    }
};
double stage_ms(const std::vector<std::pair<hipEvent_t, hipEvent_t>> &ev) {
    double ms = 0;
    for (auto &p : ev) { float t = 0; HIP_CHECK(hipEventElapsedTime(&t, p.first, p.second)); ms += t; }
    return ms;
}

// film elements (4 per pixel) of the rows a call that renders rows [row_lo, row_hi) can write: the rows and the filter's halo on either side, inside the film
static uint64_t film_rows_reach(const HostSensor &se, int32_t row_lo, int32_t row_hi, int32_t *first = nullptr, int32_t *end = nullptr) {
    const int32_t halo = se.filter == FILTER_BOX ? 0 : (int32_t) std::ceil(se.filter_radius - .5f);
    const int32_t r0 = std::max(row_lo, 0), r1 = std::min(row_hi, se.crop_h);
    const int32_t lo = std::max(r0 - halo, 0), hi = std::min(r1 + halo, se.crop_h);
    if (first) *first = lo;
    if (end) *end = hi;
    return r1 > r0 ? (uint64_t) (hi - lo) * se.crop_w * 4 : 0;   // an empty band writes nothing
}
// The device-film entry points write K colour planes and, for an rgba film, the alpha plane behind them into memory whose size only the caller knows: an rgba scene is
// refused until the caller has declared a film of K + 1 planes (a caller written for rgb films would have its buffer overrun), and a declared count is checked either way.
// [row_lo, row_hi): the film rows whose lanes the call renders.  Their splats reach `halo` rows further (the reconstruction filter), so with more than one plane a
// declared stride must hold rows [max(row_lo - halo, 0), min(row_hi + halo, H)) or plane k + 1 would be added into plane k: such a call is refused before any launch.
static uint64_t caller_film_stride(const dtof_scene *sc, int n_offsets, int32_t row_lo, int32_t row_hi) {
    const HostSensor &se = sc->host.sensor;
    const int need = (n_offsets <= 0 ? 1 : n_offsets) + (se.alpha ? 1 : 0);
    if (se.alpha && sc->film_planes < need)
        throw std::runtime_error("rgba film: the device film needs " + std::to_string(need) + " RGBW planes (the alpha film lies behind the colour films); declare them with dtof_scene_set_film_layout");
    if (sc->film_planes != 0 && sc->film_planes < need)
        throw std::runtime_error("the device film was declared with " + std::to_string(sc->film_planes) + " planes, this call writes " + std::to_string(need));
    const uint64_t full = (uint64_t) se.crop_w * se.crop_h * 4;
    if (need > 1 && sc->film_plane_stride != 0) {
        int32_t lo = 0, hi = 0;
        const uint64_t reach = film_rows_reach(se, row_lo, row_hi, &lo, &hi);
        if (sc->film_plane_stride < reach)
            throw std::runtime_error("the declared plane stride of " + std::to_string(sc->film_plane_stride) + " floats is smaller than the " + std::to_string(reach) +
                                     " floats of film rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") this call writes: the planes would overlap");
    }
    return sc->film_plane_stride ? sc->film_plane_stride : full;
}
// the rows [first, last + 1) that hold the stripes [first_row + k * stripe_period, ... + stripe_rows) below the film's height (the mapping of plan_lanes)
static std::pair<int32_t, int32_t> stripe_span(const dtof_scene *sc, int32_t first_row, int32_t stripe_rows, int32_t stripe_period) {
    const int32_t h = sc->host.sensor.crop_h, first = std::max(first_row, 0);
    const int64_t span = std::max<int64_t>(h - first, 0), v_rows = (span / stripe_period) * stripe_rows + std::min<int64_t>(span % stripe_period, stripe_rows);
    if (v_rows == 0) return {first, first};
    return {first, (int32_t) (first + ((v_rows - 1) / stripe_rows) * stripe_period + (v_rows - 1) % stripe_rows + 1)};
}

// One call of the renderer, as the entry points fill it in.  The film layout the caller declared (dtof_scene_set_film_layout) stays scene state.
struct RenderRequest {
    uint32_t seed = 0, spp = 0;                   // spp 0: the sampler's sample count
    int32_t row_begin = 0, row_end = 0;           // film rows [row_begin, row_end)
    bool stripes = false; int32_t stripe_rows = 0, stripe_period = 0;   // stripes: only the rows [row_begin + k * stripe_period, ... + stripe_rows) (interleaved shards)
    const float *offsets = nullptr; int n_offsets = 0;                // batched hetero_offset values, or
    const dtof_modulation *variants = nullptr; int n_variants = 0;   // ... batched (hetero_frequency, hetero_offset) pairs (at most one of the two)
    int films() const { return n_variants > 0 ? n_variants : n_offsets > 0 ? n_offsets : 1; }   // colour films the call writes
    float4 *lane_planes = nullptr;                // lane dumps: [films()][dump_n] results of every film (q.res), besides film 0's in lane_dump
    float *film = nullptr; uint64_t film_stride = 0;   // K films (and the alpha film behind them) film_stride floats apart
    double *film64 = nullptr; uint64_t film64_stride = 0;   // ... or the float64 film, film64_stride doubles apart: the separate splat stage accumulates in double (dtof_film64.hip)
    double *moments = nullptr;                    // ... or the moment film (dtof_moments.h: cells of kMomentCell doubles), likewise the separate splat stage's; no alpha film
    const AovArgs *aov = nullptr;                 // ... or the geometry channels of the `aov` integrator (dtof_aov.h): k_aov takes the shade loop's place behind k_generate and
                                                  // splats into aov->film itself, or -- with a lane dump -- writes the dumped lanes' channels to aov->values ([dump_n][n_channels])
    dtof_render_stats *stats = nullptr;
    LaneDebug *lane_dump = nullptr; uint64_t dump_begin = 0, dump_n = 0;   // lane_dump != nullptr: evaluate only lanes [dump_begin, dump_begin + dump_n) and copy their records out
    bool deferred = false;                        // dtof_render_rows_async: timings by events, no counters read back, no synchronisation at the end
};

// What the frame plan derives from the scene's arrays and blob header, each array walked once.  Computed per call and never cached on the scene.
struct SceneTraits {
    int32_t has_spec = 0;                 // the every-BSDF (SPEC) kernels; 2: ... whose BSDF chain loops over two records (blendbsdf)
    bool has_tris = false, has_analytic = false, has_blas = false, has_nodes16 = false;
    bool surface_emitters = false, has_env = false, null_lobe = false;
    uint32_t env_index = 0, n_instances = 0, last_instance = 0;
    uint64_t blas_triangles = 0;          // triangles behind per-mesh BLASes
    uint32_t n_nodes = 0, n_tlas_nodes = 0, n_objects = 0, stack_depth = 0, flat_off = 0;
    uint32_t flat_general = 0, flat_memo = 0;   // the flat table's DFlatKinds: objects that are general instances | instances of ONE rectangle
    bool resident_layout = false; uint32_t small_off = 0, small_words = 0;   // the blob's record block can be the resident stage's
};
static uint32_t bh_emitters(const dtof_scene &sc) { return ((const BlobHeader *) sc.blob.data())->n_emitters; }   // the emitter count the kernels see (SceneView::n_emitters)
SceneTraits scene_traits(const dtof_scene &sc) {
    const HostScene &hs = sc.host; const HostSensor &se = hs.sensor;
    const BlobHeader *bh = (const BlobHeader *) sc.blob.data();
    SceneTraits t;
    // SPEC: every BSDF but the diffuse one, masks, normal maps, textures, spot / directional / environment emitters, and cameras other than the
    // pinhole one (the diffuse-only kernels generate perspective rays only: generate_lane<PERSPECTIVE_ONLY>)
    bool spec = !hs.textures.empty() || se.thinlens || se.orthographic, blend = false;
    for (auto &sh : hs.shapes) {
        spec |= sh.bsdf != BSDF_DIFFUSE || sh.masked || sh.tex_normal >= 0 || sh.blend_other;
        blend |= sh.blend_other != nullptr;
        t.has_analytic |= sh.kind == SHAPE_SPHERE || sh.kind == SHAPE_DISK || sh.kind == SHAPE_CYLINDER;   // analytic shapes of the MESH instantiations
        // a BSDF with a null lobe (`mask`, `thindielectric`) leaves valid_ray unset -- over the whole chain of material records behind a shape (a blend's partner, the
        // back side of a two-BSDF twosided, and whatever those carry in turn), so that a nesting the loader learns to accept later cannot slip one past this test
        for (const HostShape *m = &sh; m; m = m->blend_other.get())
            t.null_lobe |= m->masked || m->bsdf == BSDF_THINDIELECTRIC || m->bsdf == BSDF_NULL;
    }
    for (size_t i = 0; i < hs.emitters.size(); ++i) {
        const auto kind = hs.emitters[i].kind;
        t.surface_emitters |= kind == EMITTER_AREA || kind == EMITTER_CONSTANT || kind == EMITTER_ENVMAP;   // the environment is "hit" by the rays that leave the scene
        spec |= kind == EMITTER_SPOT || kind == EMITTER_DIRECTIONAL || kind == EMITTER_CONSTANT || kind == EMITTER_ENVMAP;
        if (kind == EMITTER_CONSTANT || kind == EMITTER_ENVMAP) { t.has_env = true; t.env_index = (uint32_t) i; }
    }
    t.has_spec = blend ? 2 : spec ? 1 : 0;
    // anything but rectangles: the instantiations with triangle / sphere code.  The SPEC shade kernels are MESH instantiations (full 16-byte hit
    // record), so the trace kernels of the split pipeline must write that record for them too: a rectangle-only scene with textures (or any other
    // SPEC feature) counts as "has_tris" -- the compact 4-byte record is for the plain rectangle-only kernels
    t.has_tris = bh->n_tris != 0 || t.has_analytic || t.has_spec;
    const DShape *dshapes = (const DShape *) (sc.blob.data() + bh->off_shapes);
    for (uint32_t i = 0; i < bh->n_shapes; ++i)
        if (dshapes[i].kind == SHAPE_MESH && dshapes[i].blas_root != kNoChild) { t.has_blas = true; t.blas_triangles += dshapes[i].n_tris; }
    const DObject *dobj = (const DObject *) (sc.blob.data() + bh->off_objects);
    for (uint32_t i = 0; i < bh->n_objects; ++i) if (dobj[i].kind == OBJ_INSTANCE) { ++t.n_instances; t.last_instance = i; }
    t.has_nodes16 = bh->off_nodes16 != 0; t.n_nodes = bh->n_nodes; t.n_tlas_nodes = bh->n_tlas_nodes; t.n_objects = bh->n_objects;
    t.stack_depth = bh->tlas_depth; t.flat_off = bh->off_flat;
    if (bh->off_flat) {
        const DFlatKinds *kinds = (const DFlatKinds *) (sc.blob.data() + bh->off_flat + (size_t) bh->n_objects * sizeof(DFlatObject));
        t.flat_general = kinds->general; t.flat_memo = kinds->memo;
    }
    // groups | shapes | emitters | triangles | shading data | intersection records: one block of at most 24 KiB in a blob too large to stage whole
    const uint32_t small_bytes = bh->off_tables - bh->off_groups;
    t.resident_layout = bh->n_nodes > 0 && sc.blob.size() > 16 * 1024 && bh->off_shapes > bh->off_groups && bh->off_emitters > bh->off_groups && bh->off_tris > bh->off_groups &&
                        bh->off_shading >= bh->off_tris && bh->off_isect >= bh->off_shading && bh->off_tables >= bh->off_isect && small_bytes <= 24 * 1024;
    t.small_off = bh->off_groups; t.small_words = (small_bytes + 15) / 16;
    return t;
}

// What one launch of the bounce loop covers when it starts at an iteration
struct LaunchSpan { uint32_t span, chunk_blocks, res_units; bool next_runs, splat_here, terminal, resident; };

// What a frame's plan takes from the scene's flat table (plan_frame; dtof_scene_export kind 26 shows it for the automatic pipeline and the default switches):
struct FlatChoice { uint32_t memo_obj, flat_objects, facts; };
FlatChoice flat_choice(const SceneTraits &t, bool fused, bool memo_on, bool flat_on) {
    FlatChoice c;
    // instance memo (dtof_traverse.h): pays when there is exactly one instance object, which then nearly every ray visits
    c.memo_obj = fused && t.n_instances == 1 && memo_on ? t.last_instance : 0xffffffffu;
    // a handful of rectangles: test them all instead of walking a tree (trace_flat in dtof_traverse.h)
    c.flat_objects = fused && !t.has_tris && t.flat_off != 0 && flat_on ? t.n_objects : 0u;
    // ... whose only instance is the memo object and holds one rectangle (kFactOneWall; the launch of such a scene keeps the instance matrix in LDS, k_shade: memo_m_lds),
    // and then the table's shape, read off the blob's own counts: how many objects, and which of them the wall is (kFactFlatShape; 0 for more than 8 objects)
    const bool one_wall = c.flat_objects != 0 && c.memo_obj < 32u && t.flat_general == 0 && t.flat_memo == (1u << c.memo_obj);
    c.facts = one_wall ? kFactOneWall | flat_shape_fact(c.flat_objects, c.memo_obj) : 0u;
    return c;
}

// Every decision of a frame, taken before its first launch.  The batch loop reads it and sets only the per-batch and per-launch fields of its copy of rp.
struct FramePlan {
    RenderParams rp;                      // the frame's parameters, with the scene's flags and the kernel choices they carry
    SceneTraits traits;
    uint32_t n_passes = 1, run_passes = 1, dump_pass = 0;
    uint64_t lanes_per_row = 0, first = 0, last = 0, batch = 1;   // every pass: lanes [first, last) in batches of `batch`
    bool fused = false, first_inline = false, skip_tail = false, fuse_splat_ok = false, terminal_ok = false, plan_facts = false, one_wall = false;
    uint32_t flat_shape = 0;              // the shape fields of the flat table under one_wall (flat_shape_fact), 0 if it has none
    uint32_t max_inline = 1, chunk_segs = 0, res_units = 1, n_emitters = 0, id_shift = 0;   // id_shift: Queues::id_shift of the frame's launches
    ResidentStage resident;
    LaunchSwitches launch;                // launch.defer: the DEFER mode, 0 when the workspaces have no DEFER lists
    // does iteration `it` of the bounce loop run?  (the reference's last iteration only looks for emitter hits, dopplertofpath.cpp:136-171: skip_tail drops it)
    bool iteration_runs(uint32_t it) const { return it < rp.max_depth && !(it + 1 >= rp.max_depth && skip_tail); }
    LaunchSpan launch_span(uint32_t it, bool first, uint32_t n_seg) const {
        // The fused first-bounce kernel runs up to max_inline iterations itself, the path state in registers; multi-pass renders, whose stream states must be in
        // memory between the passes, one per launch.  (One compacted launch per iteration instead lost: profiles/r04_compaction_ab.txt.)
        LaunchSpan l; l.span = 1;
        if (first && n_passes == 1) while (l.span < max_inline && iteration_runs(it + l.span)) ++l.span;
        l.next_runs = iteration_runs(it + l.span);
        // no iteration follows this launch's last one: it may run in its terminal form (RenderParams::terminal)
        l.terminal = terminal_ok && !l.next_runs;
        // small frames whose whole path runs inline: one block per 64-lane chunk (8 x the waves); the count slots it adds into are zeroed first
        const bool whole_path = first && !l.next_runs;
        l.chunk_blocks = whole_path && n_seg <= chunk_segs ? kChunkBlocks : 1u;
        // the resident kernel's launch: the plan offers a stage (fused pipeline, mesh code, a wave count that fits: plan_frame) and there is one block per segment
        l.resident = first && resident.waves != 0 && l.chunk_blocks == 1;
        // parts of a segment as the resident kernel's work units shorten the launch's tail (kept for a frame sharded over many GPUs); their count slots are added into
        l.res_units = whole_path ? res_units : 1u;
        // fused splat: every wave of a whole-path launch holds the 64 samples of one pixel and adds their footprint to the film itself (no round trip through q.res)
        l.splat_here = whole_path && fuse_splat_ok;
        return l;
    }
    // The plan facts (dtof_kernels.h: kFact*) a first-bounce launch satisfies: `r` is the launch's RenderParams (batch and span fields set), depth0 its first iteration,
    // identity_queue = it reads neither a lane queue nor segment counts, dump = it writes the lane dump's camera rays.  A launcher takes a kernel compiled with a mask of
    // these only if every fact of the mask is set here; 0 (DTOF_PLAN_FACTS=0, or any launch but a first-bounce one) selects the generic kernels.
    uint32_t launch_facts(const RenderParams &r, const LaunchSpan &l, uint32_t depth0, bool first, bool identity_queue, bool dump) const {
        if (!plan_facts || !first) return 0u;
        const uint32_t depth_end = depth0 + l.span;   // one past the deepest iteration the launch runs
        uint32_t f = 0;
        if (r.n_passes == 1 && r.pass == 0) f |= kFactSinglePass;
        if (r.integrator == 0 && r.sampler_kind == SAMPLER_CORRELATED) f |= kFactDopplerCorr;
        if (!dump && !r.want_valid) f |= kFactNoLaneOutput;
        if (identity_queue) f |= kFactIdentityQueue;
        if (r.rr_depth > depth_end) f |= kFactNoRoulette;                 // the deepest test is ndepth = depth_end >= rr_depth
        if (depth_end < r.path_correlation_depth) f |= kFactCorrelated;   // the deepest test is depth_end - 1 + 1 < path_correlation_depth
        if (!l.next_runs && l.terminal) f |= kFactWholePath;
        if (l.chunk_blocks == 1) f |= kFactOneBlock;
        if (n_emitters == 1) f |= kFactOneEmitter;
        if (r.flat_objects != 0) f |= kFactFlat;
        if (one_wall) f |= kFactOneWall | flat_shape;   // the shape fields are values: a launcher matches them by equality (facts_hold)
        // the routes of the correlated sampler's time draw and of the modulation weight; n_stratum & (n_stratum - 1): a power of two has one bit
        if ((f & kFactDopplerCorr) && r.time_sampling == TIME_STRATIFIED && r.stratify != 0 && r.tcn == 2 && r.pcn == 2 && r.shutter_open_time > 0.f && r.spp > 1) f |= kFactStratifiedPairs;
        if (r.n_stratum >= 2 && (r.n_stratum & (r.n_stratum - 1u)) == 0) f |= kFactPow2Strata;
        if (r.low_pass != 0 && r.wave_type == WAVE_SIN) f |= kFactSineLowPass;
        if (depth_end < r.max_depth) f |= kFactEmitterSampled;            // the deepest test is depth_end - 1 + 1 < max_depth
        if (id_shift == 24) f |= kFactIdShift24;
        if (l.splat_here) f |= kFactFusedSplat;   // (the launcher hands in the film exactly then)
        // every segment's count is min(512, n_lanes - 512 S), a multiple of 64 if n_lanes is one: each 64-lane chunk is then whole, and its lanes are the 64-aligned
        // lanes [lane_base + 512 S + cbase, + 64), samples of one pixel when spp is a power of two >= 64.  (A striped shard -- a rank's share of a frame, virtual lanes --
        // keeps the run-time test and with it the generic kernel.)
        if (identity_queue && r.stripe_rows == 0 && r.spp_log2 != 0xffffffffu && r.spp_log2 >= 6 && (r.lane_base & 63u) == 0 && (r.n_lanes & 63u) == 0) f |= kFactWavePixel;
        // the two lanes of a pair can split the BSDF samples of the launch between them: they hold one path stream, every draw comes from it, no draw is
        // looked at for roulette or for an emitter pick, and the launch is the whole path in three iterations -- two that sample a BSDF and the terminal one
        constexpr uint32_t pair_needs = kFactWholePath | kFactWavePixel | kFactStratifiedPairs | kFactCorrelated | kFactDopplerCorr | kFactNoRoulette | kFactOneEmitter;
        if (l.span == 3 && (f & pair_needs) == pair_needs) f |= kFactPairSamples;
        return f;
    }
};

// Call validation and the split into passes and lane ranges.  SamplingIntegrator::render (integrator.cpp:121-135,227-245): spp_per_pass = min(samples_per_pass, spp)
// must divide spp; a wavefront of more than 2^32 - 1 lanes is split into more passes (integer division, as written there), and Sampler::set_samples_per_wavefront
// (sampler.cpp:75-83) insists that the sample count is a multiple of the samples per pass.  rp.spp is the samples per PASS.
void plan_lanes(FramePlan &p, const dtof_scene *sc, const RenderRequest &rq) {
    const HostSensor &se = sc->host.sensor;
    uint32_t spp = rq.spp ? rq.spp : sc->pp.sample_count;
    if (spp == 0) throw std::runtime_error("sample count must be positive");
    const uint32_t sample_count = spp;
    uint32_t per_pass = sc->pp.samples_per_pass == 0xffffffffu || sc->pp.samples_per_pass == 0 ? spp : std::min(sc->pp.samples_per_pass, spp);
    if (spp % per_pass != 0) throw std::runtime_error("sample_count (" + std::to_string(spp) + ") must be a multiple of spp_per_pass (" + std::to_string(per_pass) + ").");
    const uint64_t wavefront = (uint64_t) se.crop_w * se.crop_h * per_pass, limit = 0xffffffffull;
    if (wavefront > limit) {
        per_pass /= (uint32_t) ((wavefront + limit - 1) / limit);
        if (per_pass == 0 || spp % per_pass != 0) throw std::runtime_error("sample_count should be a multiple of samples_per_wavefront!");
    }
    p.n_passes = spp / per_pass; spp = per_pass;
    const uint64_t total_lanes = (uint64_t) se.crop_w * se.crop_h * spp;   // lanes of one pass (the wavefront)
    if (sc->pp.time_sampling != TIME_UNIFORM && sc->pp.stratify_each_interval && sample_count < (uint32_t) sc->pp.time_correlate_number)
        throw std::runtime_error("sample count must be at least time_correlate_number when per-interval stratification is on");
    if (sc->pp.integrator == 0 && sc->pp.sampler_kind == SAMPLER_CORRELATED && sc->pp.time_sampling == TIME_ANTITHETIC_MIRROR && sc->pp.time_correlate_number != 2)
        throw std::runtime_error("antithetic_mirror time sampling needs time_correlate_number == 2");   // Assert(m_time_correlate_number == 2), correlated.cpp:142
    p.rp = make_params(sc, rq.seed, spp, rq.offsets, rq.n_offsets, sample_count, rq.variants, rq.n_variants);
    p.rp.n_passes = p.n_passes;
    // lane dumps address (pass, lane) as pass * wavefront + lane and must stay inside one pass
    uint64_t dump_begin = rq.dump_begin;
    if (rq.lane_dump) {
        p.dump_pass = (uint32_t) (dump_begin / total_lanes); dump_begin %= total_lanes;
        if (p.dump_pass >= p.n_passes || dump_begin + rq.dump_n > total_lanes) throw std::runtime_error("lane range exceeds the wavefront");
    }
    const int32_t row_begin = std::max(rq.row_begin, 0), row_end = std::min(rq.row_end, se.crop_h);
    p.lanes_per_row = (uint64_t) se.crop_w * spp;
    p.first = rq.lane_dump ? dump_begin : p.lanes_per_row * (uint64_t) row_begin;
    p.last = rq.lane_dump ? dump_begin + rq.dump_n : p.lanes_per_row * (uint64_t) std::max(row_end, row_begin);
    if (p.last > total_lanes) throw std::runtime_error("lane range exceeds the wavefront");
    if (rq.stripes) {   // virtual rows [0, V): the rows of this shard's stripes in ascending order
        const uint32_t stripe_rows = (uint32_t) rq.stripe_rows, stripe_period = (uint32_t) rq.stripe_period;
        const uint64_t span = (uint64_t) std::max(row_end - row_begin, 0), full = span / stripe_period, rest = span % stripe_period;
        const uint64_t v_rows = full * stripe_rows + std::min<uint64_t>(rest, stripe_rows);
        RenderParams &rp = p.rp;
        rp.stripe_rows = stripe_rows; rp.stripe_period = stripe_period; rp.stripe_first = (uint32_t) row_begin; rp.lanes_per_row = (uint32_t) p.lanes_per_row;
        rp.d_lanes_per_row = make_fastdiv(rp.lanes_per_row); rp.d_stripe_rows = make_fastdiv(stripe_rows);
        p.first = 0; p.last = v_rows * p.lanes_per_row;
    }
    p.run_passes = rq.lane_dump ? p.dump_pass + 1 : p.n_passes;   // a lane dump of pass k needs the stream states passes 0 .. k-1 leave
}

// Every decision of the frame.  The development switches of the frame path are read here, once per frame, and nowhere else:
//   switch              default     selects
//   DTOF_PIPELINE       auto        split | fused: the pipeline
//   DTOF_FUSE_FIRST     1           0: separate k_generate + k_trace launches instead of the fused first-bounce kernel
//   DTOF_INSTANCE_MEMO  1           0: no instance memo
//   DTOF_FLAT           1           0: fused rectangle-only scenes keep the TLAS instead of testing every object (trace_flat)
//   DTOF_RESIDENT       16 / 12 / 8 waves per block of the resident first-bounce kernel, 8 | 12 | 16 (anything else: off); default 12 for every-BSDF scenes, 8 with several films
//   DTOF_RESIDENT_HALF  1           0: a TLAS of 1 025 .. 2 048 nodes takes the classic launch instead of half-float LDS planes (k_shade: RH16)
//   DTOF_FUSE_SPLAT     1           0: the splat kernel instead of the first-bounce kernel's own splat
//   DTOF_INLINE_ITERS   kMaxInline  iterations the first-bounce kernel runs back to back (1 .. kMaxInline)
//   DTOF_CHUNK_SEGS     8192        frames up to this many segments whose whole path runs inline: one block per 64-lane chunk
//   DTOF_RES_UNITS      1           work units per segment of a resident launch covering the whole path, 1 | 2 | 4 | 8 (measured and left off: profiles/r05_resident_units.txt)
//   DTOF_BATCH_LANES    2^27        lanes per wavefront batch
//   DTOF_DEFER          2           BLAS scenes' ray kernels as a pair of launches: 0 never, 1 every one, 2 all but the primary rays' (profiles/r05_mesh_room.txt section 8:
//                                   primary rays that reach a blob already fill their waves), 3 the shadow rays' only
//   DTOF_TRACE8         1           0: the six-wave ray kernels instead of the eight-wave ones
//   DTOF_NODES16        1           0: the 64-byte float nodes instead of their half-float copy
//   DTOF_TLAS_LDS       1           0: the eight-wave ray kernels walk the TLAS in global memory like the BLAS
//   DTOF_XCD_REMAP      auto        blocks per XCD run of the unstaged ray kernels (0: no remap)
//   DTOF_TRACE_BLOCK    auto        64 | 128 | 256: block of the unstaged ray kernels
//   DTOF_STAGE          1           0: never stage the scene into LDS
//   DTOF_SPLAT          auto        dpp | generic: that splat kernel
//   DTOF_TERMINAL_SKIP  1           0: the last iteration that runs keeps the half of the bounce nobody reads (BSDF sampling, continuation ray, throughput / RR,
//                                   the advance of the streams) instead of its terminal form
//   DTOF_PLAN_FACTS     1           0: a first-bounce launch always takes the generic kernel, never the one compiled with the frame plan's constants (kFact*)
// Process-wide instead: DTOF_STAT_SLOTS (sizes the count slots), DTOF_ROCTX and DTOF_SYNC_LAUNCHES (debugging aids).
FramePlan plan_frame(const dtof_scene *sc, const RenderRequest &rq) {
    const auto num = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
    const auto on = [](const char *name) { const char *e = getenv(name); return !(e && e[0] == '0'); };
    const auto str = [](const char *name) { const char *e = getenv(name); return std::string(e ? e : ""); };
    const std::string env_pipeline = str("DTOF_PIPELINE"), env_splat = str("DTOF_SPLAT");
    const int env_inline = num("DTOF_INLINE_ITERS", (int) kMaxInline), env_units = num("DTOF_RES_UNITS", 1), env_block = num("DTOF_TRACE_BLOCK", 0);
    const char *env_resident = getenv("DTOF_RESIDENT"), *env_batch = getenv("DTOF_BATCH_LANES");
    const uint64_t batch_lanes = env_batch && strtoull(env_batch, nullptr, 10) ? strtoull(env_batch, nullptr, 10) : (1ull << 27);
    FramePlan p;
    LaunchSwitches &ls = p.launch;
    ls.defer = num("DTOF_DEFER", 2); ls.trace8 = on("DTOF_TRACE8"); ls.nodes16 = on("DTOF_NODES16"); ls.tlas_lds = on("DTOF_TLAS_LDS"); ls.stage = on("DTOF_STAGE");
    ls.xcd_set = getenv("DTOF_XCD_REMAP") != nullptr; ls.xcd_remap = (uint32_t) num("DTOF_XCD_REMAP", 0);
    ls.trace_block = (uint32_t) (env_block == 64 || env_block == 128 || env_block == 256 ? env_block : 0);
    ls.splat = env_splat == "dpp" ? 1 : env_splat == "generic" ? 2 : 0;
    p.max_inline = (uint32_t) (env_inline < 1 ? 1 : env_inline > (int) kMaxInline ? (int) kMaxInline : env_inline);
    p.chunk_segs = (uint32_t) num("DTOF_CHUNK_SEGS", 8192);
    p.res_units = (uint32_t) (env_units == 1 || env_units == 2 || env_units == 4 || env_units == 8 ? env_units : 1);

    plan_lanes(p, sc, rq);
    const SceneTraits &t = p.traits = scene_traits(*sc);
    const HostSensor &se = sc->host.sensor;
    RenderParams &rp = p.rp;
    // batches of 2^27 lanes (26 GB of workspace at 200 B per lane, 40 GB with four offset films -- of 288): every launch ends with a tail in which the CUs run dry one after
    // the other, and a Domino frame in 32 launches of 2^24 lanes lost 7 % to it (C5 206 -> 193 ms, C4 44.8 -> 41.1; profiles/r03_batch_lanes.txt); one launch per C4
    // frame instead of two is another 2 % (34.86 -> 34.14 ms, profiles/r04_domino_waves_batch.txt)
    p.batch = rq.lane_dump ? std::min<uint64_t>(batch_lanes, std::max<uint64_t>(rq.dump_n, 1)) : std::max<uint64_t>(1, batch_lanes / p.lanes_per_row) * p.lanes_per_row;
    p.batch = std::min<uint64_t>(p.batch, std::max<uint64_t>(p.last - p.first, 1));
    if (p.batch > sc->ws.capacity) {   // a workspace that has to grow: keep it within the free device memory (168 B + 32 B per offset film per lane, and as much again left free)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const uint64_t per_lane = 168 + 32ull * (uint64_t) std::max<int32_t>(rp.n_offsets, 1);
            while (p.batch > (1ull << 22) && p.batch * per_lane * 2 > (uint64_t) free_b + (uint64_t) sc->ws.capacity * per_lane) p.batch = std::max<uint64_t>(1, (p.batch / 2) / p.lanes_per_row) * p.lanes_per_row;
        }
    }
    // Pipeline.  "fused" runs occlusion + continuation traversal inside the shade kernel (one kernel per bounce, and the first-bounce kernel running up to four
    // iterations with the path state in registers), "split" runs k_trace -> k_shade -> k_shadow per bounce.  Automatic: fused unless large meshes sit behind their own
    // BLAS -- deep per-mesh traversals diverge inside the fat shade kernel (mesh room, 522 k triangles: 19.8 ms fused vs 16.1 ms split; 18 k triangles still run faster
    // fused, 11.2 vs 12.1 ms, 132 k do not, 16.1 vs 13.7 ms) -- or reflectances are textured (6.7 vs 5.8 ms).  Everything else measured faster fused once the fused
    // kernels were capped at 168 VGPRs = 3 waves / SIMD (512 x 512 x 64: Cornell boxes 5.26 -> 4.60 ms, area light 7.12 -> 6.13, sphere light 6.42 -> 4.83,
    // disk 5.30 -> 3.90, Domino 1024 x 1024 x 128 with its 1 025 instances 69.5 -> 62.2 ms; profiles/r02_pipeline_choice.txt).
    p.fused = env_pipeline == "split" ? false : env_pipeline == "fused" ? true : t.blas_triangles <= 32768 && sc->host.textures.empty();
    rp.has_area = t.surface_emitters;   // area emitters make the emitter-hit term (and the last iteration) live
    rp.has_spec = t.has_spec; rp.has_tris = t.has_tris; rp.has_analytic = t.has_analytic ? 1 : 0;
    if (t.has_env) { rp.has_env = 1; rp.env_index = t.env_index; }
    // valid_ray leaves the kernels only when somebody reads it: the alpha channel of an rgba film (integrator.cpp:528-533) and the lane dumps
    rp.want_valid = (rq.lane_dump || se.alpha) ? 1 : 0;
    rp.hide_emitters = sc->pp.hide_emitters;
    rp.n_tlas_nodes = t.n_tlas_nodes; rp.has_nodes16 = t.has_nodes16; rp.has_blas = t.has_blas;   // deep per-mesh traversals diverge: see ray_shape() in dtof_kernels.hip
    // the eight-wave ray kernels of scenes with a BLAS and no analytic shape can run as a pair of launches, with 20 bytes per lane of lists
    if (!(t.has_blas && t.has_nodes16 && !t.has_analytic)) ls.defer = 0;
    // the instance memo, the flat table and what the table proves (flat_choice)
    const FlatChoice fc = flat_choice(t, p.fused, on("DTOF_INSTANCE_MEMO"), on("DTOF_FLAT"));
    rp.memo_obj = fc.memo_obj; rp.flat_objects = fc.flat_objects; rp.flat_off = t.flat_off;
    p.one_wall = (fc.facts & kFactOneWall) != 0; p.flat_shape = fc.facts & kFlatShapeFields;
    // Resident stage of the fused first-bounce kernel (k_shade<..., RESW>): scenes whose blob is too large to stage whole but whose TLAS (at most kResidentNodes nodes,
    // twice that as half-float planes, no per-mesh BLAS) and small records fit one CU's LDS beside the stack columns -- Domino: 1 024 nodes, one shared 12-triangle cube.
    // Waves: 16 (128 VGPRs) beat 12 once the nodes come from LDS, K = 4 too (Domino 44.2 vs 47.8 ms, C5 181.0 vs 192.7; profiles/r03_resident_stage_ab.txt,
    // r04_domino_waves_batch.txt); the every-BSDF kernels hold more state: 12 for one film, 8 for four (profiles/r03_resident_spec_waves.txt).
    const int waves = env_resident ? atoi(env_resident) : (rp.has_spec ? (rp.n_offsets > 1 ? 8 : 12) : 16);
    if (p.fused && (waves == 8 || waves == 12 || waves == 16) && rp.has_tris && !rp.has_blas && t.resident_layout &&
        (t.n_nodes <= kResidentNodes || (on("DTOF_RESIDENT_HALF") && t.has_nodes16 && t.n_nodes <= 2 * kResidentNodes))) {
        p.resident.small_off = t.small_off; p.resident.small_words = t.small_words; p.resident.waves = (uint32_t) waves;
        rp.res_half = t.n_nodes > kResidentNodes ? 1u : 0u;
        // the stage must fit the CU's LDS beside the stack columns (a deep TLAS needs many): fewer waves per block while it does not, none if 8 do not either
        const uint32_t limit = device_lds_limit();
        while (p.resident.waves && resident_lds(rp, p.resident, t.stack_depth, p.resident.waves).bytes() > limit) p.resident.waves = p.resident.waves > 8 ? p.resident.waves - 4 : 0;
        p.resident.n_cu = device_cu_count();
    }
    // the 16-bit traversal of the resident kernels (dtof_traverse.h: NOBLAS, encode_child16) holds for these scenes only
    if (p.resident.waves && rp.has_blas) throw std::runtime_error("internal error: the resident stage was chosen for a scene with a per-mesh BLAS");
    if (p.resident.waves && (rp.res_half || rp.n_offsets > 1) && t.n_objects >= 0x7fff)
        throw std::runtime_error("internal error: the resident stage with 16-bit child references was chosen for a scene of " + std::to_string(t.n_objects) + " objects");
    // Without surface emitters the last iteration contributes nothing and is skipped -- unless further passes follow, whose streams depend on the six draws every
    // active lane makes in it -- and unless a path can still be invalid when it gets there: a null lobe leaves valid_ray unset, and a non-null vertex of the last
    // iteration sets it (dopplertofpath.cpp:252-253), which decides whether the path returns what it gathered or 0 (:279-282); the alpha channel / the lane dump's
    // `valid` likewise depend on the hit of that iteration when max_depth is 1
    p.skip_tail = !t.surface_emitters && p.n_passes == 1 && !t.null_lobe && !rp.want_valid;
    // The terminal form of the last iteration that runs (k_shade: RenderParams::terminal) drops what only a continued path would read.  Eligible: a single pass (the
    // streams of a finished path are carried into the next pass otherwise) and no null lobe in the scene -- a null sample of that iteration would leave valid_ray unset,
    // which decides between the path's result and 0 and is what the alpha film / the lane dump's `valid` show; without one every vertex validates its path, so the
    // terminal form writes valid_out = 1 where want_valid asks for it.  The survivor count of that iteration is not consumed either: the statistics read a count only
    // as the input of the NEXT iteration, and no queue is compacted for a launch that does not happen.
    p.terminal_ok = on("DTOF_TERMINAL_SKIP") && p.n_passes == 1 && !t.null_lobe;
    // kernels compiled with the plan's constants: which facts hold is decided per launch (FramePlan::launch_facts); no result depends on the switch
    p.plan_facts = on("DTOF_PLAN_FACTS"); p.n_emitters = bh_emitters(*sc); p.id_shift = sc->id_shift;
    rp.emitter_pmf = bh_emitters(*sc) ? 1.f / (float) bh_emitters(*sc) : 0.f;   // m_emitter_pmf (scene.cpp:96)
    // fused pipeline: the first bounce kernel generates the lanes and traces the primary rays itself
    p.first_inline = p.fused && rp.integrator != INTEGRATOR_VELOCITY && p.iteration_runs(0) && on("DTOF_FUSE_FIRST");
    if (rq.aov) p.first_inline = false;   // k_aov reads the camera rays k_generate writes: the fused first-bounce kernel is never involved
    // exactly one wave per pixel, one film: measured (profiles/r04_fused_splat_ab.txt) -- with more waves per pixel (C3: 256 spp) or four films (C5) the separate
    // splat kernel, which sums 8 samples per lane before it reduces, is faster
    p.fuse_splat_ok = on("DTOF_FUSE_SPLAT") && p.fused && !rq.lane_dump && p.n_passes == 1 && !se.alpha && rp.filter == FILTER_TENT && rp.filter_radius <= 1.f &&
                      rp.filter_radius > .5f && rp.spp_log2 == 6 && rp.n_offsets == 1 && rq.film != nullptr;
    if (rq.film64 || rq.moments || rq.aov) p.fuse_splat_ok = false;   // the float64 film and the moment film are the separate splat stage's: k_shade splats in float32
    return p;
}

// The wavefront loop of one call: the plan's batches, each through the bounce loop, accumulated into rq.film.
void render_rows(dtof_scene *sc, const RenderRequest &rq) {
    if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
    ensure_device(sc);
    const FramePlan p = plan_frame(sc, rq);
    sc->last_plan_facts = 0;
    RenderParams rp = p.rp;
    dtof_render_stats *const stats = rq.stats;
    const Queues q = sc->ws.prepare((uint32_t) p.batch, rp.n_offsets, rp.want_valid, p.launch.defer != 0, sc->id_shift);
    if (rq.lane_dump) sc->ws.dbg.ensure(p.batch);
    const hipStream_t s = sc->stream;
    const uint8_t *blob = sc->d_blob.p; const uint32_t blob_bytes = (uint32_t) sc->blob.size(), stack_depth = p.traits.stack_depth;
    StageTimer tm(stats != nullptr, sc);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (stats) { memset(stats, 0, sizeof *stats); ev0 = sc->take_event(); ev1 = sc->take_event(); HIP_CHECK(hipEventRecord(ev0, s)); }
    std::vector<uint32_t> batch_lanes, batch_iters, batch_inline;   // batch_inline: iterations the first-bounce launch of the batch covered (fused pipeline)
    // per-iteration totals of every batch: sized ONCE (DevBuf::ensure reallocates without copying, and a hipFree in the middle of the frame would also synchronise the device)
    if (stats && !rq.deferred && p.last > p.first) sc->d_sums.ensure((size_t) ((p.last - p.first + p.batch - 1) / p.batch) * p.run_passes * 2 * kMaxIter);
    if (p.n_passes > 1 && p.last > p.first) {   // stream states carried from pass to pass (Sampler::advance keeps the RNGs running, sampler.cpp:52-55)
        sc->d_pass_rng.ensure((size_t) (p.last - p.first) * 3);
        rp.pass_rng = sc->d_pass_rng.p; rp.pass_first = (uint32_t) p.first;
    }
    const bool velocity = rp.integrator == INTEGRATOR_VELOCITY;
    // An aov call runs k_aov where the integrator would run.  The integrator itself still runs in every pass that another pass follows: a later pass draws its lanes
    // from the streams the paths of the earlier one left behind (Sampler::advance, sampler.cpp:52-55), and the lanes of an aov render are the scene integrator's own.
    const bool aov = rq.aov != nullptr;
    // The host runs at most two batches ahead of the device: dtof_cancel (Integrator::cancel, integrator.h:96-109) is looked at when a
    // batch is enqueued, so an unbounded run-ahead would leave nothing to cancel once the launches of a long render are queued.
    hipEvent_t batch_done[2] = { sc->take_event(), sc->take_event() };
    uint32_t batch_index = 0;
    for (uint32_t pass = 0; pass < p.run_passes; ++pass)
    for (uint64_t b0 = p.first; b0 < p.last; b0 += p.batch, ++batch_index) {
        rp.pass = pass;
        const bool dump_now = rq.lane_dump && pass == p.dump_pass;
        if (batch_index >= 2) HIP_CHECK(hipEventSynchronize(batch_done[batch_index & 1]));
        if (sc->stop.load()) break;
        rp.lane_base = (uint32_t) b0; rp.n_lanes = (uint32_t) std::min<uint64_t>(p.batch, p.last - b0);
        const uint32_t n_seg = segments_for(rp.n_lanes);
        int t = -1;
        if (rp.want_valid && !velocity && !p.iteration_runs(0)) HIP_CHECK(hipMemsetAsync(q.valid_out, 0, (size_t) rp.n_lanes * sizeof(float4), s));   // max_depth == 0: { 0, false } (dopplertofpath.cpp:87-88)
        if (!p.first_inline) {
            t = tm.begin(kStageGenerate, s); launch_generate(rp, q, s); tm.end(kStageGenerate, t, s);
            if (dump_now) launch_lane_dump_rays(rp, q, sc->ws.dbg.p, s);
        }
        const uint32_t *qin = nullptr, *count_in = nullptr; uint32_t it = 0;
        bool fused_splat_done = false;   // the first-bounce kernel of this batch splatted its lanes itself
        const bool integrate = !aov || (p.n_passes > 1 && pass + 1 < p.run_passes);
        if (aov && (!rq.lane_dump || dump_now)) {   // before the shade loop of a multi-pass render overwrites the camera rays
            AovArgs a = *rq.aov;
            if (a.values) a.values += (size_t) (b0 - p.first) * a.n_channels;
            t = tm.begin(kStageTrace, s); launch_aov(blob, blob_bytes, rp, q, a, stack_depth, p.launch, s); tm.end(kStageTrace, t, s);
        }
        if (velocity && !aov) { t = tm.begin(kStageTrace, s); launch_velocity(blob, blob_bytes, rp, q, stack_depth, p.launch, s); tm.end(kStageTrace, t, s); }
        for (; !velocity && integrate && p.iteration_runs(it); ++it) {
            if (it >= 8 && (it & 3) == 0) {   // unbounded depth: stop once every segment has drained
                std::vector<uint32_t> alive(n_seg);
                HIP_CHECK(hipMemcpyAsync(alive.data(), count_in, (size_t) n_seg * 4, hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                uint64_t sum = 0; for (uint32_t v : alive) sum += v;
                if (sum == 0) break;
            }
            const bool first = p.first_inline && it == 0;
            const LaunchSpan l = p.launch_span(it, first, n_seg);
            rp.inline_iters = l.span; rp.chunk_blocks = l.chunk_blocks; rp.res_units = l.res_units; rp.terminal = l.terminal ? 1 : 0;
            it += l.span - 1;   // `it` is now the last iteration this launch covers
            if (l.chunk_blocks > 1 || (l.res_units > 1 && l.resident)) HIP_CHECK(hipMemsetAsync(q.counts, 0, (size_t) 2 * (it + 1) * n_seg * 4, s));
            if (!p.fused || (it == 0 && !first)) { t = tm.begin(kStageTrace, s); launch_trace(blob, blob_bytes, rp, q, qin, count_in, stack_depth, p.launch, s); tm.end(kStageTrace, t, s); if (stats) stats->n_launches_trace++; }
            // per-iteration count slots; beyond kMaxIter iterations (unbounded depth, paths that russian roulette keeps alive that long)
            // the slots are reused -- only the statistics lose those iterations, no path is cut short
            uint32_t *qout = q.q[it & 1], *alive_out = q.counts + (size_t) (2 * (it % kMaxIter)) * n_seg, *shadow_out = alive_out + n_seg;
            const Stage st_shade = first ? kStageFirst : kStageShade;
            t = tm.begin(st_shade, s);
            ShadeRequest sr;
            sr.scene = blob; sr.scene_bytes = blob_bytes; sr.stack_depth = stack_depth; sr.rp = &rp; sr.q = &q; sr.switches = &p.launch; sr.stream = s;
            sr.qin = qin; sr.count_in = count_in; sr.qout = qout; sr.alive_out = alive_out; sr.shadow_out = shadow_out;
            sr.depth = it + 1 - l.span; sr.mode = first ? 2 : p.fused ? 1 : 0; sr.trace_next = l.next_runs; sr.resident = l.resident ? &p.resident : nullptr;
            sr.dbg = first && dump_now ? sc->ws.dbg.p : nullptr; sr.film = l.splat_here ? rq.film : nullptr; sr.film_stride = rq.film_stride;
            sr.facts = p.launch_facts(rp, l, sr.depth, first, qin == nullptr && count_in == nullptr, dump_now);
            const uint32_t specialised = launch_shade(sr);   // the mask of the kernel compiled with plan facts that ran, if one did
            tm.end(st_shade, t, s);
            if (specialised) { sc->plan_facts_launches++; sc->last_plan_facts = specialised; if (stats) stats->n_plan_facts_launches++; }
            fused_splat_done |= l.splat_here;
            if (stats && l.splat_here) stats->n_fused_splat_launches++;
            if (stats && first) { stats->n_launches_first++; stats->n_inline_iterations += l.span; batch_inline.push_back(l.span); }
            if (!p.fused) { t = tm.begin(kStageShadow, s); launch_shadow(blob, blob_bytes, rp, q, shadow_out, stack_depth, p.launch, s); tm.end(kStageShadow, t, s); if (stats) stats->n_launches_shadow++; }
            if (stats) stats->n_launches_shade++;
            qin = qout; count_in = alive_out;
        }
        if (p.n_passes > 1 && pass + 1 < p.run_passes) launch_pass_save(rp, q, s);
        if (dump_now) {
            launch_lane_dump(rp, q, sc->ws.dbg.p, s);
            HIP_CHECK(hipMemcpyAsync(rq.lane_dump + (b0 - p.first), sc->ws.dbg.p, (size_t) rp.n_lanes * sizeof(LaneDebug), hipMemcpyDeviceToHost, s));
            if (rq.lane_planes)   // every film's record of the batch's lanes, as the splat kernels would read them
                for (int k = 0; k < rp.n_offsets; ++k)
                    HIP_CHECK(hipMemcpyAsync(rq.lane_planes + (size_t) k * rq.dump_n + (b0 - p.first), q.res + (size_t) k * q.capacity, (size_t) rp.n_lanes * sizeof(float4), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        } else if (!rq.lane_dump && !fused_splat_done && !aov) {
            t = tm.begin(kStageSplat, s);
            if (rq.moments) launch_splat_moments(rp, q, rq.moments, s);
            else if (rq.film64) launch_splat_f64(rp, q, rq.film64, rq.film64_stride, s); else launch_splat(rp, q, rq.film, rq.film_stride, p.launch, s);
            if (sc->host.sensor.alpha && !rq.moments) {   // the alpha film (plane K behind the K offset films): the same splat over (valid, 0, 0) -- ImageBlock::put of aovs[3] (integrator.cpp:528-533)
                RenderParams ra = rp; ra.n_offsets = 1;
                Queues qa = q; qa.res = q.valid_out;
                if (rq.film64) launch_splat_f64(ra, qa, rq.film64 + (size_t) rp.n_offsets * rq.film64_stride, rq.film64_stride, s);
                else launch_splat(ra, qa, rq.film + (size_t) rp.n_offsets * rq.film_stride, rq.film_stride, p.launch, s);
            }
            tm.end(kStageSplat, t, s);
        }
        HIP_CHECK(hipGetLastError());   // a rejected launch (LDS size, launch bounds, grid) must not pass for an empty film
        HIP_CHECK(hipEventRecord(batch_done[batch_index & 1], s));
        if (stats) {   // per-iteration totals of this batch are reduced on the device; one small copy after the last batch
            const uint32_t it_counted = std::min<uint32_t>(it, kMaxIter);
            if (it_counted && !rq.deferred) launch_sum_counts(q.counts, n_seg, 2 * it_counted, sc->d_sums.p + (size_t) batch_index * 2 * kMaxIter, s);
            batch_lanes.push_back(rp.n_lanes); batch_iters.push_back(it_counted);
            stats->n_batches++;
        }
    }
    if (stats && rq.deferred) {
        HIP_CHECK(hipEventRecord(ev1, s));
        dtof_scene::DeferredFrame f; f.ev0 = ev0; f.ev1 = ev1; f.counters = *stats;
        for (int k = 0; k < kStageCount; ++k) f.ev[k] = tm.ev[k];
        for (uint32_t b : batch_lanes) f.counters.n_paths += b;
        sc->deferred.push_back(std::move(f));
        if (sc->stop.load()) throw std::runtime_error("cancelled");
        return;
    }
    if (stats) {
        HIP_CHECK(hipEventRecord(ev1, s)); HIP_CHECK(hipEventSynchronize(ev1));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1)); stats->ms_total = ms;
        std::vector<unsigned long long> sums(batch_lanes.size() * 2 * (size_t) kMaxIter);
        if (!sums.empty()) HIP_CHECK(hipMemcpy(sums.data(), sc->d_sums.p, sums.size() * 8, hipMemcpyDeviceToHost));
        std::vector<uint64_t> h_counts;
        for (size_t b = 0; b < batch_lanes.size(); ++b)
            for (uint32_t i = 0; i < 2 * batch_iters[b]; ++i) h_counts.push_back(sums[b * 2 * kMaxIter + i]);
        stats->ms_generate = stage_ms(tm.ev[kStageGenerate]); stats->ms_trace = stage_ms(tm.ev[kStageTrace]); stats->ms_first = stage_ms(tm.ev[kStageFirst]);
        stats->ms_shade = stage_ms(tm.ev[kStageShade]) + stats->ms_first; stats->ms_shadow = stage_ms(tm.ev[kStageShadow]); stats->ms_splat = stage_ms(tm.ev[kStageSplat]);
        size_t off = 0;
        for (size_t b = 0; b < batch_lanes.size(); ++b) {
            stats->n_paths += batch_lanes[b];
            uint64_t in = batch_lanes[b];
            for (uint32_t i = 0; i < batch_iters[b]; ++i) {
                stats->n_bounces += in; stats->n_shadow_rays += h_counts[off + 2 * i + 1];
                if (b < batch_inline.size() && i < batch_inline[b]) stats->n_bounces_inline += in;
                in = h_counts[off + 2 * i];
            }
            off += 2 * (size_t) batch_iters[b];
        }
    } else {
        HIP_CHECK(hipStreamSynchronize(s));
    }
    if (sc->stop.load()) throw std::runtime_error("cancelled");
}

// The device-film entry points: the null and stripe checks, the caller's film layout, and for the async forms the events a refused frame took go back to the pool
void render_device_film(dtof_scene *sc, RenderRequest rq) {
    if (!sc || !rq.film) throw std::runtime_error("null argument");
    if (rq.stripes) {
        if (rq.row_begin < 0 || rq.stripe_rows <= 0 || rq.stripe_period < rq.stripe_rows) throw std::runtime_error("invalid stripe layout");
        rq.row_end = sc->host.sensor.crop_h;
    }
    sc->stop = false;
    const std::pair<int32_t, int32_t> rows = rq.stripes ? stripe_span(sc, rq.row_begin, rq.stripe_rows, rq.stripe_period) : std::make_pair(rq.row_begin, rq.row_end);
    rq.film_stride = caller_film_stride(sc, rq.films(), rows.first, rows.second);
    dtof_render_stats local;
    if (rq.deferred) rq.stats = &local;
    try { render_rows(sc, rq); }
    catch (...) { if (rq.deferred && sc->deferred.empty()) sc->events_used = 0; throw; }
}

// The variants arguments of the C ABI as a request carries them: NULL / 0 = the integrator's own pair; the count is checked here, before anything is enqueued
void set_variants(RenderRequest &rq, const dtof_modulation *variants, int n_variants) {
    if (!variants || n_variants <= 0) return;
    if (n_variants > kMaxOffsets) throw std::runtime_error("at most 4 modulation variants can be batched per traversal");
    rq.variants = variants; rq.n_variants = n_variants;
}

// The host-buffer renders (dtof_render_offsets / _variants): the library's own film of rq.films() colour planes (and the alpha plane), developed into out_rgb
void render_host_films(dtof_scene *sc, RenderRequest rq, float *out_rgb) {
    if (!sc || !out_rgb) throw std::runtime_error("null argument");
    if (sc->pp.integrator != INTEGRATOR_DOPPLER && rq.n_variants > 0) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");   // before the film is cleared
    ensure_device(sc);
    sc->stop = false;
    const int k = rq.films();
    const HostSensor &se = sc->host.sensor;
    size_t px = (size_t) se.crop_w * se.crop_h;
    const int planes = k + (se.alpha ? 1 : 0), ch = se.alpha ? 4 : 3;   // rgba: one more film plane for the alpha channel, four channels out
    sc->d_film.ensure(px * 4 * planes); sc->d_rgb.ensure(px * ch * k);
    HIP_CHECK(hipMemsetAsync(sc->d_film.p, 0, px * 4 * planes * sizeof(float), sc->stream));
    rq.row_begin = 0; rq.row_end = se.crop_h;
    rq.film = sc->d_film.p; rq.film_stride = px * 4;   // the library's own film
    render_rows(sc, rq);
    if (se.alpha) for (int i = 0; i < k; ++i) launch_develop_rgba(sc->d_film.p + px * 4 * i, sc->d_film.p + px * 4 * k, sc->d_rgb.p + px * 4 * i, (int64_t) px, sc->stream);
    else launch_develop(sc->d_film.p, sc->d_rgb.p, (int64_t) px * k, sc->stream);
    HIP_CHECK(hipMemcpyAsync(out_rgb, sc->d_rgb.p, px * ch * k * sizeof(float), hipMemcpyDeviceToHost, sc->stream));
    HIP_CHECK(hipStreamSynchronize(sc->stream));
}

// render_host_films with the library's own FLOAT64 film (dtof_render_variants_f64): developed in double into out_rgb; out_films: the raw film planes, or null
void render_host_films_f64(dtof_scene *sc, RenderRequest rq, float *out_rgb, double *out_films) {
    if (!sc || !out_rgb) throw std::runtime_error("null argument");
    if (sc->pp.integrator != INTEGRATOR_DOPPLER && rq.n_variants > 0) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");
    if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
    ensure_device(sc);
    sc->stop = false;
    const int k = rq.films();
    const HostSensor &se = sc->host.sensor;
    const size_t px = (size_t) se.crop_w * se.crop_h;
    const int planes = k + (se.alpha ? 1 : 0), ch = se.alpha ? 4 : 3;
    sc->d_film64.ensure(px * 4 * planes); sc->d_rgb.ensure(px * ch * k);
    HIP_CHECK(hipMemsetAsync(sc->d_film64.p, 0, px * 4 * planes * sizeof(double), sc->stream));
    rq.row_begin = 0; rq.row_end = se.crop_h;
    rq.film = nullptr; rq.film64 = sc->d_film64.p; rq.film64_stride = px * 4;
    render_rows(sc, rq);
    if (se.alpha) for (int i = 0; i < k; ++i) launch_develop_rgba_f64(sc->d_film64.p + px * 4 * i, sc->d_film64.p + px * 4 * k, sc->d_rgb.p + px * 4 * i, (int64_t) px, sc->stream);
    else launch_develop_f64(sc->d_film64.p, k, 0, sc->d_rgb.p, (int64_t) px, sc->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out_rgb, sc->d_rgb.p, px * ch * k * sizeof(float), hipMemcpyDeviceToHost, sc->stream));
    if (out_films) HIP_CHECK(hipMemcpyAsync(out_films, sc->d_film64.p, px * 4 * planes * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
    HIP_CHECK(hipStreamSynchronize(sc->stream));
}

std::map<std::string, std::string> to_map(const char *const *names, const char *const *values, int n) {
    std::map<std::string, std::string> m;
    for (int i = 0; i < n; ++i) m[names[i]] = values[i];
    return m;
}

PropBag make_bag(const char *plugin, const char *const *names, const char *types, const char *const *values, int n) {
    PropBag b; b.plugin = plugin ? plugin : "";
    for (int i = 0; i < n; ++i) {
        PropValue v; std::string val = values[i];
        switch (types[i]) {
            case 'f': v.type = PropValue::Float; v.f = std::stod(val); break;
            case 'i': v.type = PropValue::Int; v.i = std::stoll(val); break;
            case 'b': v.type = PropValue::Bool; if (val != "true" && val != "false") throw std::runtime_error("could not parse boolean value \"" + val + "\""); v.b = val == "true"; break;
            case 's': v.type = PropValue::String; v.s = val; break;
            default: throw std::runtime_error(std::string("unknown property type '") + types[i] + "'");
        }
        b.values[names[i]] = v;
    }
    return b;
}

dtof_scene *finish_scene(HostScene &&hs) {
    auto sc = new dtof_scene();
    try {
        sc->host = std::move(hs);
        if (!sc->host.has_sensor && sc->host.sampler.plugin.empty()) sc->host.sampler.plugin = "independent";   // no sensor, no sampler: Sensor's default (sensor.cpp:63-66)
        sc->pp = make_plugin_params(sc->host.integrator, sc->host.sampler);
        {   // the hit record packs (object, shape in its group) into 32 bits (Queues::hit_id): the object index gets 24 bits unless a shapegroup
            // needs more than the remaining 8 for its shapes; 0xffffffff stays free as the "miss" value
            uint32_t max_shapes = 1; for (auto &g : sc->host.groups) max_shapes = std::max(max_shapes, g.n_shapes);
            uint32_t shape_bits = 0; while ((1ull << shape_bits) < max_shapes) ++shape_bits;
            uint32_t obj_bits = 1; while ((1ull << obj_bits) < sc->host.objects.size() + 1ull) ++obj_bits;
            if (obj_bits + shape_bits > 31) throw std::runtime_error("too many scene objects / shapes per shapegroup: object index and shape index must fit 31 bits together");
            sc->id_shift = shape_bits <= 8 && obj_bits <= 24 ? 24 : 31 - shape_bits;
        }
        sc->blob = build_scene_blob(sc->host);
    } catch (...) { delete sc; throw; }
    return sc;
}

}  // namespace

// ================================================================================ C ABI
extern "C" {

const char *dtof_version(void) { return "dtof 0.1 (HIP, gfx950; dopplertofpath + correlated)"; }
const char *dtof_last_error(void) { return g_last_error.c_str(); }

int dtof_scene_load_string(const char *xml, const char *const *pn, const char *const *pv, int n, dtof_scene **out) {
    return guarded([&] {
        if (!xml || !out) throw std::runtime_error("null argument");
        *out = finish_scene(load_scene_xml(xml, to_map(pn, pv, n)));
    });
}
int dtof_scene_load_file(const char *path, const char *const *pn, const char *const *pv, int n, dtof_scene **out) {
    return guarded([&] {
        if (!path || !out) throw std::runtime_error("null argument");
        std::string p = path, dir = ".";
        size_t k = p.find_last_of('/'); if (k != std::string::npos) dir = k ? p.substr(0, k) : "/";
        *out = finish_scene(load_scene_xml(read_file(path), to_map(pn, pv, n), dir));
    });
}
void dtof_scene_destroy(dtof_scene *scene) { delete scene; }

int dtof_scene_set_integrator(dtof_scene *sc, const char *plugin, const char *const *names, const char *types, const char *const *values, int n) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null scene");
        PropBag b = make_bag(plugin, names, types, values, n);
        PluginParams p = make_plugin_params(b, sc->host.sampler);
        sc->host.integrator = b; sc->pp = p;
    });
}
int dtof_scene_set_sampler(dtof_scene *sc, const char *plugin, const char *const *names, const char *types, const char *const *values, int n) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null scene");
        PropBag b = make_bag(plugin, names, types, values, n);
        PluginParams p = make_plugin_params(sc->host.integrator, b);
        sc->host.sampler = b; sc->pp = p;
    });
}

struct dtof_integrator { PropBag bag; };
struct dtof_sampler_plugin { PropBag bag; };
static PropBag default_sampler_bag() { PropBag b; b.plugin = "correlated"; return b; }
static PropBag default_integrator_bag() { PropBag b; b.plugin = "dopplertofpath"; return b; }
int dtof_integrator_create(const char *plugin, const char *const *names, const char *types, const char *const *values, int n, dtof_integrator **out) {
    return guarded([&] {
        if (!out) throw std::runtime_error("null argument");
        PropBag b = make_bag(plugin, names, types, values, n);
        (void) make_plugin_params(b, default_sampler_bag());   // the constructor's checks (names, types, value ranges)
        *out = new dtof_integrator { b };
    });
}
void dtof_integrator_destroy(dtof_integrator *i) { delete i; }
int dtof_sampler_plugin_create(const char *plugin, const char *const *names, const char *types, const char *const *values, int n, dtof_sampler_plugin **out) {
    return guarded([&] {
        if (!out) throw std::runtime_error("null argument");
        PropBag b = make_bag(plugin, names, types, values, n);
        (void) make_plugin_params(default_integrator_bag(), b);
        *out = new dtof_sampler_plugin { b };
    });
}
void dtof_sampler_plugin_destroy(dtof_sampler_plugin *s) { delete s; }
int dtof_integrator_render(const dtof_integrator *integ, const dtof_sampler_plugin *smp, dtof_scene *sc, uint32_t sensor_index,
                           uint32_t seed, uint32_t spp, float *out_rgb, dtof_render_stats *stats) {
    int rc = guarded([&] {
        if (!integ || !sc) throw std::runtime_error("null argument");
        const PropBag &sb = smp ? smp->bag : sc->host.sampler;
        PluginParams p = make_plugin_params(integ->bag, sb);
        sc->host.integrator = integ->bag; sc->host.sampler = sb; sc->pp = p;
    });
    return rc ? rc : dtof_render(sc, sensor_index, seed, spp, out_rgb, stats);
}

int dtof_scene_get_info(const dtof_scene *sc, dtof_scene_info *info) {
    return guarded([&] {
        if (!sc || !info) throw std::runtime_error("null argument");
        const HostSensor &se = sc->host.sensor; const PluginParams &p = sc->pp;
        const BlobHeader *h = (const BlobHeader *) sc->blob.data();
        memset(info, 0, sizeof *info);
        info->film_width = se.film_w; info->film_height = se.film_h; info->crop_x = se.crop_x; info->crop_y = se.crop_y;
        info->crop_width = se.crop_w; info->crop_height = se.crop_h; info->sample_count = p.sample_count;
        info->n_shapes = h->n_shapes; info->n_groups = h->n_groups; info->n_objects = h->n_objects; info->n_emitters = h->n_emitters;
        info->n_triangles = h->n_tris; info->n_bvh_nodes = h->n_nodes; info->scene_blob_bytes = h->total_bytes;
        info->time = p.time; info->w_g = p.w_g_mhz; info->g_1 = p.g_1; info->g_0 = p.g_0; info->w_s = p.w_s_mhz;
        info->phase_offset = p.phase_offset; info->hetero_frequency = p.hetero_frequency; info->antithetic_shift = p.antithetic_shift;
        info->wave_type = p.wave_type; info->low_frequency_component_only = p.low_frequency_component_only;
        info->time_sampling = p.time_sampling; info->stratify_each_interval = p.stratify_each_interval;
        info->path_correlation_depth = p.path_correlation_depth; info->max_depth = p.max_depth; info->rr_depth = p.rr_depth;
        info->base_seed = p.base_seed; info->time_correlate_number = p.time_correlate_number; info->path_correlate_number = p.path_correlate_number;
        info->bvh_stack_depth = h->tlas_depth;
        info->filter_radius = se.filter_radius;
        info->filter_halo = se.filter == FILTER_BOX ? 0 : (int32_t) std::ceil(se.filter_radius - .5f);
        info->has_alpha = se.alpha ? 1 : 0;
    });
}

int dtof_scene_export(const dtof_scene *sc, int kind, float *out, size_t cap, size_t *n_written) {
    return guarded([&] {
        if (!sc || !n_written) throw std::runtime_error("null argument");
        std::vector<float> v;
        if (kind == 0) for (auto &o : sc->host.objects) {
            v.push_back(o.key_time[0]); v.push_back(o.key_time[1]);
            v.insert(v.end(), o.key[0], o.key[0] + 16); v.insert(v.end(), o.key[1], o.key[1] + 16);
        } else if (kind == 1) for (auto &s : sc->host.shapes) {
            v.insert(v.end(), s.to_world, s.to_world + 16); v.insert(v.end(), s.to_object, s.to_object + 16);
        } else if (kind == 2) {
            const HostSensor &s = sc->host.sensor;
            v.insert(v.end(), s.to_world, s.to_world + 16);
            v.push_back(s.x_fov); v.push_back(s.near_clip); v.push_back(s.far_clip); v.push_back(s.shutter_open); v.push_back(s.shutter_close);
            v.push_back(s.orthographic ? 2.f : s.thinlens ? 1.f : 0.f); v.push_back(s.aperture_radius); v.push_back(s.focus_distance);
        } else if (kind == 3) for (auto &e : sc->host.emitters) {
            v.insert(v.end(), e.pos, e.pos + 3); v.insert(v.end(), e.intensity, e.intensity + 3);
        } else if (kind >= 4 && kind <= 7) for (auto &s : sc->host.shapes) {
            if (s.kind != SHAPE_MESH) continue;
            if (kind == 4) v.insert(v.end(), s.positions.begin(), s.positions.end());
            else if (kind == 5) v.insert(v.end(), s.normals.begin(), s.normals.end());
            else if (kind == 6) v.insert(v.end(), s.texcoords.begin(), s.texcoords.end());
            else for (uint32_t f : s.faces) { float b; memcpy(&b, &f, 4); v.push_back(b); }
        } else if (kind == 8) for (auto &s : sc->host.shapes) {
            if (s.kind != SHAPE_SPHERE) continue;
            v.insert(v.end(), s.center, s.center + 3); v.push_back(s.radius); v.push_back(s.sphere_inv_area); v.push_back(s.flip_normals ? 1.f : 0.f);
        } else if (kind == 9) for (auto &s : sc->host.shapes) {
            v.push_back((float) s.bsdf); v.push_back(s.twosided ? 1.f : 0.f); v.push_back(s.diel_eta); v.push_back(s.nonlinear ? 1.f : 0.f);
            v.push_back(s.inv_eta_2); v.push_back(s.fdr_int); v.push_back(s.spec_sampling_weight);
            v.insert(v.end(), s.refl, s.refl + 3); v.insert(v.end(), s.spec_refl, s.spec_refl + 3); v.insert(v.end(), s.spec_trans, s.spec_trans + 3);
            v.insert(v.end(), s.cond_eta, s.cond_eta + 3); v.insert(v.end(), s.cond_k, s.cond_k + 3); v.push_back(s.alpha_u); v.push_back(s.alpha_v);
        } else if (kind == 13) for (auto &t : sc->host.textures) {
            v.push_back((float) t.kind); v.push_back((float) t.filter); v.push_back((float) t.wrap); v.push_back((float) t.channels);
            v.push_back((float) t.width); v.push_back((float) t.height);
            v.insert(v.end(), t.to_uv, t.to_uv + 4); v.insert(v.end(), t.color0, t.color0 + 3); v.insert(v.end(), t.color1, t.color1 + 3); v.push_back(t.mean);
        } else if (kind == 14) for (auto &t : sc->host.textures) v.insert(v.end(), t.data.begin(), t.data.end());
        else if (kind == 15) for (auto &s : sc->host.shapes) v.push_back((float) s.tex_refl);
        else if (kind == 17) for (auto &s : sc->host.shapes) v.push_back(s.sample_all ? 1.f : 0.f);
        else if (kind == 19) for (auto &s : sc->host.shapes) { v.push_back((float) s.tex_spec); v.push_back((float) s.tex_trans); v.push_back((float) s.tex_alpha_u); v.push_back((float) s.tex_alpha_v); }   // textures on the other slots: indices into the texture table, -1 = none
        else if (kind == 20) for (auto &s : sc->host.shapes) { v.push_back(s.masked ? 1.f : 0.f); v.push_back(s.opacity); v.push_back((float) s.tex_opacity); }   // mask: masked, opacity, its texture
        else if (kind == 21) for (auto &s : sc->host.shapes) v.push_back((float) s.tex_normal);   // normalmap / bumpmap: its texture, -1 = none
        else if (kind == 22) for (auto &s : sc->host.shapes) { v.push_back(s.bumpmap ? 1.f : 0.f); v.push_back(s.bump_scale); }   // bumpmap: is one, scale
        else if (kind == 24) for (auto &s : sc->host.shapes) v.push_back((float) s.tex_radiance);   // texture on the area emitter's radiance, -1 = a constant
        else if (kind == 25) {   // the flat table's shading frames as packed into the blob, with the shape constants they were computed from
            const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
            if (bh->off_flat) {
                const DFlatObject *fo = (const DFlatObject *) (sc->blob.data() + bh->off_flat);
                const DFlatFrame *fr = (const DFlatFrame *) ((const uint8_t *) (fo + bh->n_objects) + sizeof(DFlatKinds) + (size_t) bh->n_objects * sizeof(DFlatZ));
                const DObject *ob = (const DObject *) (sc->blob.data() + bh->off_objects);
                const DShape *shp = (const DShape *) (sc->blob.data() + bh->off_shapes);
                const DGroup *grp = (const DGroup *) (sc->blob.data() + bh->off_groups);
                for (uint32_t i = 0; i < bh->n_objects; ++i) {
                    const DShape &d = shp[fo[i].instance ? grp[ob[i].index].first_shape : ob[i].index];   // an instance: the first shape of its group
                    v.push_back((float) fo[i].instance); v.insert(v.end(), d.n, d.n + 3); v.insert(v.end(), d.dp_du, d.dp_du + 3);
                    v.insert(v.end(), fr[i].s, fr[i].s + 3); v.insert(v.end(), fr[i].t, fr[i].t + 3);
                }
            }
        }
        else if (kind == 26) {   // the flat table's facts as a frame plan takes them (automatic pipeline, default switches): kFactOneWall holds, a shape is known, its object count, its wall index
            const SceneTraits t = scene_traits(*sc);
            const FlatChoice c = flat_choice(t, t.blas_triangles <= 32768 && sc->host.textures.empty(), true, true);
            v.push_back((c.facts & kFactOneWall) ? 1.f : 0.f); v.push_back((c.facts & kFactFlatShape) ? 1.f : 0.f); v.push_back((float) flat_shape_count(c.facts)); v.push_back((float) flat_shape_wall(c.facts));
        }
        else if (kind == 23) for (auto &s : sc->host.shapes) {   // blendbsdf: is one, weight, its texture, kind and two-sidedness of bsdf_1
            v.push_back(s.blend_other ? (s.two_bsdfs ? 2.f : 1.f) : 0.f); v.push_back(s.blend_weight); v.push_back((float) s.tex_blend);   // 1 blendbsdf, 2 twosided with two BSDFs
            v.push_back(s.blend_other ? (float) s.blend_other->bsdf : -1.f); v.push_back(s.blend_other && s.blend_other->twosided ? 1.f : 0.f);
        }
        else if (kind == 18) for (auto &e : sc->host.emitters) {   // every emitter: kind, pos, intensity, first row of to_local (directional: its direction)
            v.push_back((float) e.kind); v.insert(v.end(), e.pos, e.pos + 3); v.insert(v.end(), e.intensity, e.intensity + 3); v.insert(v.end(), e.to_local, e.to_local + 3);
        }
        else if (kind == 16) {   // the environment map as packed into the blob: header words, m_data, then every level of the hierarchical warp
            const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
            const DEmitter *de = (const DEmitter *) (sc->blob.data() + bh->off_emitters);
            for (uint32_t i = 0; i < bh->n_emitters; ++i) if (de[i].kind == EMITTER_ENVMAP) {
                const DEnvmap *e = (const DEnvmap *) (sc->blob.data() + de[i].shape);
                v.push_back((float) e->w); v.push_back((float) e->h); v.push_back((float) e->n_levels); v.push_back(e->scale);
                v.insert(v.end(), de[i].pos, de[i].pos + 3); v.push_back(de[i].cutoff_angle);
                v.insert(v.end(), e->to_world, e->to_world + 12); v.insert(v.end(), de[i].to_local, de[i].to_local + 12);
                const float *d = (const float *) (sc->blob.data() + e->data_off);
                v.insert(v.end(), d, d + (size_t) e->w * e->h * 3);
                for (uint32_t k = 0; k < e->n_levels; ++k) {
                    const uint32_t end = k + 1 < e->n_levels ? e->level_off[k + 1] : bh->total_bytes;
                    const float *lv = (const float *) (sc->blob.data() + e->level_off[k]);
                    size_t count = k == 0 ? (size_t) e->w * e->h : 0;
                    if (k > 0) { uint32_t lx = e->w - 1, ly = e->h - 1; for (uint32_t j = 1; j <= k; ++j) { lx += lx & 1u; ly += ly & 1u; if (j < k) { lx >>= 1; ly >>= 1; } } count = (size_t) lx * ly; }
                    (void) end;
                    v.push_back((float) e->level_w[k]); v.push_back((float) count);
                    v.insert(v.end(), lv, lv + count);
                }
            }
        }
        else if (kind == 12) for (auto &s : sc->host.shapes) {
            v.push_back(s.beckmann ? 0.f : 1.f);
        } else if (kind == 10) for (auto &s : sc->host.shapes) {
            if (s.bsdf == BSDF_ROUGHPLASTIC) v.insert(v.end(), s.rough_table.begin(), s.rough_table.end());
        } else if (kind == 11) for (auto &e : sc->host.emitters) {
            if (e.kind != EMITTER_SPOT) continue;
            v.insert(v.end(), e.pos, e.pos + 3); v.insert(v.end(), e.intensity, e.intensity + 3); v.insert(v.end(), e.to_local, e.to_local + 12);
            v.push_back(e.cutoff_angle); v.push_back(e.cos_cutoff); v.push_back(e.cos_beam); v.push_back(e.inv_transition);
        } else throw std::runtime_error("unknown export kind");
        *n_written = v.size();
        if (out) { if (v.size() > cap) throw std::runtime_error("export buffer too small"); memcpy(out, v.data(), v.size() * 4); }
    });
}

int dtof_render_rows(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                     const float *offsets, int n_offsets, float *d_film, dtof_render_stats *stats) {
    RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = row_begin; rq.row_end = row_end;
    rq.offsets = offsets; rq.n_offsets = n_offsets; rq.film = d_film; rq.stats = stats;
    return guarded([&] { render_device_film(sc, rq); });
}

int dtof_render_rows_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end, const float *offsets, int n_offsets, float *d_film) {
    RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = row_begin; rq.row_end = row_end;
    rq.offsets = offsets; rq.n_offsets = n_offsets; rq.film = d_film; rq.deferred = true;
    return guarded([&] { render_device_film(sc, rq); });
}
int dtof_scene_set_film_layout(dtof_scene *sc, int32_t planes, uint64_t plane_stride_floats) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null scene");
        if (planes < 0) throw std::runtime_error("negative plane count");
        const HostSensor &se = sc->host.sensor;
        if (plane_stride_floats != 0 && (plane_stride_floats % 4 != 0 || plane_stride_floats < (uint64_t) se.crop_w * 4))
            throw std::runtime_error("plane stride must be a multiple of 4 floats and at least one film row");
        sc->film_planes = planes; sc->film_plane_stride = plane_stride_floats;
    });
}
int dtof_scene_set_stream(dtof_scene *sc, void *hip_stream) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null scene");
        if (!sc->deferred.empty()) throw std::runtime_error("frames are still in flight on the current stream: call dtof_async_collect first");
        ensure_device(sc);
        // nothing of ours is left behind on the stream we leave.  A FOREIGN stream may already be gone (the caller's torch stream was collected before it handed the stream
        // back): no frame is in flight on it (checked above), so a failing wait there means a dead handle, not lost work -- fall through to the new stream
        if (hipStreamSynchronize(sc->stream) != hipSuccess) {
            (void) hipGetLastError();
            if (sc->stream == sc->own_stream) throw std::runtime_error("hipStreamSynchronize failed on the scene's own stream");
        }
        sc->stream = hip_stream ? (hipStream_t) hip_stream : sc->own_stream;
    });
}
int dtof_render_stripes_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                              const float *offsets, int n_offsets, float *d_film) {
    RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = first_row; rq.stripes = true; rq.stripe_rows = stripe_rows; rq.stripe_period = stripe_period;
    rq.offsets = offsets; rq.n_offsets = n_offsets; rq.film = d_film; rq.deferred = true;
    return guarded([&] { render_device_film(sc, rq); });
}
int dtof_clear_async(dtof_scene *sc, void *d_ptr, size_t bytes) {
    return guarded([&] {
        if (!sc || !d_ptr) throw std::runtime_error("null argument");
        ensure_device(sc);
        HIP_CHECK(hipMemsetAsync(d_ptr, 0, bytes, sc->stream));
    });
}
int dtof_develop_async(dtof_scene *sc, const float *d_film, float *d_rgb, int64_t n_pixels) {
    return guarded([&] {
        if (!sc || !d_film || !d_rgb) throw std::runtime_error("null argument");
        ensure_device(sc);
        launch_develop(d_film, d_rgb, n_pixels, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
// one finished deferred frame added to a statistics block (its stream has been waited for); returns the frame's duration
static float add_deferred_frame(dtof_render_stats *sum, const dtof_scene::DeferredFrame &f) {
    float t = 0; HIP_CHECK(hipEventElapsedTime(&t, f.ev0, f.ev1));
    sum->ms_total += t;
    sum->ms_generate += stage_ms(f.ev[kStageGenerate]); sum->ms_trace += stage_ms(f.ev[kStageTrace]); sum->ms_first += stage_ms(f.ev[kStageFirst]);
    sum->ms_shade += stage_ms(f.ev[kStageShade]) + stage_ms(f.ev[kStageFirst]); sum->ms_shadow += stage_ms(f.ev[kStageShadow]); sum->ms_splat += stage_ms(f.ev[kStageSplat]);
    sum->n_paths += f.counters.n_paths; sum->n_batches += f.counters.n_batches;
    sum->n_launches_trace += f.counters.n_launches_trace; sum->n_launches_shade += f.counters.n_launches_shade; sum->n_launches_shadow += f.counters.n_launches_shadow;
    sum->n_launches_first += f.counters.n_launches_first; sum->n_inline_iterations += f.counters.n_inline_iterations; sum->n_fused_splat_launches += f.counters.n_fused_splat_launches; sum->n_plan_facts_launches += f.counters.n_plan_facts_launches;
    return t;
}
int dtof_async_collect(dtof_scene *sc, dtof_render_stats *sum, double *frame_ms, uint32_t capacity, uint32_t *n_frames) {
    return guarded([&] {
        if (!sc || !sum || !n_frames) throw std::runtime_error("null argument");
        ensure_device(sc);
        HIP_CHECK(hipStreamSynchronize(sc->stream));
        memset(sum, 0, sizeof *sum);
        *n_frames = (uint32_t) sc->deferred.size();
        uint32_t i = 0;
        for (auto &f : sc->deferred) {
            const float t = add_deferred_frame(sum, f);
            if (frame_ms && i < capacity) frame_ms[i] = t;
            ++i;
        }
        sc->deferred.clear(); sc->events_used = 0;
    });
}

// ---------------------------------------------------------------- radial-velocity map (dtof_reconstruct.hip)
// The checks the three entries share, made before a device is touched: a refused call enqueues and writes nothing.
static void check_velocity_scalars(uint32_t n_passes, double exposure_time, double w_g_mhz) {
    if (n_passes == 0) throw std::runtime_error("n_passes must be at least 1");
    if (!std::isfinite(exposure_time) || !(exposure_time > 0)) throw std::runtime_error("exposure_time must be finite and > 0");
    if (!std::isfinite(w_g_mhz) || !(w_g_mhz > 0)) throw std::runtime_error("w_g_mhz must be finite and > 0");
}
static void check_grid(int64_t n_pixels) {   // one lane per pixel in blocks of 256: the block count is a 32-bit grid dimension
    if (n_pixels < 0) throw std::runtime_error("negative pixel count");
    if (n_pixels > (int64_t) 0x7fffffff * 256) throw std::runtime_error("too many pixels for one launch");
}
static VelocityMapArgs velocity_args(int n_pairs, const int32_t *hom, const int32_t *het, uint32_t n_passes, double exposure_time, double w_g_mhz) {
    VelocityMapArgs a; memset(&a, 0, sizeof a);
    a.n_pairs = n_pairs;
    for (int k = 0; k < n_pairs; ++k) {
        if (hom[k] < 0 || hom[k] >= 2 * n_pairs || het[k] < 0 || het[k] >= 2 * n_pairs)
            throw std::runtime_error("pair " + std::to_string(k) + ": plane index outside the " + std::to_string(2 * n_pairs) + " planes of the sum");
        a.hom[k] = hom[k]; a.het[k] = het[k];
    }
    a.n_passes = (float) n_passes; a.exposure_time = (float) exposure_time;
    a.inv_time = 1.0 / exposure_time; a.w_g_hz = w_g_mhz * 1e6; a.conf_floor = 1e-5 * 0.0015;   // in double, once, as Python forms them
    return a;
}

int dtof_develop_accumulate_async(dtof_scene *sc, const float *d_film, int32_t planes, uint64_t plane_stride_floats, float *d_rgb_sum, int64_t n_pixels, int first) {
    return guarded([&] {
        if (!sc || !d_film || !d_rgb_sum) throw std::runtime_error("null argument");
        if (planes < 1 || planes > 65535) throw std::runtime_error("the film must have between 1 and 65535 planes");
        check_grid(n_pixels);
        if (plane_stride_floats != 0 && (plane_stride_floats % 4 != 0 || plane_stride_floats < (uint64_t) n_pixels * 4))
            throw std::runtime_error("plane stride must be a multiple of 4 floats and at least n_pixels * 4");
        if ((uintptr_t) d_film % 16 != 0 || (uintptr_t) d_rgb_sum % 4 != 0) throw std::runtime_error("the film must be 16-byte aligned, the sum 4-byte aligned");
        ensure_device(sc);
        launch_develop_accumulate(d_film, planes, plane_stride_floats, d_rgb_sum, n_pixels, first != 0, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
int dtof_velocity_map_async(dtof_scene *sc, const float *d_rgb_sum, int n_pairs, const int32_t *homodyne_planes, const int32_t *heterodyne_planes, uint32_t n_passes,
                            double exposure_time, double w_g_mhz, int64_t n_pixels, float *d_tof, double *d_velocity_pairs, double *d_velocity) {
    return guarded([&] {
        if (!sc || !d_rgb_sum || !homodyne_planes || !heterodyne_planes || !d_velocity) throw std::runtime_error("null argument");
        if (n_pairs < 1 || n_pairs > kMaxVelocityPairs) throw std::runtime_error("between 1 and 16 (homodyne, heterodyne) pairs can be combined");
        check_velocity_scalars(n_passes, exposure_time, w_g_mhz);
        check_grid(n_pixels);
        if ((uintptr_t) d_rgb_sum % 4 != 0 || (uintptr_t) d_tof % 4 != 0 || (uintptr_t) d_velocity_pairs % 8 != 0 || (uintptr_t) d_velocity % 8 != 0)
            throw std::runtime_error("misaligned buffer");
        const VelocityMapArgs a = velocity_args(n_pairs, homodyne_planes, heterodyne_planes, n_passes, exposure_time, w_g_mhz);
        ensure_device(sc);
        launch_velocity_map(d_rgb_sum, a, n_pixels, d_tof, d_velocity_pairs, d_velocity, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
int dtof_velocity_map_variants(const float *offsets, int n_offsets, dtof_modulation *out_variants) {
    return guarded([&] {
        if (!offsets || !out_variants) throw std::runtime_error("null argument");
        if (n_offsets < 1 || n_offsets > kMaxVelocityPairs) throw std::runtime_error("between 1 and 16 offsets make a velocity map");
        for (int g = 0; g < n_offsets; g += 2) {   // a homodyne / heterodyne pair never straddles two traversals
            const int n = std::min(2, n_offsets - g);
            for (int j = 0; j < n; ++j) {
                out_variants[2 * g + j] = dtof_modulation { 0.f, offsets[g + j] };
                out_variants[2 * g + n + j] = dtof_modulation { 1.f, offsets[g + j] };
            }
        }
    });
}
// dtof_render_velocity_map / _f64: the same loop over the library's own float32 or float64 film (film64: k_splat_f64 and k_develop_accumulate_f64)
static void velocity_map_render(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                                double *out_velocity, double *out_velocity_pairs, float *out_tof, dtof_render_stats *stats, bool film64) {
    if (!sc || !offsets || !out_velocity) throw std::runtime_error("null argument");
    if (n_offsets < 1 || n_offsets > kMaxVelocityPairs) throw std::runtime_error("between 1 and 16 offsets make a velocity map");
    check_velocity_scalars(n_passes, exposure_time, w_g_mhz);
    if (sc->pp.integrator != INTEGRATOR_DOPPLER) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");
    if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
    dtof_modulation variants[2 * kMaxVelocityPairs];
    if (dtof_velocity_map_variants(offsets, n_offsets, variants) != DTOF_OK) throw std::runtime_error(g_last_error);
    int32_t hom[kMaxVelocityPairs], het[kMaxVelocityPairs];   // offset j of group g = j / 2: its films lie behind the 4 * g planes of the full groups before it
    for (int j = 0; j < n_offsets; ++j) {
        const int g = j / 2, n = std::min(2, n_offsets - 2 * g);
        hom[j] = 4 * g + j % 2; het[j] = 4 * g + n + j % 2;
    }
    const VelocityMapArgs a = velocity_args(n_offsets, hom, het, n_passes, exposure_time, w_g_mhz);
    ensure_device(sc);
    sc->stop = false;
    const HostSensor &se = sc->host.sensor;
    const size_t px = (size_t) se.crop_w * se.crop_h;
    const int alpha = se.alpha ? 1 : 0;
    if (film64) sc->d_film64.ensure(px * 4 * (kMaxOffsets + alpha)); else sc->d_film.ensure(px * 4 * (kMaxOffsets + alpha));   // the library's own film: the caller's declared layout is not consulted
    sc->d_vm_sum.ensure(px * 3 * 2 * n_offsets); sc->d_vm_tof.ensure(px * 2 * n_offsets); sc->d_vm_maps.ensure(px * (n_offsets + 1));
    const hipStream_t s = sc->stream;
    const size_t first_frame = sc->deferred.size();   // frames the caller has not collected yet stay his
    try {
        for (int g = 0; g < n_offsets; g += 2) {
            const int films = 2 * std::min(2, n_offsets - g);
            for (uint32_t pass = 0; pass < n_passes; ++pass) {
                if (film64) HIP_CHECK(hipMemsetAsync(sc->d_film64.p, 0, px * 4 * (films + alpha) * sizeof(double), s));
                else HIP_CHECK(hipMemsetAsync(sc->d_film.p, 0, px * 4 * (films + alpha) * sizeof(float), s));
                dtof_render_stats frame;
                RenderRequest rq; rq.seed = pass; rq.spp = spp; rq.row_begin = 0; rq.row_end = se.crop_h;
                if (film64) { rq.film64 = sc->d_film64.p; rq.film64_stride = px * 4; } else { rq.film = sc->d_film.p; rq.film_stride = px * 4; }
                rq.deferred = true; rq.stats = &frame;
                set_variants(rq, variants + 2 * g, films);
                render_rows(sc, rq);
                // the alpha plane behind them is left out
                if (film64) launch_develop_accumulate_f64(sc->d_film64.p, films, 0, sc->d_vm_sum.p + px * 3 * 2 * g, (int64_t) px, pass == 0, s);
                else launch_develop_accumulate(sc->d_film.p, films, 0, sc->d_vm_sum.p + px * 3 * 2 * g, (int64_t) px, pass == 0, s);
            }
        }
        double *d_pairs = sc->d_vm_maps.p + px;
        launch_velocity_map(sc->d_vm_sum.p, a, (int64_t) px, out_tof ? sc->d_vm_tof.p : nullptr, out_velocity_pairs ? d_pairs : nullptr, sc->d_vm_maps.p, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out_velocity, sc->d_vm_maps.p, px * sizeof(double), hipMemcpyDeviceToHost, s));
        if (out_velocity_pairs) HIP_CHECK(hipMemcpyAsync(out_velocity_pairs, d_pairs, px * n_offsets * sizeof(double), hipMemcpyDeviceToHost, s));
        if (out_tof) HIP_CHECK(hipMemcpyAsync(out_tof, sc->d_vm_tof.p, px * 2 * n_offsets * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        dtof_render_stats sum; memset(&sum, 0, sizeof sum);
        for (size_t i = first_frame; i < sc->deferred.size(); ++i) add_deferred_frame(&sum, sc->deferred[i]);
        if (stats) *stats = sum;
    } catch (...) {   // the frames of this call leave the list either way (their events go back to the pool once no frame is in flight)
        if (sc->deferred.size() > first_frame) { (void) hipStreamSynchronize(s); sc->deferred.resize(first_frame); }
        if (sc->deferred.empty()) sc->events_used = 0;
        throw;
    }
    sc->deferred.resize(first_frame);
    if (sc->deferred.empty()) sc->events_used = 0;
}
int dtof_render_velocity_map(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                             double *out_velocity, double *out_velocity_pairs, float *out_tof, dtof_render_stats *stats) {
    return guarded([&] { velocity_map_render(sc, n_passes, spp, offsets, n_offsets, exposure_time, w_g_mhz, out_velocity, out_velocity_pairs, out_tof, stats, false); });
}

// ---------------------------------------------------------------- float64 film (dtof_film64.hip)
int dtof_render_velocity_map_f64(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                                 double *out_velocity, double *out_velocity_pairs, float *out_tof, dtof_render_stats *stats) {
    return guarded([&] { velocity_map_render(sc, n_passes, spp, offsets, n_offsets, exposure_time, w_g_mhz, out_velocity, out_velocity_pairs, out_tof, stats, true); });
}
int dtof_render_variants_f64(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants, float *out_images, double *out_films,
                             dtof_render_stats *stats) {
    return guarded([&] {
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.stats = stats; set_variants(rq, variants, n_variants);
        render_host_films_f64(sc, rq, out_images, out_films);
    });
}
int dtof_render_rows_variants_f64(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end, const dtof_modulation *variants, int n_variants,
                                  double *d_film, int32_t planes, uint64_t plane_stride_doubles, dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || !d_film) throw std::runtime_error("null argument");
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = row_begin; rq.row_end = row_end; rq.stats = stats;
        set_variants(rq, variants, n_variants);
        if (sc->pp.integrator != INTEGRATOR_DOPPLER && rq.n_variants > 0) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");
        if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
        if ((uintptr_t) d_film % 8 != 0) throw std::runtime_error("the film must be 8-byte aligned");
        const HostSensor &se = sc->host.sensor;
        const int need = rq.films() + (se.alpha ? 1 : 0);   // the alpha film lies behind the colour films
        if (planes < need) throw std::runtime_error("the device film has " + std::to_string(planes) + " planes, this call writes " + std::to_string(need));
        if (plane_stride_doubles != 0 && (plane_stride_doubles % 4 != 0 || plane_stride_doubles < (uint64_t) se.crop_w * 4))
            throw std::runtime_error("plane stride must be a multiple of 4 doubles and at least one film row");
        int32_t lo = 0, hi = 0;
        const uint64_t reach = film_rows_reach(se, row_begin, row_end, &lo, &hi);
        if (need > 1 && plane_stride_doubles != 0 && plane_stride_doubles < reach)
            throw std::runtime_error("the plane stride of " + std::to_string(plane_stride_doubles) + " doubles is smaller than the " + std::to_string(reach) +
                                     " doubles of film rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") this call writes: the planes would overlap");
        rq.film64 = d_film; rq.film64_stride = plane_stride_doubles ? plane_stride_doubles : (uint64_t) se.crop_w * se.crop_h * 4;
        sc->stop = false;
        render_rows(sc, rq);
    });
}

// ---------------------------------------------------------------- moment film (dtof_moments.hip)
int dtof_moment_planes(int n_variants) { return n_variants < 0 || n_variants > kMaxOffsets ? -1 : moment_planes(std::max(n_variants, 1)); }
static void add_stats(dtof_render_stats &sum, const dtof_render_stats &f) {
    sum.n_paths += f.n_paths; sum.n_bounces += f.n_bounces; sum.n_shadow_rays += f.n_shadow_rays;
    sum.ms_total += f.ms_total; sum.ms_generate += f.ms_generate; sum.ms_trace += f.ms_trace; sum.ms_shade += f.ms_shade; sum.ms_shadow += f.ms_shadow; sum.ms_splat += f.ms_splat;
    sum.n_launches_trace += f.n_launches_trace; sum.n_launches_shade += f.n_launches_shade; sum.n_launches_shadow += f.n_launches_shadow; sum.n_batches += f.n_batches;
    sum.n_launches_first += f.n_launches_first; sum.ms_first += f.ms_first; sum.n_inline_iterations += f.n_inline_iterations; sum.n_bounces_inline += f.n_bounces_inline;
    sum.n_fused_splat_launches += f.n_fused_splat_launches; sum.n_plan_facts_launches += f.n_plan_facts_launches;
}
int dtof_render_moments(dtof_scene *sc, uint32_t seed, uint32_t spp, uint32_t n_passes, const dtof_modulation *variants, int n_variants, int developed,
                        double *out_planes, dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || !out_planes) throw std::runtime_error("null argument");
        if (n_passes == 0) throw std::runtime_error("the moment film needs at least one pass");
        if (n_variants < 0 || n_variants > kMaxOffsets) throw std::runtime_error("between 0 and 4 modulation variants make a moment film");
        if (n_variants > 0 && !variants) throw std::runtime_error("null argument: n_variants > 0 without variants");
        if (sc->pp.integrator != INTEGRATOR_DOPPLER && n_variants > 0) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");
        if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
        ensure_device(sc);
        sc->stop = false;
        const HostSensor &se = sc->host.sensor;
        const size_t px = (size_t) se.crop_w * se.crop_h;
        const int planes = moment_planes(std::max(n_variants, 1));
        sc->d_moments.ensure(px * kMomentCell); sc->d_moment_planes.ensure(px * planes);
        const hipStream_t s = sc->stream;
        HIP_CHECK(hipMemsetAsync(sc->d_moments.p, 0, px * kMomentCell * sizeof(double), s));   // once: the raw sums of the passes add up
        dtof_render_stats sum; memset(&sum, 0, sizeof sum);
        for (uint32_t pass = 0; pass < n_passes; ++pass) {
            dtof_render_stats frame;
            RenderRequest rq; rq.seed = seed + pass; rq.spp = spp; rq.row_begin = 0; rq.row_end = se.crop_h; rq.stats = &frame;
            rq.moments = sc->d_moments.p;
            set_variants(rq, variants, n_variants);
            render_rows(sc, rq);
            add_stats(sum, frame);
        }
        launch_develop_moments(sc->d_moments.p, planes, developed != 0, sc->d_moment_planes.p, (int64_t) px, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out_planes, sc->d_moment_planes.p, px * planes * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (stats) *stats = sum;
    });
}

// ---------------------------------------------------------------- geometry channels of the `aov` integrator (dtof_aov.hip)
int dtof_aov_parse(const char *spec, int32_t *types, int capacity, int *n_types, char *names_buf, size_t names_capacity, int *n_channels) {
    return guarded([&] {
        if (!spec) throw std::runtime_error("null argument");
        std::vector<int32_t> t; std::vector<std::string> names;
        parse_aovs(spec, t, names);
        if (n_types) *n_types = (int) t.size();
        if (n_channels) *n_channels = (int) names.size();
        if (types) {
            if (capacity < (int) t.size()) throw std::runtime_error("dtof_aov_parse: the spec has " + std::to_string(t.size()) + " types, the buffer holds " + std::to_string(std::max(capacity, 0)));
            std::copy(t.begin(), t.end(), types);
        }
        if (names_buf) {
            size_t need = 0; for (auto &n : names) need += n.size() + 1;
            if (names_capacity < need) throw std::runtime_error("dtof_aov_parse: the channel names take " + std::to_string(need) + " bytes, the buffer holds " + std::to_string(names_capacity));
            char *w = names_buf;
            for (auto &n : names) { memcpy(w, n.c_str(), n.size() + 1); w += n.size() + 1; }
        }
    });
}
int dtof_scene_get_aovs(const dtof_scene *sc, char *buf, size_t capacity) {
    return guarded([&] {
        if (!sc || !buf) throw std::runtime_error("null argument");
        if (capacity < sc->host.aovs.size() + 1) throw std::runtime_error("dtof_scene_get_aovs: the spec takes " + std::to_string(sc->host.aovs.size() + 1) + " bytes");
        memcpy(buf, sc->host.aovs.c_str(), sc->host.aovs.size() + 1);
    });
}
// the channel table of a call: everything a call can be refused for, before any device call
static AovArgs aov_args(const dtof_scene *sc, const int32_t *types, int n_types) {
    if (!types) throw std::runtime_error("null argument");
    if (n_types < 1) throw std::runtime_error("No AOVs were specified!");
    if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
    AovArgs a; a.film = nullptr; a.values = nullptr; a.n_channels = 0; a.slots[0] = a.slots[1] = a.slots[2] = 0;
    for (int i = 0; i < n_types; ++i) {
        if (types[i] < 0 || types[i] >= kAovTypes) throw std::runtime_error("AOV type " + std::to_string(types[i]) + " is not one of the DTOF_AOV_* constants");
        for (int k = 0; k < kAovTypeChannels[types[i]]; ++k, ++a.n_channels) {
            if (a.n_channels >= (uint32_t) kAovMaxChannels)
                throw std::runtime_error("the aov film holds at most " + std::to_string(kAovMaxChannels) + " channels beside the weight (a pixel is a cell of 32 doubles)");
            a.slots[a.n_channels / kAovSlotsPerWord] |= (uint64_t) (kAovTypeSlot[types[i]] + k) << (5u * (a.n_channels % kAovSlotsPerWord));
        }
    }
    return a;
}
int dtof_render_aovs(dtof_scene *sc, uint32_t seed, uint32_t spp, uint32_t n_passes, const int32_t *types, int n_types, int developed, double *out_planes,
                     dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || !out_planes) throw std::runtime_error("null argument");
        if (n_passes == 0) throw std::runtime_error("the aov film needs at least one pass");
        AovArgs a = aov_args(sc, types, n_types);
        ensure_device(sc);
        sc->stop = false;
        const HostSensor &se = sc->host.sensor;
        const size_t px = (size_t) se.crop_w * se.crop_h;
        const int planes = 1 + (int) a.n_channels;
        sc->d_moments.ensure(px * kMomentCell); sc->d_moment_planes.ensure(px * planes);
        const hipStream_t s = sc->stream;
        HIP_CHECK(hipMemsetAsync(sc->d_moments.p, 0, px * kMomentCell * sizeof(double), s));   // once: the raw sums of the passes add up
        a.film = sc->d_moments.p;
        dtof_render_stats sum; memset(&sum, 0, sizeof sum);
        for (uint32_t pass = 0; pass < n_passes; ++pass) {
            dtof_render_stats frame;
            RenderRequest rq; rq.seed = seed + pass; rq.spp = spp; rq.row_begin = 0; rq.row_end = se.crop_h; rq.stats = &frame; rq.aov = &a;
            render_rows(sc, rq);
            add_stats(sum, frame);
        }
        launch_develop_moments(sc->d_moments.p, planes, developed != 0, sc->d_moment_planes.p, (int64_t) px, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out_planes, sc->d_moment_planes.p, px * planes * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (stats) *stats = sum;
    });
}
int dtof_sample_aov_lanes(dtof_scene *sc, uint32_t seed, uint32_t spp, const int32_t *types, int n_types, uint64_t lane_begin, uint64_t n, float *out_lanes12,
                          float *out_values) {
    return guarded([&] {
        if (!sc || !out_lanes12 || !out_values) throw std::runtime_error("null argument");
        AovArgs a = aov_args(sc, types, n_types);
        ensure_device(sc);
        sc->stop = false;
        if (n == 0) return;
        // the scene integrator's lanes, for their rgb ...
        std::vector<LaneDebug> lanes(n), own(n);
        { RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.lane_dump = own.data(); rq.dump_begin = lane_begin; rq.dump_n = n; render_rows(sc, rq); }
        // ... and the aov kernel's: the sample position, time and camera ray are the ones it read
        DevBuf<float> d_values; d_values.ensure((size_t) n * a.n_channels);
        a.values = d_values.p;
        { RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.lane_dump = lanes.data(); rq.dump_begin = lane_begin; rq.dump_n = n; rq.aov = &a; render_rows(sc, rq); }
        HIP_CHECK(hipMemcpy(out_values, d_values.p, (size_t) n * a.n_channels * sizeof(float), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) { memcpy(out_lanes12 + 12 * i, &lanes[i], 36); memcpy(out_lanes12 + 12 * i + 9, own[i].rgb, 12); }
    });
}

int dtof_develop_f64_async(dtof_scene *sc, const double *d_film64, float *d_rgb, int64_t n_pixels) {
    return guarded([&] {
        if (!sc || !d_film64 || !d_rgb) throw std::runtime_error("null argument");
        check_grid(n_pixels);
        if ((uintptr_t) d_film64 % 8 != 0 || (uintptr_t) d_rgb % 4 != 0) throw std::runtime_error("the film must be 8-byte aligned, the image 4-byte aligned");
        ensure_device(sc);
        launch_develop_f64(d_film64, 1, 0, d_rgb, n_pixels, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
int dtof_develop_rgba_f64_async(dtof_scene *sc, const double *d_film64, const double *d_alpha_film64, float *d_rgba, int64_t n_pixels) {
    return guarded([&] {
        if (!sc || !d_film64 || !d_alpha_film64 || !d_rgba) throw std::runtime_error("null argument");
        check_grid(n_pixels);
        if ((uintptr_t) d_film64 % 8 != 0 || (uintptr_t) d_alpha_film64 % 8 != 0 || (uintptr_t) d_rgba % 16 != 0)
            throw std::runtime_error("the films must be 8-byte aligned, the image 16-byte aligned");
        ensure_device(sc);
        launch_develop_rgba_f64(d_film64, d_alpha_film64, d_rgba, n_pixels, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}

// ---------------------------------------------------------------- denoiser (dtof_denoise.hip)
// every refusal of the two entries (denoise_check, dtof_denoise_args.h), before a device is touched
static DenoiseArgs denoise_args(const float *colour, int n_planes, int32_t width, int32_t height, const double *variance, const float *normal, const float *position,
                                const dtof_denoise_params *p, const double *out_colour, const double *out_variance) {
    DenoiseBuffers b { colour, variance, normal, position, out_colour, out_variance };
    DenoiseArgs a;
    const std::string err = denoise_check(b, n_planes, width, height, p == nullptr, p ? p->levels : 0, p ? p->sigma_normal : 0.0, p ? p->sigma_position : 0.0,
                                          p ? p->sigma_luminance : 0.0, &a);
    if (!err.empty()) throw std::runtime_error("dtof_denoise: " + err);
    return a;
}
int dtof_denoise_async(dtof_scene *sc, const float *d_colour, int n_planes, int32_t width, int32_t height, const double *d_variance, const float *d_normal,
                       const float *d_position, const dtof_denoise_params *params, double *d_out_colour, double *d_out_variance) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null argument");
        const DenoiseArgs a = denoise_args(d_colour, n_planes, width, height, d_variance, d_normal, d_position, params, d_out_colour, d_out_variance);
        ensure_device(sc);
        sc->d_denoise.ensure(denoise_scratch_doubles(a));
        launch_denoise(a, d_colour, d_variance, d_normal, d_position, d_out_colour, d_out_variance, sc->d_denoise.p, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
int dtof_denoise(const float *colour, int n_planes, int32_t width, int32_t height, const double *variance, const float *normal, const float *position,
                 const dtof_denoise_params *params, double *out_colour, double *out_variance) {
    return guarded([&] {
        const DenoiseArgs a = denoise_args(colour, n_planes, width, height, variance, normal, position, params, out_colour, out_variance);
        const size_t n = (size_t) width * height, k = (size_t) n_planes;
        DevBuf<float> d_colour, d_normal, d_position; DevBuf<double> d_variance, d_out_colour, d_out_variance, d_scratch;
        d_colour.ensure(k * n * 3); d_out_colour.ensure(k * n * 3); d_scratch.ensure(denoise_scratch_doubles(a));
        HIP_CHECK(hipMemcpyAsync(d_colour.p, colour, k * n * 3 * sizeof(float), hipMemcpyHostToDevice, nullptr));
        if (variance) { d_variance.ensure(k * n); HIP_CHECK(hipMemcpyAsync(d_variance.p, variance, k * n * sizeof(double), hipMemcpyHostToDevice, nullptr)); }
        if (normal) { d_normal.ensure(n * 3); HIP_CHECK(hipMemcpyAsync(d_normal.p, normal, n * 3 * sizeof(float), hipMemcpyHostToDevice, nullptr)); }
        if (position) { d_position.ensure(n * 3); HIP_CHECK(hipMemcpyAsync(d_position.p, position, n * 3 * sizeof(float), hipMemcpyHostToDevice, nullptr)); }
        if (out_variance) d_out_variance.ensure(k * n);
        launch_denoise(a, d_colour.p, d_variance.p, d_normal.p, d_position.p, d_out_colour.p, d_out_variance.p, d_scratch.p, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out_colour, d_out_colour.p, k * n * 3 * sizeof(double), hipMemcpyDeviceToHost, nullptr));
        if (out_variance) HIP_CHECK(hipMemcpyAsync(out_variance, d_out_variance.p, k * n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
        HIP_CHECK(hipStreamSynchronize(nullptr));
    });
}

int dtof_render_stripes(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                        const float *offsets, int n_offsets, float *d_film, dtof_render_stats *stats) {
    RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = first_row; rq.stripes = true; rq.stripe_rows = stripe_rows; rq.stripe_period = stripe_period;
    rq.offsets = offsets; rq.n_offsets = n_offsets; rq.film = d_film; rq.stats = stats;
    return guarded([&] { render_device_film(sc, rq); });
}

int dtof_develop(const float *d_film, float *d_rgb, int64_t n_pixels) {
    return guarded([&] {
        if (!d_film || !d_rgb) throw std::runtime_error("null argument");
        launch_develop(d_film, d_rgb, n_pixels, nullptr);
        HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(nullptr));
    });
}

int dtof_render_offsets(dtof_scene *sc, uint32_t seed, uint32_t spp, const float *offsets, int n_offsets, float *out_rgb, dtof_render_stats *stats) {
    return guarded([&] {
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.offsets = offsets; rq.n_offsets = n_offsets; rq.stats = stats;
        render_host_films(sc, rq, out_rgb);
    });
}
int dtof_render_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants, float *out_rgb, dtof_render_stats *stats) {
    return guarded([&] {
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.stats = stats; set_variants(rq, variants, n_variants);
        render_host_films(sc, rq, out_rgb);
    });
}
int dtof_render_rows_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                              const dtof_modulation *variants, int n_variants, float *d_film, dtof_render_stats *stats) {
    return guarded([&] {
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = row_begin; rq.row_end = row_end; rq.film = d_film; rq.stats = stats;
        set_variants(rq, variants, n_variants); render_device_film(sc, rq);
    });
}
int dtof_render_rows_variants_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                                    const dtof_modulation *variants, int n_variants, float *d_film) {
    return guarded([&] {
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = row_begin; rq.row_end = row_end; rq.film = d_film; rq.deferred = true;
        set_variants(rq, variants, n_variants); render_device_film(sc, rq);
    });
}
int dtof_render_stripes_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                                 const dtof_modulation *variants, int n_variants, float *d_film, dtof_render_stats *stats) {
    return guarded([&] {
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = first_row; rq.stripes = true; rq.stripe_rows = stripe_rows; rq.stripe_period = stripe_period;
        rq.film = d_film; rq.stats = stats;
        set_variants(rq, variants, n_variants); render_device_film(sc, rq);
    });
}
int dtof_render_stripes_variants_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                                       const dtof_modulation *variants, int n_variants, float *d_film) {
    return guarded([&] {
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = first_row; rq.stripes = true; rq.stripe_rows = stripe_rows; rq.stripe_period = stripe_period;
        rq.film = d_film; rq.deferred = true;
        set_variants(rq, variants, n_variants); render_device_film(sc, rq);
    });
}

int dtof_render(dtof_scene *sc, uint32_t sensor_index, uint32_t seed, uint32_t spp, float *out_rgb, dtof_render_stats *stats) {
    if (sensor_index != 0) { g_last_error = "Scene::render(): sensor index " + std::to_string(sensor_index) + " is out of bounds!"; return DTOF_ERR_INVALID; }
    return dtof_render_offsets(sc, seed, spp, nullptr, 0, out_rgb, stats);
}

void dtof_cancel(dtof_scene *sc) { if (sc) sc->stop = true; }
uint64_t dtof_scene_plan_facts_launches(const dtof_scene *sc) { return sc ? sc->plan_facts_launches : 0; }
uint32_t dtof_scene_last_plan_facts(const dtof_scene *sc) { return sc ? sc->last_plan_facts : 0; }

int dtof_sample_lanes_valid(dtof_scene *sc, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out, uint32_t *valid) {
    return guarded([&] {
        if (!sc || !out) throw std::runtime_error("null argument");
        static_assert(sizeof(LaneDebug) == 52, "LaneDebug is 13 floats");
        sc->stop = false;
        if (n == 0) return;
        std::vector<LaneDebug> lanes(n);
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.lane_dump = lanes.data(); rq.dump_begin = lane_begin; rq.dump_n = n;
        render_rows(sc, rq);
        for (uint64_t i = 0; i < n; ++i) { memcpy(out + 12 * i, &lanes[i], 48); if (valid) valid[i] = lanes[i].valid != 0.f ? 1u : 0u; }
    });
}
int dtof_sample_lanes_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants,
                               uint64_t lane_begin, uint64_t n, float *out, uint32_t *valid, float *out_rgb) {
    return guarded([&] {
        if (!sc || !out || !out_rgb) throw std::runtime_error("null argument");
        RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.dump_begin = lane_begin; rq.dump_n = n;
        set_variants(rq, variants, n_variants);
        if (sc->pp.integrator != INTEGRATOR_DOPPLER && rq.n_variants > 0) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");
        sc->stop = false;
        if (n == 0) return;
        std::vector<LaneDebug> lanes(n);
        std::vector<float4> planes((size_t) rq.films() * n);
        rq.lane_dump = lanes.data(); rq.lane_planes = planes.data();
        render_rows(sc, rq);
        for (uint64_t i = 0; i < n; ++i) { memcpy(out + 12 * i, &lanes[i], 48); if (valid) valid[i] = lanes[i].valid != 0.f ? 1u : 0u; }
        for (size_t i = 0; i < planes.size(); ++i) { out_rgb[3 * i] = planes[i].x; out_rgb[3 * i + 1] = planes[i].y; out_rgb[3 * i + 2] = planes[i].z; }
    });
}
int dtof_sample_lanes(dtof_scene *sc, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out) {
    return dtof_sample_lanes_valid(sc, seed, spp, lane_begin, n, out, nullptr);
}
int dtof_develop_on_stream(const float *d_film, float *d_rgb, int64_t n_pixels, void *hip_stream) {
    return guarded([&] {
        if (!d_film || !d_rgb) throw std::runtime_error("null argument");
        launch_develop(d_film, d_rgb, n_pixels, (hipStream_t) hip_stream);
        HIP_CHECK(hipGetLastError());
    });
}
int dtof_develop_rgba(const float *d_film, const float *d_alpha_film, float *d_rgba, int64_t n_pixels) {
    return guarded([&] {
        if (!d_film || !d_alpha_film || !d_rgba) throw std::runtime_error("null argument");
        launch_develop_rgba(d_film, d_alpha_film, d_rgba, n_pixels, nullptr);
        HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(nullptr));
    });
}

// ---------------------------------------------------------------- sampler
static RenderParams sampler_params(const dtof_sampler *s) {
    RenderParams rp; memset(&rp, 0, sizeof rp);
    rp.base_seed = s->base_seed; rp.seed = s->seed; rp.seed_value = s->base_seed + s->seed;
    rp.spp = s->spw; rp.tcn = (uint32_t) s->tcn; rp.pcn = (uint32_t) s->pcn;
    rp.n_stratum = s->sample_count / (uint32_t) s->tcn;
    rp.inv_n_stratum = rp.n_stratum ? 1.0f / (float) (int) rp.n_stratum : 0.f;
    rp.inv_tcn = 1.0f / (float) s->tcn;
    rp.d_spp = make_fastdiv(rp.spp); rp.d_tcn = make_fastdiv(rp.tcn); rp.d_pcn = make_fastdiv(rp.pcn); rp.d_stratum = make_fastdiv(rp.n_stratum);
    rp.d_w = make_fastdiv(1); rp.n_passes = 1;
    return rp;
}
static SamplerState sampler_state(dtof_sampler *s) {
    SamplerState st; st.rng = s->rng.p; st.rng_time = s->rng_time.p; st.rng_path = s->rng_path.p; st.perm_seed = s->perm.p; st.dim = s->dim.p; st.n = s->wavefront;
    return st;
}
static void need_seeded(const dtof_sampler *s) { if (!s) throw std::runtime_error("null sampler"); if (!s->seeded) throw std::runtime_error("sampler is not seeded"); }

int dtof_sampler_create(uint32_t sample_count, uint32_t base_seed, int32_t tcn, int32_t pcn, dtof_sampler **out) {
    return guarded([&] {
        if (!out) throw std::runtime_error("null argument");
        if (tcn <= 0 || pcn <= 0) throw std::runtime_error("correlate numbers must be positive");
        auto s = new dtof_sampler(); s->sample_count = sample_count; s->base_seed = base_seed; s->tcn = tcn; s->pcn = pcn;
        *out = s;
    });
}
void dtof_sampler_destroy(dtof_sampler *s) { delete s; }
int dtof_sampler_set_samples_per_wavefront(dtof_sampler *s, uint32_t spw) {
    return guarded([&] {
        if (!s) throw std::runtime_error("null sampler");
        if (spw == 0 || s->sample_count % spw != 0) throw std::runtime_error("sample_count should be a multiple of samples_per_wavefront!");
        s->spw = spw;
    });
}
int dtof_sampler_seed(dtof_sampler *s, uint32_t seed, uint32_t wavefront_size) {
    return guarded([&] {
        if (!s) throw std::runtime_error("null sampler");
        if (wavefront_size == 0xffffffffu) { if (s->wavefront == 0) throw std::runtime_error("Sampler::seed(): wavefront_size should be specified!"); }
        else s->wavefront = wavefront_size;
        s->seed = seed; s->sample_index = 0;
        uint32_t n = s->wavefront;
        s->rng.ensure(n); s->rng_time.ensure(n); s->rng_path.ensure(n); s->perm.ensure(n); s->dim.ensure(n); s->out.ensure(2 * (size_t) n); s->flags.ensure(n);
        launch_sampler_seed(sampler_params(s), sampler_state(s), nullptr);
        HIP_CHECK(hipGetLastError()); HIP_CHECK(hipDeviceSynchronize());
        s->seeded = true;
    });
}
int dtof_sampler_advance(dtof_sampler *s) {
    return guarded([&] { need_seeded(s); s->sample_index++; HIP_CHECK(hipMemset(s->dim.p, 0, (size_t) s->wavefront * 4)); });
}
static void sampler_draw(dtof_sampler *s, const uint8_t *correlate, int all, int mode, float *out, int stride, int offset) {
    uint32_t n = s->wavefront;
    if (correlate) HIP_CHECK(hipMemcpy(s->flags.p, correlate, n, hipMemcpyHostToDevice));
    if (mode == 0) launch_sampler_next_1d(sampler_params(s), sampler_state(s), s->out.p, nullptr);
    else launch_sampler_next_correlate(sampler_params(s), sampler_state(s), correlate ? s->flags.p : nullptr, all, s->out.p, nullptr);
    HIP_CHECK(hipGetLastError());
    std::vector<float> tmp(n);
    HIP_CHECK(hipMemcpy(tmp.data(), s->out.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) out[(size_t) i * stride + offset] = tmp[i];
}
int dtof_sampler_next_1d(dtof_sampler *s, float *out) { return guarded([&] { need_seeded(s); sampler_draw(s, nullptr, 0, 0, out, 1, 0); }); }
int dtof_sampler_next_2d(dtof_sampler *s, float *out) {
    return guarded([&] { need_seeded(s); sampler_draw(s, nullptr, 0, 0, out, 2, 0); sampler_draw(s, nullptr, 0, 0, out, 2, 1); });
}
int dtof_sampler_next_1d_correlate(dtof_sampler *s, const uint8_t *c, int all, float *out) {
    return guarded([&] { need_seeded(s); sampler_draw(s, c, all, 1, out, 1, 0); });
}
int dtof_sampler_next_2d_correlate(dtof_sampler *s, const uint8_t *c, int all, float *out) {
    return guarded([&] { need_seeded(s); sampler_draw(s, c, all, 1, out, 2, 0); sampler_draw(s, c, all, 1, out, 2, 1); });
}
int dtof_sampler_next_1d_time(dtof_sampler *s, int strategy, float shift, int stratify, float *out) {
    return guarded([&] {
        need_seeded(s);
        if (strategy < 0 || strategy > TIME_REGULAR) throw std::runtime_error("unknown time sampling strategy");
        if (strategy == TIME_ANTITHETIC_MIRROR && s->tcn != 2)   // Assert(m_time_correlate_number == 2), correlated.cpp:142
            throw std::runtime_error("antithetic_mirror time sampling needs time_correlate_number == 2");
        if (strategy != TIME_UNIFORM && stratify && s->sample_count < (uint32_t) s->tcn)
            throw std::runtime_error("sample count must be at least time_correlate_number when per-interval stratification is on");
        RenderParams rp = sampler_params(s); rp.time_sampling = strategy; rp.antithetic_shift = shift; rp.stratify = stratify;
        launch_sampler_next_time(rp, sampler_state(s), s->sample_index * s->spw, s->out.p, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, s->out.p, (size_t) s->wavefront * 4, hipMemcpyDeviceToHost));
    });
}
int dtof_sampler_get_state(dtof_sampler *s, uint32_t *out7) {
    return guarded([&] {
        need_seeded(s);
        uint32_t n = s->wavefront; std::vector<uint2> a(n), b(n), c(n); std::vector<uint32_t> p(n);
        HIP_CHECK(hipMemcpy(a.data(), s->rng.p, (size_t) n * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(b.data(), s->rng_time.p, (size_t) n * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(c.data(), s->rng_path.p, (size_t) n * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(p.data(), s->perm.p, (size_t) n * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t *o = out7 + 7 * (size_t) i;
            o[0] = a[i].x; o[1] = a[i].y; o[2] = b[i].x; o[3] = b[i].y; o[4] = c[i].x; o[5] = c[i].y; o[6] = p[i];
        }
    });
}
// Sampler::fork (correlated.cpp:25-32: same configuration, fresh unseeded state) and Sampler::clone (:34-36: same configuration AND
// the current per-lane state: three PCG streams, permutation seed, dimension / sample index)
int dtof_sampler_fork(const dtof_sampler *s, dtof_sampler **out) {
    return guarded([&] {
        if (!s || !out) throw std::runtime_error("null argument");
        auto f = new dtof_sampler(); f->sample_count = s->sample_count; f->base_seed = s->base_seed; f->tcn = s->tcn; f->pcn = s->pcn;
        *out = f;
    });
}
int dtof_sampler_clone(const dtof_sampler *s, dtof_sampler **out) {
    return guarded([&] {
        if (!s || !out) throw std::runtime_error("null argument");
        std::unique_ptr<dtof_sampler> c(new dtof_sampler());
        c->sample_count = s->sample_count; c->base_seed = s->base_seed; c->tcn = s->tcn; c->pcn = s->pcn;
        c->seed = s->seed; c->wavefront = s->wavefront; c->spw = s->spw; c->sample_index = s->sample_index; c->seeded = s->seeded;
        if (s->seeded) {
            const size_t n = s->wavefront;
            c->rng.ensure(n); c->rng_time.ensure(n); c->rng_path.ensure(n); c->perm.ensure(n); c->dim.ensure(n); c->out.ensure(2 * n); c->flags.ensure(n);
            HIP_CHECK(hipMemcpy(c->rng.p, s->rng.p, n * 8, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(c->rng_time.p, s->rng_time.p, n * 8, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(c->rng_path.p, s->rng_path.p, n * 8, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(c->perm.p, s->perm.p, n * 4, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(c->dim.p, s->dim.p, n * 4, hipMemcpyDeviceToDevice));
        }
        *out = c.release();
    });
}
int dtof_sampler_set_sample_count(dtof_sampler *s, uint32_t spp) {   // Sampler::set_sample_count (sampler.h:129)
    return guarded([&] {
        if (!s) throw std::runtime_error("null sampler");
        if (spp == 0 || spp % s->spw != 0) throw std::runtime_error("sample_count should be a multiple of samples_per_wavefront!");
        s->sample_count = spp;
    });
}
int dtof_sampler_seeded(const dtof_sampler *s) { return s && s->seeded ? 1 : 0; }   // Sampler::seeded (sampler.h:141)
uint32_t dtof_sampler_wavefront_size(const dtof_sampler *s) { return s ? s->wavefront : 0; }
uint32_t dtof_sampler_sample_count(const dtof_sampler *s) { return s ? s->sample_count : 0; }

int dtof_eval_modulation(dtof_scene *sc, int mode, const float *t, const float *len, float *out, uint32_t n) {
    return guarded([&] {
        if (!sc || !t || !out || (mode == 0 && !len)) throw std::runtime_error("null argument");
        if (mode < 0 || mode > 2) throw std::runtime_error("unknown mode");
        RenderParams rp = make_params(sc, 0, sc->pp.sample_count ? sc->pp.sample_count : 1, nullptr, 0);
        DevBuf<float> dt, dl, dout; dt.ensure(n); dl.ensure(n); dout.ensure(n);
        HIP_CHECK(hipMemcpy(dt.p, t, (size_t) n * 4, hipMemcpyHostToDevice));
        if (len) HIP_CHECK(hipMemcpy(dl.p, len, (size_t) n * 4, hipMemcpyHostToDevice));
        launch_waveform_eval(rp, dt.p, dl.p, dout.p, mode, n, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    });
}

int dtof_eval_component(int component, const float *params, int n_params, const float *in, int in_stride, float *out, int out_stride, uint32_t n) {
    return guarded([&] {
        if ((!in || !out) && n) throw std::runtime_error("null argument");
        if (component < 0 || component >= COMP_COUNT) throw std::runtime_error("unknown component");
        if (n_params < 0 || n_params > 8 || (n_params && !params)) throw std::runtime_error("a component takes at most 8 parameters");
        static const int need_in[COMP_COUNT] = { 3, 6, 6, 5, 1, 1, 1, 2, 2, 2, 2, 3, 2, 1 }, need_out[COMP_COUNT] = { 1, 1, 1, 4, 4, 1, 1, 3, 2, 2, 3, 6, 1, 1 };
        static const int need_par[COMP_COUNT] = { 4, 4, 4, 4, 1, 2, 5, 0, 0, 0, 0, 0, 0, 1 };
        if (in_stride < need_in[component] || out_stride < need_out[component] || n_params < need_par[component])
            throw std::runtime_error("strides / parameter count too small for this component");
        int dev_count = 0;
        if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) { (void) hipGetLastError(); throw HipError("hipGetDeviceCount: no ROCm-capable device is detected"); }
        ComponentArgs a; memset(&a, 0, sizeof a);
        a.component = component; a.in_stride = in_stride; a.out_stride = out_stride; a.n = n;
        for (int i = 0; i < n_params; ++i) a.p[i] = params[i];
        RenderParams rp; memset(&rp, 0, sizeof rp);
        if (component == COMP_RFILTER) {
            const int kind = (int) a.p[0];
            if (kind < FILTER_BOX || kind > FILTER_LANCZOS || !(a.p[1] > 0.f)) throw std::runtime_error("unknown filter / non-positive radius");
            set_filter(rp, kind, a.p[1], a.p[2], a.p[3], a.p[4]);
        }
        DevBuf<float> din, dout; din.ensure((size_t) n * in_stride); dout.ensure((size_t) n * out_stride);
        HIP_CHECK(hipMemcpy(din.p, in, (size_t) n * in_stride * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(dout.p, 0, (size_t) n * out_stride * 4));
        a.in = din.p; a.out = dout.p;
        launch_component(a, rp, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t) n * out_stride * 4, hipMemcpyDeviceToHost));
    });
}

int dtof_bsdf_eval_ex(dtof_scene *sc, uint32_t shape_index, int spec, uint32_t n, const float *in29, float *out14) {
    return guarded([&] {
        if (!sc || (n && (!in29 || !out14))) throw std::runtime_error("null argument");
        const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
        if (shape_index >= bh->n_shapes) throw std::runtime_error("shape index out of range");
        if (spec == -1) spec = scene_traits(*sc).has_spec;
        // the instantiations the render path can run on this shape: a scene's SPEC is at least what each of its shapes needs (scene_traits)
        const DShape &sh = ((const DShape *) (sc->blob.data() + bh->off_shapes))[shape_index];
        const bool two_records = sh.flags & (SF_BLEND | SF_TWOSIDED2);
        const bool plain_diffuse = sh.bsdf == BSDF_DIFFUSE && !two_records && !(sh.flags & (SF_MASK | SF_NORMALMAP | SF_BUMPMAP)) && !(sh.nonlinear >> 1);
        if (spec < 0 || spec > 2) throw std::runtime_error("dtof_bsdf_eval_ex: spec must be -1, 0, 1 or 2");
        if (spec == 0 && !plain_diffuse) throw std::runtime_error("dtof_bsdf_eval_ex: the SPEC = 0 kernels run on untextured (twosided) diffuse shapes only");
        if (spec == 1 && two_records) throw std::runtime_error("dtof_bsdf_eval_ex: a blendbsdf / two-BSDF twosided runs in the SPEC = 2 kernels only");
        ensure_device(sc);
        DevBuf<float> din, dout; din.ensure((size_t) n * 29); dout.ensure((size_t) n * 14);
        HIP_CHECK(hipMemcpy(din.p, in29, (size_t) n * 29 * 4, hipMemcpyHostToDevice));
        (spec == 0 ? launch_bsdf_eval_0 : spec == 1 ? launch_bsdf_eval_1 : launch_bsdf_eval_2)(sc->d_blob.p, shape_index, din.p, dout.p, n, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out14, dout.p, (size_t) n * 56, hipMemcpyDeviceToHost));
    });
}
int dtof_bsdf_eval(dtof_scene *sc, uint32_t shape_index, uint32_t n, const float *in11, float *out14) {
    // the flat local frame of the reference's BSDF unit tests, spec = 2
    std::vector<float> in29;
    if (in11 && n) {
        static const float flat[18] = { 1, 0, 0,  0, 1, 0,  0, 0, 1,  1, 0, 0,  0, 1, 0,  0, 0, 1 };   // dp_du, dp_dv, n, sh_s, sh_t, sh_n
        in29.resize((size_t) n * 29);
        for (size_t i = 0; i < n; ++i) { memcpy(&in29[i * 29], in11 + i * 11, 44); memcpy(&in29[i * 29 + 11], flat, sizeof flat); }
    }
    return dtof_bsdf_eval_ex(sc, shape_index, 2, n, in29.empty() ? nullptr : in29.data(), out14);
}
int dtof_emitter_eval(dtof_scene *sc, int mode, int level, int32_t shape_or_minus1, uint32_t n, const float *in, float *out) {
    return guarded([&] {
        if (!sc || (n && (!in || !out))) throw std::runtime_error("null argument");
        if (mode < 0 || mode > 2) throw std::runtime_error("dtof_emitter_eval: mode must be 0 (sample), 1 (hit) or 2 (miss)");
        const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
        const DShape *shapes = (const DShape *) (sc->blob.data() + bh->off_shapes);
        const DEmitter *emitters = (const DEmitter *) (sc->blob.data() + bh->off_emitters);
        const SceneTraits t = scene_traits(*sc);
        if (level == -1) level = t.has_spec ? 3 + t.has_spec : t.has_tris ? (t.surface_emitters ? 3 : 2) : (t.surface_emitters ? 1 : 0);   // what render_rows launches
        if (level < 0 || level > 6) throw std::runtime_error("dtof_emitter_eval: level must be -1 or 0 .. 6");
        const bool area = level == 1 || (level >= 3 && level != 6), mesh = level >= 2 && level != 6, spec = level == 4 || level == 5;
        // the levels the render path could run on this scene (scene_traits, render_rows)
        bool points_only = true, points_and_plain_rects = true, plain = true;
        for (uint32_t i = 0; i < bh->n_emitters; ++i) {
            const DEmitter &em = emitters[i];
            points_only &= em.kind == EMITTER_POINT;
            if (em.kind == EMITTER_AREA) {
                if (em.shape >= bh->n_shapes) throw std::runtime_error("dtof_emitter_eval: an emitter's shape index is out of range");
                points_and_plain_rects &= shapes[em.shape].kind == SHAPE_RECT && !shapes[em.shape].tex_radiance;
                plain &= !shapes[em.shape].tex_radiance;
            } else if (em.kind != EMITTER_POINT) points_and_plain_rects = plain = false;
        }
        if (!area && !spec && !points_only) throw std::runtime_error("dtof_emitter_eval: the kernels without area emitters run on scenes with point emitters only");
        if (area && !mesh && !spec && !points_and_plain_rects) throw std::runtime_error("dtof_emitter_eval: the rectangle-only kernels run on point emitters and untextured rectangle lights only");
        if (!spec && !plain) throw std::runtime_error("dtof_emitter_eval: spot, directional and environment emitters and textured radiance run in the SPEC kernels only");
        if (level == 6 && bh->n_emitters != 1) throw std::runtime_error("dtof_emitter_eval: the one-emitter fact holds on scenes with exactly one emitter");
        uint32_t index = 0;
        if (mode == 0) {
            if (bh->n_emitters == 0) throw std::runtime_error("dtof_emitter_eval: the scene has no emitter");
        } else if (mode == 1) {
            if (shape_or_minus1 < 0 || (uint32_t) shape_or_minus1 >= bh->n_shapes) throw std::runtime_error("dtof_emitter_eval: shape index out of range");
            if (!(shapes[shape_or_minus1].flags & SF_EMITTER) || !area) throw std::runtime_error("dtof_emitter_eval: the shape carries no emitter");
            index = (uint32_t) shape_or_minus1;
        } else {
            if (!t.has_env || !spec) throw std::runtime_error("dtof_emitter_eval: the scene has no environment");
            index = t.env_index;
        }
        // the table searches index by their sample, and the sampler produces [0, 1 - 2^-24] only: nothing else reaches the device
        const uint32_t n_in = mode == 0 ? 5 : mode == 1 ? 11 : 3, n_out = mode == 0 ? 14 : mode == 1 ? 5 : 4;
        for (size_t i = 0; i < (size_t) n * n_in; ++i) if (!std::isfinite(in[i])) throw std::runtime_error("dtof_emitter_eval: a query holds a float that is not finite");
        if (mode == 0) for (size_t i = 0; i < n; ++i) for (int k = 3; k < 5; ++k)
            if (!(in[i * 5 + k] >= 0.f && in[i * 5 + k] < 1.f)) throw std::runtime_error("dtof_emitter_eval: a draw lies outside [0, 1)");
        ensure_device(sc);
        const float pmf = bh_emitters(*sc) ? 1.f / (float) bh_emitters(*sc) : 0.f;   // m_emitter_pmf, as make_params sets it
        DevBuf<float> din, dout; din.ensure((size_t) n * n_in); dout.ensure((size_t) n * n_out);
        HIP_CHECK(hipMemcpy(din.p, in, (size_t) n * n_in * 4, hipMemcpyHostToDevice));
        (level == 4 ? launch_emitter_eval_spec1 : level == 5 ? launch_emitter_eval_spec2 : mesh ? launch_emitter_eval_mesh : launch_emitter_eval_plain)
            (sc->d_blob.p, level, mode, index, pmf, din.p, dout.p, n, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, dout.p, (size_t) n * n_out * 4, hipMemcpyDeviceToHost));
    });
}
int dtof_camera_rays(dtof_scene *sc, uint32_t n, const float *samples4, float *out7) {
    return guarded([&] {
        if (!sc || (n && (!samples4 || !out7))) throw std::runtime_error("null argument");
        if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
        ensure_device(sc);
        const RenderParams rp = make_params(sc, 0, sc->pp.sample_count ? sc->pp.sample_count : 1, nullptr, 0);
        DevBuf<float> din, dout; din.ensure((size_t) n * 4); dout.ensure((size_t) n * 7);
        HIP_CHECK(hipMemcpy(din.p, samples4, (size_t) n * 16, hipMemcpyHostToDevice));
        launch_camera_rays(rp, din.p, dout.p, n, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out7, dout.p, (size_t) n * 28, hipMemcpyDeviceToHost));
    });
}

static int ray_query(dtof_scene *sc, uint32_t n, const float *rays8, float *out19, int32_t *ids, bool any, float *uv4 = nullptr) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids || (!any && !out19)))) throw std::runtime_error("null argument");
        ensure_device(sc);
        const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
        DevBuf<float> dr, dout, duv; DevBuf<int32_t> dids;
        dr.ensure((size_t) n * 8); dout.ensure(any ? 1 : (size_t) n * 19); dids.ensure((size_t) n * (any ? 1 : 3));
        if (uv4) duv.ensure((size_t) n * 4);
        HIP_CHECK(hipMemcpy(dr.p, rays8, (size_t) n * 32, hipMemcpyHostToDevice));
        launch_ray_query(sc->d_blob.p, dr.p, dout.p, dids.p, uv4 ? duv.p : nullptr, n, any, bh->tlas_depth, nullptr);
        HIP_CHECK(hipGetLastError());
        if (!any) HIP_CHECK(hipMemcpy(out19, dout.p, (size_t) n * 19 * 4, hipMemcpyDeviceToHost));
        if (uv4 && n) HIP_CHECK(hipMemcpy(uv4, duv.p, (size_t) n * 16, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(ids, dids.p, (size_t) n * (any ? 1 : 3) * 4, hipMemcpyDeviceToHost));
    });
}
int dtof_ray_intersect(dtof_scene *sc, uint32_t n, const float *rays8, float *out19, int32_t *ids3) { return ray_query(sc, n, rays8, out19, ids3, false); }
int dtof_ray_intersect_uv(dtof_scene *sc, uint32_t n, const float *rays8, float *out19, int32_t *ids3, float *uv4) { return ray_query(sc, n, rays8, out19, ids3, false, uv4); }
int dtof_ray_test(dtof_scene *sc, uint32_t n, const float *rays8, int32_t *occluded) { return ray_query(sc, n, rays8, nullptr, occluded, true); }

// trace_flat over arrays (dtof_flat_query.hip): the query a frame of this scene runs at every path vertex, in the form asked for
int dtof_flat_query(dtof_scene *sc, int form, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids || (!any && !out3)))) throw std::runtime_error("null argument");
        if (form < 0 || form >= (int) kFlatQueryForms) throw std::runtime_error("dtof_flat_query: form must be 0 (generic), 1 (one_wall) or 2 (shape)");
        if (n > (1u << 24)) throw std::runtime_error("dtof_flat_query: more than 2^24 rays in one call");
        // the memo object and the object count of a frame plan (automatic pipeline, default switches: dtof_scene_export kind 26)
        const SceneTraits t = scene_traits(*sc);
        const FlatChoice c = flat_choice(t, t.blas_triangles <= 32768 && sc->host.textures.empty(), true, true);
        if (c.flat_objects == 0) throw std::runtime_error("dtof_flat_query: the scene has no flat table (rectangles only, at most 8 objects, fused pipeline)");
        if (form >= 1 && !(c.facts & kFactOneWall)) throw std::runtime_error("dtof_flat_query: the one_wall and shape forms need exactly one instance that holds one rectangle");
        if (form == 2 && (flat_query_facts(2) == 0 || (c.facts & kFlatShapeFields) != (flat_query_facts(2) & kFlatShapeFields)))
            throw std::runtime_error("dtof_flat_query: the shape form is compiled for a table of " + std::to_string(flat_shape_count(flat_query_facts(2))) + " rectangles with the wall at index " +
                                     std::to_string(flat_shape_wall(flat_query_facts(2))) + ", this table has " + std::to_string(c.flat_objects) + " and " + std::to_string(c.memo_obj));
        ensure_device(sc);
        DevBuf<float> dr, dout; DevBuf<int32_t> dids;
        dr.ensure((size_t) n * 8); dout.ensure(any ? 1 : (size_t) n * 3); dids.ensure(n);
        if (n) HIP_CHECK(hipMemcpy(dr.p, rays8, (size_t) n * 32, hipMemcpyHostToDevice));
        launch_flat_query(sc->d_blob.p, (uint32_t) sc->blob.size(), t.flat_off, c.flat_objects, c.memo_obj, form, any != 0, dr.p, dout.p, dids.p, n, nullptr);
        HIP_CHECK(hipGetLastError());
        if (n && !any) HIP_CHECK(hipMemcpy(out3, dout.p, (size_t) n * 12, hipMemcpyDeviceToHost));
        if (n) HIP_CHECK(hipMemcpy(ids, dids.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    });
}

// ... and the pair form of the shaped walk (trace_flat: PAIR_RAYS), which k_shade runs where the two lanes of a correlated pair hold the same ray: rays 2k and 2k + 1
// must be equal in o, d and maxt, bit for bit (their times are their own); anything else is refused here, on the host, before a lane relies on it
int dtof_flat_query_pairs(dtof_scene *sc, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids || (!any && !out3)))) throw std::runtime_error("null argument");
        if (n & 1u) throw std::runtime_error("dtof_flat_query_pairs: an odd number of rays");
        if (n > (1u << 24)) throw std::runtime_error("dtof_flat_query_pairs: more than 2^24 rays in one call");
        for (uint32_t i = 0; i < n; i += 2) {
            const float *a = rays8 + (size_t) i * 8, *b = a + 8;
            if (memcmp(a, b, 24) != 0 || memcmp(a + 7, b + 7, 4) != 0)
                throw std::runtime_error("dtof_flat_query_pairs: rays " + std::to_string(i) + " and " + std::to_string(i + 1) + " differ in o, d or maxt");
        }
        const SceneTraits t = scene_traits(*sc);
        const FlatChoice c = flat_choice(t, t.blas_triangles <= 32768 && sc->host.textures.empty(), true, true);
        if (!kFlatQueryPairsBuilt || c.flat_objects == 0 || !(c.facts & kFactOneWall) || (c.facts & kFlatShapeFields) != (flat_query_facts(2) & kFlatShapeFields))
            throw std::runtime_error("dtof_flat_query_pairs: the pair form is compiled for a flat table of 5 rectangles whose one instance, of one rectangle, is at index 2" +
                                     (c.flat_objects ? ", this table has " + std::to_string(c.flat_objects) + " objects" : std::string(", this scene has no flat table")));
        ensure_device(sc);
        DevBuf<float> dr, dout; DevBuf<int32_t> dids;
        dr.ensure((size_t) n * 8); dout.ensure(any ? 1 : (size_t) n * 3); dids.ensure(n);
        if (n) HIP_CHECK(hipMemcpy(dr.p, rays8, (size_t) n * 32, hipMemcpyHostToDevice));
        launch_flat_query(sc->d_blob.p, (uint32_t) sc->blob.size(), t.flat_off, c.flat_objects, c.memo_obj, kFlatQueryPairs, any != 0, dr.p, dout.p, dids.p, n, nullptr);
        HIP_CHECK(hipGetLastError());
        if (n && !any) HIP_CHECK(hipMemcpy(out3, dout.p, (size_t) n * 12, hipMemcpyDeviceToHost));
        if (n) HIP_CHECK(hipMemcpy(ids, dids.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    });
}

// Lane generation over arrays (dtof_pair_setup.hip): what C2's kernel computes at the head of every chunk, per lane (form 0) or with the pair's piece evaluated once
// for the pairs of two chunks (form 1).  The kernels are compiled with the facts of kHeadlinePairFacts that lane generation reads (kPairSetupLaneFacts); a scene, a
// sample count or a range that does not meet them is refused here, before anything is launched or written.
int dtof_pair_setup_lanes(dtof_scene *sc, int form, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, uint32_t *out16) {
    return guarded([&] {
        if (!sc || (n && !out16)) throw std::runtime_error("null argument");
        if (form != 0 && form != 1) throw std::runtime_error("dtof_pair_setup_lanes: form must be 0 (per lane) or 1 (chunk pairs)");
        if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor");
        if ((lane_begin & 63u) != 0 || (n & 63u) != 0) throw std::runtime_error("dtof_pair_setup_lanes: lane_begin and n must be multiples of 64 (whole chunks)");
        if (n > (1u << 24)) throw std::runtime_error("dtof_pair_setup_lanes: more than 2^24 lanes in one call");
        FramePlan p; RenderRequest rq; rq.seed = seed; rq.spp = spp;
        plan_lanes(p, sc, rq);
        RenderParams &rp = p.rp;
        const auto need = [](bool ok, const char *what) { if (!ok) throw std::runtime_error(std::string("dtof_pair_setup_lanes: lane generation is compiled for ") + what); };
        need(p.n_passes == 1, "a single pass");
        need(rp.integrator == 0 && rp.sampler_kind == SAMPLER_CORRELATED, "the dopplertofpath integrator with the correlated sampler");
        need(rp.path_correlation_depth > 0, "a path-correlated camera sample (path_correlation_depth > 0)");
        need(rp.time_sampling == TIME_STRATIFIED && rp.stratify != 0 && rp.tcn == 2 && rp.pcn == 2 && rp.shutter_open_time > 0.f && rp.spp > 1,
             "stratified time sampling per interval with pairs (time_correlate_number = path_correlate_number = 2) and an open shutter");
        need(rp.n_stratum >= 2 && (rp.n_stratum & (rp.n_stratum - 1u)) == 0, "a power-of-two stratum count");
        need(rp.spp_log2 != 0xffffffffu && rp.spp_log2 >= 6, "a power-of-two sample count of at least 64 (whole waves of one pixel)");
        need(!rp.orthographic && rp.aperture_radius == 0.f, "the perspective camera");
        const uint64_t total = (uint64_t) sc->host.sensor.crop_w * sc->host.sensor.crop_h * rp.spp;
        if (lane_begin + n > total) throw std::runtime_error("lane range exceeds the wavefront");
        if (n == 0) return;
        ensure_device(sc);
        rp.lane_base = (uint32_t) lane_begin; rp.n_lanes = (uint32_t) n;
        DevBuf<uint32_t> dout; dout.ensure((size_t) n * kPairSetupWords);
        launch_pair_setup_lanes(rp, form, dout.p, nullptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out16, dout.p, (size_t) n * kPairSetupWords * 4, hipMemcpyDeviceToHost));
    });
}

// trace_scene / trace_deferred over arrays (dtof_tree_query.hip): the TLAS / BLAS query in the form a frame's ray kernels run it.  A form the scene does not meet is
// refused before anything is launched or written.
int dtof_tree_query(dtof_scene *sc, int form, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids3) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids3 || (!any && !out3)))) throw std::runtime_error("null argument");
        if (n > (1u << 24)) throw std::runtime_error("dtof_tree_query: more than 2^24 rays in one call");
        const SceneTraits t = scene_traits(*sc);
        const TreeQueryScene q { t.stack_depth, t.n_tlas_nodes, t.has_nodes16, t.has_analytic };
        if (const char *why = tree_query_refusal(form, q)) throw std::runtime_error(std::string("dtof_tree_query: ") + why);
        ensure_device(sc);
        const size_t per = any ? 1 : 3;
        DevBuf<float> dr, dout; DevBuf<int32_t> dids;
        dr.ensure((size_t) n * 8); dout.ensure(any ? 1 : (size_t) n * 3); dids.ensure((size_t) n * per);
        if (n) HIP_CHECK(hipMemcpy(dr.p, rays8, (size_t) n * 32, hipMemcpyHostToDevice));
        launch_tree_query(sc->d_blob.p, q, form, any != 0, dr.p, dout.p, dids.p, n, nullptr);
        HIP_CHECK(hipGetLastError());
        if (n && !any) HIP_CHECK(hipMemcpy(out3, dout.p, (size_t) n * 12, hipMemcpyDeviceToHost));
        if (n) HIP_CHECK(hipMemcpy(ids3, dids.p, (size_t) n * per * 4, hipMemcpyDeviceToHost));
    });
}

#ifdef DTOF_TRAVERSAL_STATS
// development builds (make STATS=1): read and reset the traversal counters of dtof_traverse.h
// (`n` of the kTravStats slots into out8; dtof_debug_traversal_stats: the first 16)
int dtof_debug_traversal_stats_n(unsigned long long *out8, uint32_t n) {
    return guarded([&] {
        HIP_CHECK(hipDeviceSynchronize());
        unsigned long long all[kTravStats];
        if (!read_traversal_stats(all)) throw HipError("hipMemcpyFromSymbol(g_trav_stats) failed");
        for (uint32_t i = 0; i < n && i < kTravStats; ++i) out8[i] = all[i];
    });
}
int dtof_debug_traversal_stats(unsigned long long *out8) { return dtof_debug_traversal_stats_n(out8, 16); }
#endif

}  // extern "C"
