// dtof_host.h -- what the host library's translation units share: the error plumbing of the C ABI, the scene and sampler objects behind its handles, a render call
// as the entry points fill it in, and the declarations of the frame path (dtof_render.hip) that the C ABI's files (dtof_abi_scene / _films / _probes.hip) call.
// Host code only: no kernel reads this header.
#pragma once
#include "../../include/dtof.h"
#include "dtof_kernels.h"
#include "dtof_aov.h"
#include "dtof_scene.h"
#include "dtof_pixel_list.h"
#include <atomic>
#include <cstring>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

namespace dtof {

extern thread_local std::string g_last_error;   // dtof_last_error: per calling thread (dtof_abi_scene.hip)

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
#define HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    throw dtof::HipError(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

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
// The device round trip of an entry over host arrays: every array gets a device copy of max(bytes, room) bytes, the inputs' `bytes` are uploaded, `launch` is handed the
// device arrays (inputs, then outputs), its status is checked, and the outputs' `bytes` are downloaded.  An array of no bytes is neither allocated nor copied, so an
// entry called with n == 0 returns DTOF_OK and writes nothing.  `room`: bytes the kernel is handed although none are copied (an optional input that was not given).
struct HostArray { const void *host; size_t bytes, room = 0; };
template <typename Launch> void round_trip(std::initializer_list<HostArray> in, std::initializer_list<HostArray> out, Launch &&launch) {
    std::vector<DevBuf<uint8_t>> dev(in.size() + out.size());
    std::vector<void *> p;
    for (const auto &list : { in, out }) for (const HostArray &a : list) {
        DevBuf<uint8_t> &d = dev[p.size()];
        d.ensure(std::max(a.bytes, a.room)); p.push_back(d.p);
        if (p.size() <= in.size() && a.bytes) HIP_CHECK(hipMemcpy(d.p, a.host, a.bytes, hipMemcpyHostToDevice));
    }
    launch(p.data(), p.data() + in.size());
    HIP_CHECK(hipGetLastError());
    size_t i = in.size();
    for (const HostArray &a : out) { if (a.bytes) HIP_CHECK(hipMemcpy(const_cast<void *>(a.host), dev[i].p, a.bytes, hipMemcpyDeviceToHost)); ++i; }
}

// per-iteration count slots of a batch (statistics + the queue counts of the previous iteration); reused cyclically beyond that.
// DTOF_STAT_SLOTS shrinks it so that the tests can exercise the wrap-around with short paths.
extern const uint32_t kMaxIter;
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

}  // namespace dtof

struct dtof_scene {
    dtof::HostScene host;
    dtof::PluginParams pp;
    std::vector<uint8_t> blob;
    dtof::DevBuf<uint8_t> d_blob; bool uploaded = false;
    dtof::Workspace ws;
    dtof::DevBuf<float> d_film, d_rgb;
    dtof::DevBuf<double> d_film64;   // the library's own float64 film (dtof_render_variants_f64, dtof_render_velocity_map_f64)
    dtof::DevBuf<double> d_moments, d_moment_planes;   // the moment film (dtof_render_moments) or the aov film (dtof_render_aovs) of the call: cells of kMomentCell doubles per pixel, and the dense planes copied out
    dtof::DevBuf<uint32_t> d_adaptive; dtof::DevBuf<double> d_adaptive_metric;   // dtof_render_adaptive / _pixels: count, the pass's list, its length and the selection's scratch; the metric map
    dtof::DevBuf<double> d_aov_cells;   // the aov cells of a request that names the moment film as well (dtof_render_denoised, dtof_render_velocity_map_denoised): both cell films at once
    dtof::DevBuf<double> d_denoise;   // dtof_denoise_async: the guide records and the two sets of working planes
    dtof::DevBuf<double> d_denoise_io; dtof::DevBuf<uint32_t> d_denoise_extent;   // the denoised renders: the denoiser's arguments and results; the extent reduction's block records and result
    dtof::DevBuf<float> d_vm_sum, d_vm_tof; dtof::DevBuf<double> d_vm_maps;   // dtof_render_velocity_map: the passes' sum, the ToF images, the per-pair maps and the combined map
    // the caller's device film as declared with dtof_scene_set_film_layout (0 = not declared: colour planes only, W * H * 4 apart)
    int32_t film_planes = 0; uint64_t film_plane_stride = 0;
    dtof::DevBuf<unsigned long long> d_sums;       // [batch][2*kMaxIter] per-iteration totals (survivors, shadow rays)
    dtof::DevBuf<uint2> d_pass_rng;                // multi-pass renders: [lane][3] stream states between the passes
    uint32_t id_shift = 24;                  // Queues::id_shift of this scene
    hipStream_t stream = nullptr;                        // the library's own, or the caller's (dtof_scene_set_stream)
    hipStream_t own_stream = nullptr;                    // what ensure_device created and the destructor destroys
    std::atomic<bool> stop { false };
    uint64_t plan_facts_launches = 0;        // first-bounce launches that took a kernel compiled with plan facts, since the scene was loaded (dtof_scene_plan_facts_launches)
    uint32_t last_plan_facts = 0;            // ... and the FACTS mask of the one the last frame launched, 0 if it launched none (dtof_scene_last_plan_facts)
    uint32_t last_splat = 0;                 // the float32 splat kernel and shape of the last frame's last batch (SplatChoice::packed, kSplatFusedWord; dtof_scene_last_splat)
    // reusable statistics plumbing (creating events / pinned memory per call costs ~0.3 ms)
    std::vector<hipEvent_t> event_pool; size_t events_used = 0;
    // frames enqueued by dtof_render_rows_async and not collected yet: their events (frame, stages) and launch counters; no host synchronisation until dtof_async_collect
    struct DeferredFrame { hipEvent_t ev0, ev1; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[dtof::kStageCount]; dtof_render_stats counters; };
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
    dtof::DevBuf<uint2> rng, rng_time, rng_path; dtof::DevBuf<uint32_t> perm, dim; dtof::DevBuf<float> out; dtof::DevBuf<uint8_t> flags;
};

namespace dtof {

// One call of the renderer, as the entry points fill it in.  The film layout the caller declared (dtof_scene_set_film_layout) stays scene state.
struct RenderRequest {
    uint32_t seed = 0, spp = 0;                   // spp 0: the sampler's sample count
    int32_t row_begin = 0, row_end = 0;           // film rows [row_begin, row_end)
    bool stripes = false; int32_t stripe_rows = 0, stripe_period = 0;   // stripes: only the rows [row_begin + k * stripe_period, ... + stripe_rows) (interleaved shards)
    const float *offsets = nullptr; int n_offsets = 0;                // batched hetero_offset values, or
    const dtof_modulation *variants = nullptr; int n_variants = 0;   // ... batched (hetero_frequency, hetero_offset) pairs (at most one of the two)
    const float *w_g_mhz = nullptr;               // with variants: film k's illumination frequency w_g (MHz), n_variants of them; null = the integrator's own for every film
    int films() const { return n_variants > 0 ? n_variants : n_offsets > 0 ? n_offsets : 1; }   // colour films the call writes
    float4 *lane_planes = nullptr;                // lane dumps: [films()][dump_n] results of every film (q.res), besides film 0's in lane_dump
    float *film = nullptr; uint64_t film_stride = 0;   // K films (and the alpha film behind them) film_stride floats apart
    double *film64 = nullptr; uint64_t film64_stride = 0;   // ... or the float64 film, film64_stride doubles apart: the separate splat stage accumulates in double (dtof_film64.hip)
    double *moments = nullptr;                    // ... or the moment film (dtof_moments.h: cells of kMomentCell doubles), likewise the separate splat stage's; no alpha film
    const AovArgs *aov = nullptr;                 // ... or the geometry channels of the `aov` integrator (dtof_aov.h): k_aov takes the shade loop's place behind k_generate and
                                                  // splats into aov->film itself, or -- with a lane dump -- writes the dumped lanes' channels to aov->values ([dump_n][n_channels]).
                                                  // Named TOGETHER with film64 and / or moments (rows form, no lane dump): one traversal, three films -- k_aov, then the bounce
                                                  // loop in every pass, then the splat stage of film64 + moments; aov->film is then a cell film of its own
    dtof_render_stats *stats = nullptr;
    LaneDebug *lane_dump = nullptr; uint64_t dump_begin = 0, dump_n = 0;   // lane_dump != nullptr: evaluate only lanes [dump_begin, dump_begin + dump_n) and copy their records out
    bool deferred = false;                        // dtof_render_rows_async: timings by events, no counters read back, no synchronisation at the end
    // pixels != nullptr: the LIST form -- only the n_pixels listed pixels are rendered (a DEVICE array of strictly ascending flat indices y * crop_w + x of the crop
    // window; RenderParams::pixels), virtual lanes [0, n_pixels * spp).  An empty list launches nothing.  It takes film64 and / or moments, one pass per render, no
    // stripes, no row range (row_begin = row_end = 0), no aov; a lane dump covers whole pixels of the list (check_pixel_list, dtof_render.hip).
    const uint32_t *pixels = nullptr; uint32_t n_pixels = 0;
};
// The two shapes of a request: the film rows [row_begin, row_end), or the stripes [first_row + k * stripe_period, ... + stripe_rows) below the film's height
inline RenderRequest rows_request(uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end, dtof_render_stats *stats = nullptr, bool deferred = false) {
    RenderRequest rq; rq.seed = seed; rq.spp = spp; rq.row_begin = row_begin; rq.row_end = row_end; rq.stats = stats; rq.deferred = deferred;
    return rq;
}
inline RenderRequest stripes_request(uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period, dtof_render_stats *stats = nullptr, bool deferred = false) {
    RenderRequest rq = rows_request(seed, spp, first_row, 0, stats, deferred);
    rq.stripes = true; rq.stripe_rows = stripe_rows; rq.stripe_period = stripe_period;
    return rq;
}

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
// What one launch of the bounce loop covers when it starts at an iteration
struct LaunchSpan { uint32_t span, chunk_blocks, res_units; bool next_runs, splat_here, terminal, resident; };
// What a frame's plan takes from the scene's flat table (plan_frame; dtof_scene_export kind 26 shows it for the automatic pipeline and the default switches):
struct FlatChoice { uint32_t memo_obj, flat_objects, facts; };

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
    LaunchSpan launch_span(uint32_t it, bool first, uint32_t n_seg) const;   // (dtof_render.hip, like everything declared below)
    uint32_t launch_facts(const RenderParams &r, const LaunchSpan &l, uint32_t depth0, bool first, bool identity_queue, bool dump) const;
};

// ---------------------------------------------------------------- the frame path (dtof_render.hip)
void ensure_device(dtof_scene *sc);
void set_filter(RenderParams &rp, int32_t filter, float radius, float stddev, float B, float C);
RenderParams make_params(const dtof_scene *sc, uint32_t seed, uint32_t spp, const float *offsets, int n_offsets, uint32_t sample_count = 0,
                         const dtof_modulation *variants = nullptr, int n_variants = 0, const float *w_g_mhz = nullptr);
double stage_ms(const std::vector<std::pair<hipEvent_t, hipEvent_t>> &ev);
SceneTraits scene_traits(const dtof_scene &sc);
FlatChoice flat_choice(const SceneTraits &t, bool fused, bool memo_on, bool flat_on);
FlatChoice default_flat_choice(const dtof_scene &sc, const SceneTraits &t);   // ... of the automatic pipeline with the default switches
void check_pixel_list(const dtof_scene *sc, const RenderRequest &rq);   // the refusals of the list form, before any device call (render_rows makes them first of all)
PixelListFacts pixel_list_facts(const dtof_scene *sc, uint32_t spp, uint32_t n_pixels);   // the scene's and the call's part of the facts; the entry adds what it renders into
void refuse_pixel_list(const PixelListFacts &f);   // throws the refusal's message
void plan_lanes(FramePlan &p, const dtof_scene *sc, const RenderRequest &rq);
FramePlan plan_frame(const dtof_scene *sc, const RenderRequest &rq);
void render_rows(dtof_scene *sc, const RenderRequest &rq);

inline uint32_t bh_emitters(const dtof_scene &sc) { return ((const BlobHeader *) sc.blob.data())->n_emitters; }   // the emitter count the kernels see (SceneView::n_emitters)
// The refusals that many entries share, each called at the position where that entry makes it
inline void need_sensor(const dtof_scene *sc) { if (!sc->host.has_sensor) throw std::runtime_error("the scene does not contain a sensor"); }
inline void need_doppler_for(const dtof_scene *sc, bool batched_modulation) {
    if (sc->pp.integrator != INTEGRATOR_DOPPLER && batched_modulation) throw std::runtime_error("modulation offsets only apply to the dopplertofpath integrator");
}
// a plane stride in `unit` (0: dense planes) is a multiple of 4 and at least `least`, which the message names
inline void check_plane_stride(uint64_t stride, uint64_t least, const char *unit, const char *least_name) {
    if (stride != 0 && (stride % 4 != 0 || stride < least)) throw std::runtime_error(std::string("plane stride must be a multiple of 4 ") + unit + " and at least " + least_name);
}

}  // namespace dtof
