// dtof_render.hip -- host orchestration of the wavefront renderer: the frame path.  The C ABI (include/dtof.h) that calls it is in dtof_abi_*.hip, what they share in dtof_host.h.
//
// Replaces, for the `dopplertofpath` + `correlated` path only, SamplingIntegrator::render
// (src/render/integrator.cpp:104-347, JIT branch :226-340): wavefront set-up, sampler seeding,
// lane->pixel mapping, the bounce loop and the film develop.  One host thread drives one HIP
// stream; the wavefront of W*H*spp lanes is cut into row-band batches (results are invariant to
// the cut because every lane's RNG streams are pure functions of its global lane index,
// sampler.cpp:115-134 / correlated.cpp:38-64).
#include "dtof_host.h"
#include "dtof_film64.h"
#include "dtof_moments.h"
#include "dtof_splat_choice.h"
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>

namespace dtof {

const uint32_t kMaxIter = [] { const char *e = getenv("DTOF_STAT_SLOTS"); int v = e ? atoi(e) : 0; return (uint32_t) (v >= 2 ? v : 256); }();

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
static void m4_mul(const float *a, const float *b, float *out) {
    float r[16];
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
        float s = a[4 * i] * b[j];
        for (int k = 1; k < 4; ++k) s = fmaf(a[4 * i + k], b[4 * k + j], s);
        r[4 * i + j] = s;
    }
    memcpy(out, r, sizeof r);
}
static void m4_identity(float *m) { memset(m, 0, 64); m[0] = m[5] = m[10] = m[15] = 1.f; }

// sample_to_camera: inverse of perspective_projection (include/mitsuba/render/sensor.h:226-262) as
// PerspectiveCamera::update_camera_transforms builds it (src/sensors/perspective.cpp:172-198); the
// Transform class carries analytic inverses, so this is the reversed product of the factor inverses.
static void sample_to_camera(const HostSensor &s, float *inv_out) {
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
// At most one of the two is given (n > 0); neither: the integrator's own pair.  w_g_mhz (with variants only): film k's illumination frequency, null = the integrator's own.
RenderParams make_params(const dtof_scene *sc, uint32_t seed, uint32_t spp, const float *offsets, int n_offsets, uint32_t sample_count,
                         const dtof_modulation *variants, int n_variants, const float *w_g_mhz) {
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
    const auto w_g_of = [](float mhz) { return (float) (2 * M_PI * (double) mhz * 1e6); };
    const auto phi_coef_of = [](float mhz) { return (float) ((2 * M_PI * (double) mhz) / 300); };
    for (int k = 0; k < kMaxOffsets; ++k) { rp.w_g[k] = w_g_of(pp.w_g_mhz); rp.phi_coef[k] = phi_coef_of(pp.w_g_mhz); }
    const auto w_d_of = [&](float hetero_frequency) { return (float) (2 * M_PI / (double) pp.time * (double) hetero_frequency); };
    const auto phase_of = [](float hetero_offset) { return (float) ((double) (hetero_offset * 2) * M_PI); };   // dopplertofpath.cpp:30-32
    for (int k = 0; k < kMaxOffsets; ++k) rp.w_d[k] = w_d_of(pp.hetero_frequency);
    rp.amp = (float) (0.5 * (double) pp.g_1);
    rp.g_1 = pp.g_1; rp.g_0 = pp.g_0;
    rp.wave_type = pp.wave_type; rp.low_pass = pp.low_frequency_component_only;
    if (n_variants > 0) {   // film k: the render of an integrator with hetero_frequency = f_k, hetero_offset = o_k (constructor roundings, dopplertofpath.cpp:26-32)
        if (n_variants > kMaxOffsets) throw std::runtime_error("at most 4 modulation variants can be batched per traversal");
        rp.n_offsets = n_variants;
        for (int k = 0; k < n_variants; ++k) { rp.w_d[k] = w_d_of(variants[k].hetero_frequency); rp.phase[k] = phase_of(variants[k].hetero_offset); }
        if (w_g_mhz) for (int k = 0; k < n_variants; ++k) { rp.w_g[k] = w_g_of(w_g_mhz[k]); rp.phi_coef[k] = phi_coef_of(w_g_mhz[k]); }   // ... and w_g = w_g_mhz[k] (:62-69)
    } else if (n_offsets <= 0) { rp.n_offsets = 1; rp.phase[0] = pp.phase_offset; }
    else {
        if (n_offsets > kMaxOffsets) throw std::runtime_error("at most 4 modulation offsets can be batched per traversal");
        rp.n_offsets = n_offsets;
        for (int k = 0; k < n_offsets; ++k) rp.phase[k] = phase_of(offsets[k]);
    }
    rp.path_correlation_depth = pp.path_correlation_depth; rp.max_depth = pp.max_depth; rp.rr_depth = pp.rr_depth;
    rp.integrator = pp.integrator;
    rp.sampler_kind = pp.sampler_kind; rp.jitter = pp.jitter; rp.inv_spp = 1.0f / (float) sample_count;   // dr::rcp(ScalarFloat(m_sample_count))
    need_doppler_for(sc, n_offsets > 0 || n_variants > 0);
    return rp;
}

// Optional roctx ranges around the stage launches (the counterpart of the reference's ScopedPhase / NVTX ranges,
// include/mitsuba/core/profiler.h): DTOF_ROCTX=1 loads the roctx library at run time, `rocprofv3 --marker-trace` then shows
// "dtof:generate|trace|shade|shadow|splat|first" ranges on the host timeline.  No link-time dependency.
namespace {
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
}  // namespace
double stage_ms(const std::vector<std::pair<hipEvent_t, hipEvent_t>> &ev) {
    double ms = 0;
    for (auto &p : ev) { float t = 0; HIP_CHECK(hipEventElapsedTime(&t, p.first, p.second)); ms += t; }
    return ms;
}

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
FlatChoice default_flat_choice(const dtof_scene &sc, const SceneTraits &t) { return flat_choice(t, t.blas_triangles <= 32768 && sc.host.textures.empty(), true, true); }

LaunchSpan FramePlan::launch_span(uint32_t it, bool first, uint32_t n_seg) const {
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
uint32_t FramePlan::launch_facts(const RenderParams &r, const LaunchSpan &l, uint32_t depth0, bool first, bool identity_queue, bool dump) const {
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
    // A pixel list likewise: its global lanes come from the table, which only the run-time branch of global_lane reads.
    if (identity_queue && r.stripe_rows == 0 && r.pixels == nullptr && r.spp_log2 != 0xffffffffu && r.spp_log2 >= 6 && (r.lane_base & 63u) == 0 && (r.n_lanes & 63u) == 0) f |= kFactWavePixel;
    // the two lanes of a pair can split the BSDF samples of the launch between them: they hold one path stream, every draw comes from it, no draw is
    // looked at for roulette or for an emitter pick, and the launch is the whole path in three iterations -- two that sample a BSDF and the terminal one
    constexpr uint32_t pair_needs = kFactWholePath | kFactWavePixel | kFactStratifiedPairs | kFactCorrelated | kFactDopplerCorr | kFactNoRoulette | kFactOneEmitter;
    if (l.span == 3 && (f & pair_needs) == pair_needs) f |= kFactPairSamples;
    return f;
}

// The list form of a request (RenderRequest::pixels): what it cannot be combined with (pixel_list_refusal, dtof_pixel_list.h).  No device call is made here;
// render_rows asks before anything else.
PixelListFacts pixel_list_facts(const dtof_scene *sc, uint32_t spp, uint32_t n_pixels) {
    PixelListFacts f;
    f.spp = spp ? spp : sc->pp.sample_count; f.samples_per_pass = sc->pp.samples_per_pass;
    f.n_pixels = n_pixels; f.crop_pixels = (uint64_t) sc->host.sensor.crop_w * sc->host.sensor.crop_h;
    return f;
}
void refuse_pixel_list(const PixelListFacts &f) {
    const std::string why = pixel_list_refusal(f);
    if (!why.empty()) throw std::runtime_error(why);
}
void check_pixel_list(const dtof_scene *sc, const RenderRequest &rq) {
    if (!rq.pixels) return;
    PixelListFacts f = pixel_list_facts(sc, rq.spp, rq.n_pixels);
    f.stripes = rq.stripes; f.row_range = rq.row_begin != 0 || rq.row_end != 0; f.aov = rq.aov != nullptr;
    f.film32 = rq.film != nullptr; f.film64 = rq.film64 != nullptr; f.moments = rq.moments != nullptr;
    f.lane_dump = rq.lane_dump != nullptr; f.dump_begin = rq.dump_begin; f.dump_n = rq.dump_n;
    refuse_pixel_list(f);
}

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
    p.rp = make_params(sc, rq.seed, spp, rq.offsets, rq.n_offsets, sample_count, rq.variants, rq.n_variants, rq.w_g_mhz);
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
    if (rq.pixels) {   // virtual lanes [0, n_pixels * spp): sample v % spp of listed pixel v / spp; the batches' unit (lanes_per_row) is one pixel
        if (p.n_passes != 1) throw std::runtime_error("a pixel list needs one pass per render");   // (the carried stream states are indexed by virtual lane)
        p.rp.pixels = rq.pixels;
        p.lanes_per_row = spp;
        p.first = rq.lane_dump ? dump_begin : 0;
        p.last = rq.lane_dump ? dump_begin + rq.dump_n : (uint64_t) rq.n_pixels * spp;
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
    // (a pixel list's batches are whole pixels, lane dumps included: lanes_per_row is its spp)
    p.batch = rq.lane_dump && !rq.pixels ? std::min<uint64_t>(batch_lanes, std::max<uint64_t>(rq.dump_n, 1)) : std::max<uint64_t>(1, batch_lanes / p.lanes_per_row) * p.lanes_per_row;
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
    need_sensor(sc);
    check_pixel_list(sc, rq);
    // a guard for internal callers: no entry of the C ABI forms this request (a lane dump never splats, so the films such a request names would stay empty)
    if (rq.aov && (rq.film64 || rq.moments) && rq.lane_dump) throw std::runtime_error("a lane dump cannot be combined with an aov request that names a film");
    ensure_device(sc);
    const FramePlan p = plan_frame(sc, rq);
    sc->last_plan_facts = 0; sc->last_splat = 0;
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
    // An aov request that names the float64 film and / or the moment film as well: the integrator runs in EVERY pass behind k_aov and the splat stage fills those films
    // from the same lanes -- one traversal, three films.  (The float32 film is not part of the combination: the splat stage writes it only when neither is named.)
    const bool aov_films = aov && (rq.film64 != nullptr || rq.moments != nullptr);
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
        const bool integrate = !aov || (p.n_passes > 1 && pass + 1 < p.run_passes) || aov_films;
        if (aov && (!rq.lane_dump || dump_now)) {   // before the shade loop of a multi-pass render overwrites the camera rays
            AovArgs a = *rq.aov;
            if (a.values) a.values += (size_t) (b0 - p.first) * a.n_channels;
            t = tm.begin(kStageTrace, s); launch_aov(blob, blob_bytes, rp, q, a, stack_depth, p.launch, s); tm.end(kStageTrace, t, s);
        }
        // (k_velocity reads the camera rays k_aov read and leaves them alone; an aov request that names a film needs its results for the splat stage)
        if (velocity && (!aov || aov_films)) { t = tm.begin(kStageTrace, s); launch_velocity(blob, blob_bytes, rp, q, stack_depth, p.launch, s); tm.end(kStageTrace, t, s); }
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
        } else if (!rq.lane_dump && !fused_splat_done && (!aov || aov_films)) {
            t = tm.begin(kStageSplat, s);
            // a request may name BOTH the moment film and the float64 film: one traversal, two films (the alpha plane of an rgba scene then goes to the float64 film only)
            if (rq.moments) launch_splat_moments(rp, q, rq.moments, s);
            if (rq.film64) launch_splat_f64(rp, q, rq.film64, rq.film64_stride, s);
            if (!rq.moments && !rq.film64) sc->last_splat = launch_splat(rp, q, rq.film, rq.film_stride, p.launch, s);
            if (sc->host.sensor.alpha && (rq.film64 || !rq.moments)) {   // the alpha film (plane K behind the K offset films): the same splat over (valid, 0, 0) -- ImageBlock::put of aovs[3] (integrator.cpp:528-533)
                RenderParams ra = rp; ra.n_offsets = 1;
                Queues qa = q; qa.res = q.valid_out;
                if (rq.film64) launch_splat_f64(ra, qa, rq.film64 + (size_t) rp.n_offsets * rq.film64_stride, rq.film64_stride, s);
                else launch_splat(ra, qa, rq.film + (size_t) rp.n_offsets * rq.film_stride, rq.film_stride, p.launch, s);
            }
            tm.end(kStageSplat, t, s);
        } else if (fused_splat_done) sc->last_splat = kSplatFusedWord;
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

}  // namespace dtof
