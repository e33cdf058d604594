// dtof_abi_probes.hip -- the C ABI (include/dtof.h) of the test sweeps: the sampler object, the building blocks of the render kernels "over arrays" (modulation, the
// float32 components, BSDF and emitter chains, camera rays, the ray queries in every form a frame runs them, lane generation), and the traversal counters of the
// DTOF_TRAVERSAL_STATS build.  No frame is rendered here; what these entries need from the frame path they take from dtof_host.h.
#include "dtof_host.h"
#include "dtof_flat_query.h"
#include "dtof_pair_setup.h"
#include "dtof_tree_query.h"
#include "dtof_fused_query.h"
#include "dtof_surface_query.h"
#include <cmath>
#include <memory>

using namespace dtof;

extern "C" {

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
        const size_t bytes = (size_t) n * 4;
        round_trip({ { t, bytes }, { len, len ? bytes : 0, bytes } }, { { out, bytes } }, [&](void *const *in, void *const *o) {
            launch_waveform_eval(rp, (const float *) in[0], (const float *) in[1], (float *) o[0], mode, n, nullptr);
        });
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
        const size_t out_bytes = (size_t) n * out_stride * 4;
        round_trip({ { in, (size_t) n * in_stride * 4 } }, { { out, out_bytes } }, [&](void *const *din, void *const *dout) {
            if (out_bytes) HIP_CHECK(hipMemset(dout[0], 0, out_bytes));
            a.in = (const float *) din[0]; a.out = (float *) dout[0];
            launch_component(a, rp, nullptr);
        });
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
        round_trip({ { in29, (size_t) n * 29 * 4 } }, { { out14, (size_t) n * 14 * 4 } }, [&](void *const *in, void *const *out) {
            (spec == 0 ? launch_bsdf_eval_0 : spec == 1 ? launch_bsdf_eval_1 : launch_bsdf_eval_2)(sc->d_blob.p, shape_index, (const float *) in[0], (float *) out[0], n, nullptr);
        });
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
        round_trip({ { in, (size_t) n * n_in * 4 } }, { { out, (size_t) n * n_out * 4 } }, [&](void *const *din, void *const *dout) {
            (level == 4 ? launch_emitter_eval_spec1 : level == 5 ? launch_emitter_eval_spec2 : mesh ? launch_emitter_eval_mesh : launch_emitter_eval_plain)
                (sc->d_blob.p, level, mode, index, pmf, (const float *) din[0], (float *) dout[0], n, nullptr);
        });
    });
}
int dtof_camera_rays(dtof_scene *sc, uint32_t n, const float *samples4, float *out7) {
    return guarded([&] {
        if (!sc || (n && (!samples4 || !out7))) throw std::runtime_error("null argument");
        need_sensor(sc);
        ensure_device(sc);
        const RenderParams rp = make_params(sc, 0, sc->pp.sample_count ? sc->pp.sample_count : 1, nullptr, 0);
        round_trip({ { samples4, (size_t) n * 16 } }, { { out7, (size_t) n * 28 } }, [&](void *const *in, void *const *out) {
            launch_camera_rays(rp, (const float *) in[0], (float *) out[0], n, nullptr);
        });
    });
}

static int ray_query(dtof_scene *sc, uint32_t n, const float *rays8, float *out19, int32_t *ids, bool any, float *uv4 = nullptr) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids || (!any && !out19)))) throw std::runtime_error("null argument");
        ensure_device(sc);
        const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
        // (an occlusion query writes no record: its kernel is handed one float)
        round_trip({ { rays8, (size_t) n * 32 } }, { { out19, any ? 0 : (size_t) n * 19 * 4, 4 }, { ids, (size_t) n * (any ? 1 : 3) * 4 }, { uv4, uv4 ? (size_t) n * 16 : 0 } },
                   [&](void *const *in, void *const *out) {
            launch_ray_query(sc->d_blob.p, (const float *) in[0], (float *) out[0], (int32_t *) out[1], (float *) out[2], n, any, bh->tlas_depth, nullptr);
        });
    });
}
int dtof_ray_intersect(dtof_scene *sc, uint32_t n, const float *rays8, float *out19, int32_t *ids3) { return ray_query(sc, n, rays8, out19, ids3, false); }
int dtof_ray_intersect_uv(dtof_scene *sc, uint32_t n, const float *rays8, float *out19, int32_t *ids3, float *uv4) { return ray_query(sc, n, rays8, out19, ids3, false, uv4); }
int dtof_ray_test(dtof_scene *sc, uint32_t n, const float *rays8, int32_t *occluded) { return ray_query(sc, n, rays8, nullptr, occluded, true); }

// what the two flat queries do once the call is accepted: t and c are the table of a frame plan (automatic pipeline, default switches: dtof_scene_export kind 26)
static void run_flat_query(dtof_scene *sc, const SceneTraits &t, const FlatChoice &c, int form, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids, float *zrow8 = nullptr) {
    ensure_device(sc);
    round_trip({ { rays8, (size_t) n * 32 } }, { { out3, any ? 0 : (size_t) n * 12, 4 }, { ids, (size_t) n * 4 }, { zrow8, zrow8 ? (size_t) n * 32 : 0 } }, [&](void *const *in, void *const *out) {
        launch_flat_query(sc->d_blob.p, (uint32_t) sc->blob.size(), t.flat_off, c.flat_objects, c.memo_obj, form, any != 0, (const float *) in[0], (float *) out[0], (int32_t *) out[1], n, nullptr, zrow8 ? (float *) out[2] : nullptr);
    });
}
// trace_flat over arrays (dtof_flat_query.hip): the query a frame of this scene runs at every path vertex, in the form asked for
int dtof_flat_query(dtof_scene *sc, int form, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids || (!any && !out3)))) throw std::runtime_error("null argument");
        if (form < 0 || form >= (int) kFlatQueryForms) throw std::runtime_error("dtof_flat_query: form must be 0 (generic), 1 (one_wall) or 2 (shape)");
        if (n > (1u << 24)) throw std::runtime_error("dtof_flat_query: more than 2^24 rays in one call");
        // the memo object and the object count of a frame plan (automatic pipeline, default switches: dtof_scene_export kind 26)
        const SceneTraits t = scene_traits(*sc);
        const FlatChoice c = default_flat_choice(*sc, t);
        if (c.flat_objects == 0) throw std::runtime_error("dtof_flat_query: the scene has no flat table (rectangles only, at most 8 objects, fused pipeline)");
        if (form >= 1 && !(c.facts & kFactOneWall)) throw std::runtime_error("dtof_flat_query: the one_wall and shape forms need exactly one instance that holds one rectangle");
        if (form == 2 && (flat_query_facts(2) == 0 || (c.facts & kFlatShapeFields) != (flat_query_facts(2) & kFlatShapeFields)))
            throw std::runtime_error("dtof_flat_query: the shape form is compiled for a table of " + std::to_string(flat_shape_count(flat_query_facts(2))) + " rectangles with the wall at index " +
                                     std::to_string(flat_shape_wall(flat_query_facts(2))) + ", this table has " + std::to_string(c.flat_objects) + " and " + std::to_string(c.memo_obj));
        run_flat_query(sc, t, c, form, any, n, rays8, out3, ids);
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
        const FlatChoice c = default_flat_choice(*sc, t);
        if (!kFlatQueryPairsBuilt || c.flat_objects == 0 || !(c.facts & kFactOneWall) || (c.facts & kFlatShapeFields) != (flat_query_facts(2) & kFlatShapeFields))
            throw std::runtime_error("dtof_flat_query_pairs: the pair form is compiled for a flat table of 5 rectangles whose one instance, of one rectangle, is at index 2" +
                                     (c.flat_objects ? ", this table has " + std::to_string(c.flat_objects) + " objects" : std::string(", this scene has no flat table")));
        run_flat_query(sc, t, c, kFlatQueryPairs, any, n, rays8, out3, ids);
    });
}

// ... and the shaped walk with the plain rectangles' z rows computed on the matrix cores (trace_flat: ZROW, dtof_zrow_mfma.h), as k_shade runs a vertex's shadow and
// continuation queries under that shape; zrow8, if given, receives the eight MFMA values per ray.  The kernel is written for the one shape: any other table is refused here
int dtof_flat_query_zrow(dtof_scene *sc, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids, float *zrow8) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids || (!any && !out3)))) throw std::runtime_error("null argument");
        if (n > (1u << 24)) throw std::runtime_error("dtof_flat_query_zrow: more than 2^24 rays in one call");
        const SceneTraits t = scene_traits(*sc);
        const FlatChoice c = default_flat_choice(*sc, t);
        if (!kFlatQueryZrowBuilt || c.flat_objects == 0 || !(c.facts & kFactOneWall) || (c.facts & kFlatShapeFields) != (flat_query_facts(2) & kFlatShapeFields))
            throw std::runtime_error("dtof_flat_query_zrow: the MFMA z rows are compiled for a flat table of 5 rectangles whose one instance, of one rectangle, is at index 2" +
                                     (c.flat_objects ? ", this table has " + std::to_string(c.flat_objects) + " objects" : std::string(", this scene has no flat table")));
        run_flat_query(sc, t, c, kFlatQueryZrow, any, n, rays8, out3, ids, zrow8);
    });
}

// Lane generation over arrays (dtof_pair_setup.hip): what C2's kernel computes at the head of every chunk, per lane (form 0) or with the pair's piece evaluated once
// for the pairs of two chunks (form 1).  The kernels are compiled with the facts of kHeadlinePairFacts that lane generation reads (kPairSetupLaneFacts); a scene, a
// sample count or a range that does not meet them is refused here, before anything is launched or written.
int dtof_pair_setup_lanes(dtof_scene *sc, int form, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, uint32_t *out16) {
    return guarded([&] {
        if (!sc || (n && !out16)) throw std::runtime_error("null argument");
        if (form != 0 && form != 1) throw std::runtime_error("dtof_pair_setup_lanes: form must be 0 (per lane) or 1 (chunk pairs)");
        need_sensor(sc);
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
        round_trip({}, { { out16, (size_t) n * kPairSetupWords * 4 } }, [&](void *const *, void *const *out) { launch_pair_setup_lanes(rp, form, (uint32_t *) out[0], nullptr); });
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
        round_trip({ { rays8, (size_t) n * 32 } }, { { out3, any ? 0 : (size_t) n * 12, 4 }, { ids3, (size_t) n * (any ? 1 : 3) * 4 } }, [&](void *const *in, void *const *out) {
            launch_tree_query(sc->d_blob.p, q, form, any != 0, (const float *) in[0], (float *) out[0], (int32_t *) out[1], n, nullptr);
        });
    });
}

// trace_scene over arrays as the FUSED shade kernels run it themselves (dtof_fused_query.hip): the classic launch's walk and the resident stage's, with the instance memo
// and the stack columns in k_shade's layout.  The refusals are the plan's own conditions (scene_traits, flat_choice, plan_frame), made before anything is launched or written.
int dtof_fused_query(dtof_scene *sc, int form, int waves, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids3) {
    return guarded([&] {
        if (!sc || (n && (!rays8 || !ids3 || (!any && !out3)))) throw std::runtime_error("dtof_fused_query: null argument");
        if (n > (1u << 24)) throw std::runtime_error("dtof_fused_query: more than 2^24 rays in one call");
        if (sc->blob.size() < sizeof(BlobHeader)) throw std::runtime_error("dtof_fused_query: the scene has no device blob");
        const SceneTraits t = scene_traits(*sc);
        const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
        const DShape *shp = (const DShape *) (sc->blob.data() + bh->off_shapes);
        bool only_rects = true;
        for (uint32_t i = 0; i < bh->n_shapes; ++i) only_rects &= shp[i].kind == SHAPE_RECT;
        // the memo object as flat_choice picks it for a fused frame: exactly one instance
        const FusedQueryScene q { (uint32_t) sc->blob.size(), t.stack_depth, t.n_nodes, t.n_objects, t.small_off, t.small_words, flat_choice(t, true, true, false).memo_obj,
                                  t.has_tris, t.has_blas, t.has_nodes16, t.resident_layout, only_rects };
        const std::string why = fused_query_refusal(form, (uint32_t) waves, q, form >= 2 && form < kFusedQueryForms ? device_lds_limit() : 0u);
        if (!why.empty()) throw std::runtime_error("dtof_fused_query: " + why);
        ensure_device(sc);
        round_trip({ { rays8, (size_t) n * 32 } }, { { out3, any ? 0 : (size_t) n * 12, 4 }, { ids3, (size_t) n * (any ? 1 : 3) * 4 } }, [&](void *const *in, void *const *out) {
            launch_fused_query(sc->d_blob.p, q, form, (uint32_t) waves, any != 0, (const float *) in[0], (float *) out[0], (int32_t *) out[1], n, nullptr);
        });
    });
}

// compute_surface / offset_p over arrays of hits (dtof_surface_query.hip): the surface-interaction fill in the form a frame's kernels run it.  A form the scene does not
// meet and an id out of range are refused before anything is launched or written: the kernel indexes the blob's tables with the ids as they are.
int dtof_surface_eval(dtof_scene *sc, int form, int want_frame, uint32_t n, const float *in10, const int32_t *ids3, float *out32) {
    return guarded([&] {
        if (!sc || (n && (!in10 || !ids3 || !out32))) throw std::runtime_error("null argument");
        if (form < 0 || form >= kSurfaceForms) throw std::runtime_error("dtof_surface_eval: form must be 0 (mesh), 1 (rect), 2 (rect_memo_regs), 3 (rect_memo_lds), 4 (one_wall) or 5 (mesh_memo_regs)");
        if (want_frame != 0 && want_frame != 1) throw std::runtime_error("dtof_surface_eval: want_frame must be 0 or 1");
        if (n > (1u << 24)) throw std::runtime_error("dtof_surface_eval: more than 2^24 hits in one call");
        if (sc->blob.size() < sizeof(BlobHeader)) throw std::runtime_error("dtof_surface_eval: the scene has no device blob");
        const BlobHeader *bh = (const BlobHeader *) sc->blob.data();
        const DObject *ob = (const DObject *) (sc->blob.data() + bh->off_objects);
        const DGroup *grp = (const DGroup *) (sc->blob.data() + bh->off_groups);
        const DShape *shp = (const DShape *) (sc->blob.data() + bh->off_shapes);
        const SceneTraits t = scene_traits(*sc);
        const FlatChoice c = default_flat_choice(*sc, t);
        SurfaceQueryScene q { (uint32_t) sc->blob.size(), t.flat_off, c.flat_objects, t.n_instances == 1 ? t.last_instance : 0xffffffffu };
        const bool rect_form = form >= 1 && form <= 4, memo_form = form >= 2;
        if (rect_form) for (uint32_t i = 0; i < bh->n_shapes; ++i)
            if (shp[i].kind != SHAPE_RECT) throw std::runtime_error("dtof_surface_eval: forms 1 to 4 are the rectangle-only kernels' and the scene has a shape that is not a rectangle");
        if (rect_form && sc->blob.size() > 16u * 1024u) throw std::runtime_error("dtof_surface_eval: the scene does not fit the LDS stage of forms 1 to 4");   // (launch_shade stages up to 16 KiB)
        if (memo_form && form != 4 && q.memo_obj == 0xffffffffu) throw std::runtime_error("dtof_surface_eval: the memo forms need a memo object (exactly one instance)");
        if (form == 4) {
            if (!(c.facts & kFactOneWall)) throw std::runtime_error("dtof_surface_eval: the one_wall form needs a flat table whose one instance holds one rectangle");
            q.memo_obj = c.memo_obj;
        }
        for (uint32_t i = 0; i < n; ++i) {
            const int32_t *id = ids3 + (size_t) i * 3;
            if (id[0] < 0 || (uint32_t) id[0] >= bh->n_objects) throw std::runtime_error("dtof_surface_eval: hit " + std::to_string(i) + ": object out of range");
            const DObject &o = ob[id[0]];
            const bool inst = o.kind == OBJ_INSTANCE;
            if (id[1] < 0 || (uint32_t) id[1] >= (inst ? grp[o.index].n_shapes : 1u)) throw std::runtime_error("dtof_surface_eval: hit " + std::to_string(i) + ": shape beyond its group");
            const DShape &s = shp[inst ? grp[o.index].first_shape + id[1] : o.index];
            if (id[2] < 0 || (s.kind == SHAPE_MESH && (uint32_t) id[2] >= s.n_tris)) throw std::runtime_error("dtof_surface_eval: hit " + std::to_string(i) + ": primitive beyond the mesh's triangles");
        }
        ensure_device(sc);
        round_trip({ { in10, (size_t) n * kSurfaceIn * 4 }, { ids3, (size_t) n * 12 } }, { { out32, (size_t) n * kSurfaceOut * 4 } }, [&](void *const *in, void *const *out) {
            launch_surface_query(sc->d_blob.p, q, form, want_frame != 0, (const float *) in[0], (const int32_t *) in[1], (float *) out[0], n, nullptr);
        });
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
