// dtof_abi_scene.hip -- the C ABI (include/dtof.h) of the scene object: load / free / last error, the integrator and sampler plugins, scene info and export,
// the caller's film layout and stream, cancellation and the plan-facts counters.  No entry here launches a kernel.
#include "dtof_host.h"
#include "dtof_world_to_pixel.h"
#include <cmath>
#include <map>

using namespace dtof;

thread_local std::string dtof::g_last_error;

static std::map<std::string, std::string> to_map(const char *const *names, const char *const *values, int n) {
    std::map<std::string, std::string> m;
    for (int i = 0; i < n; ++i) m[names[i]] = values[i];
    return m;
}

static PropBag make_bag(const char *plugin, const char *const *names, const char *types, const char *const *values, int n) {
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

static dtof_scene *finish_scene(HostScene &&hs) {
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

// the scene's integrator or sampler replaced: the new bag passes the constructors' checks against the plugin that stays before anything changes
static int set_plugin(dtof_scene *sc, bool integrator, const char *plugin, const char *const *names, const char *types, const char *const *values, int n) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null scene");
        PropBag b = make_bag(plugin, names, types, values, n);
        PluginParams p = integrator ? make_plugin_params(b, sc->host.sampler) : make_plugin_params(sc->host.integrator, b);
        (integrator ? sc->host.integrator : sc->host.sampler) = b; sc->pp = p;
    });
}
int dtof_scene_set_integrator(dtof_scene *sc, const char *plugin, const char *const *names, const char *types, const char *const *values, int n) { return set_plugin(sc, true, plugin, names, types, values, n); }
int dtof_scene_set_sampler(dtof_scene *sc, const char *plugin, const char *const *names, const char *types, const char *const *values, int n) { return set_plugin(sc, false, plugin, names, types, values, n); }

struct dtof_integrator { PropBag bag; };
struct dtof_sampler_plugin { PropBag bag; };
// a plugin object's bag, after the constructor's checks (names, types, value ranges) beside the default plugin of the other kind
static PropBag plugin_bag(bool integrator, const char *plugin, const char *const *names, const char *types, const char *const *values, int n) {
    PropBag b = make_bag(plugin, names, types, values, n), other; other.plugin = integrator ? "correlated" : "dopplertofpath";
    (void) (integrator ? make_plugin_params(b, other) : make_plugin_params(other, b));
    return b;
}
int dtof_integrator_create(const char *plugin, const char *const *names, const char *types, const char *const *values, int n, dtof_integrator **out) {
    return guarded([&] { if (!out) throw std::runtime_error("null argument"); *out = new dtof_integrator { plugin_bag(true, plugin, names, types, values, n) }; });
}
void dtof_integrator_destroy(dtof_integrator *i) { delete i; }
int dtof_sampler_plugin_create(const char *plugin, const char *const *names, const char *types, const char *const *values, int n, dtof_sampler_plugin **out) {
    return guarded([&] { if (!out) throw std::runtime_error("null argument"); *out = new dtof_sampler_plugin { plugin_bag(false, plugin, names, types, values, n) }; });
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

int dtof_scene_world_to_pixel(const dtof_scene *sc, double *out12) {
    return guarded([&] {
        if (!sc || !out12) throw std::runtime_error("null argument");
        need_sensor(sc);
        double s[12];
        world_to_pixel(sc->host.sensor, s);
        memcpy(out12, s, sizeof s);
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
            const FlatChoice c = default_flat_choice(*sc, scene_traits(*sc));
            v.push_back((c.facts & kFactOneWall) ? 1.f : 0.f); v.push_back((c.facts & kFactFlatShape) ? 1.f : 0.f); v.push_back((float) flat_shape_count(c.facts)); v.push_back((float) flat_shape_wall(c.facts));
        }
        else if (kind == 27) {   // the triangles as the blob orders them: for every mesh shape its object, its index in the object's group, its triangle count and then DTri::face of
            const BlobHeader *bh = (const BlobHeader *) sc->blob.data();   // each in the BLAS's order -- what maps Hit::prim to the face index of the mesh's own order (integers as bit patterns)
            const DObject *ob = (const DObject *) (sc->blob.data() + bh->off_objects);
            const DShape *shp = (const DShape *) (sc->blob.data() + bh->off_shapes);
            const DGroup *grp = (const DGroup *) (sc->blob.data() + bh->off_groups);
            const DTri *tri = (const DTri *) (sc->blob.data() + bh->off_tris);
            const auto word = [&](uint32_t x) { float b; memcpy(&b, &x, 4); v.push_back(b); };
            for (uint32_t i = 0; i < bh->n_objects; ++i) {
                const bool inst = ob[i].kind == OBJ_INSTANCE;
                for (uint32_t k = 0; k < (inst ? grp[ob[i].index].n_shapes : 1u); ++k) {
                    const DShape &d = shp[inst ? grp[ob[i].index].first_shape + k : ob[i].index];
                    if (d.kind != SHAPE_MESH) continue;
                    word(i); word(k); word(d.n_tris);
                    for (uint32_t f = 0; f < d.n_tris; ++f) word(tri[d.first_tri + f].face);
                }
            }
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
                    const float *lv = (const float *) (sc->blob.data() + e->level_off[k]);
                    size_t count = k == 0 ? (size_t) e->w * e->h : 0;
                    if (k > 0) { uint32_t lx = e->w - 1, ly = e->h - 1; for (uint32_t j = 1; j <= k; ++j) { lx += lx & 1u; ly += ly & 1u; if (j < k) { lx >>= 1; ly >>= 1; } } count = (size_t) lx * ly; }
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

int dtof_scene_set_film_layout(dtof_scene *sc, int32_t planes, uint64_t plane_stride_floats) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null scene");
        if (planes < 0) throw std::runtime_error("negative plane count");
        check_plane_stride(plane_stride_floats, (uint64_t) sc->host.sensor.crop_w * 4, "floats", "one film row");
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
void dtof_cancel(dtof_scene *sc) { if (sc) sc->stop = true; }
uint64_t dtof_scene_plan_facts_launches(const dtof_scene *sc) { return sc ? sc->plan_facts_launches : 0; }
uint32_t dtof_scene_last_plan_facts(const dtof_scene *sc) { return sc ? sc->last_plan_facts : 0; }
uint32_t dtof_scene_last_splat(const dtof_scene *sc) { return sc ? sc->last_splat : 0; }

}  // extern "C"
