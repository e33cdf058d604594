/*
 * dtof.h -- C ABI of libdtof: the MI355X-native `dopplertofpath` integrator and
 * `correlated` sampler (drop-in for that hot path of juhyeonkim95/Mitsuba3DopplerToF).
 *
 * Plain C, opaque handles, caller-owned buffers, integer status codes (0 = ok) with a
 * thread-local message in dtof_last_error().  No C++ or torch types cross this boundary.
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository root).  All compute runs in hand-written HIP kernels on the
 * current HIP device; there is no CPU fallback -- without a GPU every compute entry
 * point returns DTOF_ERR_HIP.
 */
#ifndef DTOF_H
#define DTOF_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTOF_OK            0
#define DTOF_ERR_INVALID   1   /* bad argument / unsupported scene feature / parse error (reference: Throw(...)) */
#define DTOF_ERR_HIP       2   /* HIP runtime failure (no device, out of memory, launch failure) */
#define DTOF_ERR_CANCELLED 3   /* Integrator::cancel() was called */

typedef struct dtof_scene   dtof_scene;     /* Scene + Sensor + Film + the two plugins' parameters */
typedef struct dtof_sampler dtof_sampler;   /* CorrelatedSampler state for n lanes (device resident) */

/* Version / capability string, e.g. "dtof 0.1 (gfx950)". */
const char *dtof_version(void);
/* Message of the last failing call on this thread (reference: the what() of the C++ exception). */
const char *dtof_last_error(void);

/* ---------------------------------------------------------------- scene loading
 * Replaces xml::load_file / xml::load_string (src/core/xml.cpp:1348-1429, called from
 * src/mitsuba/mitsuba.cpp:355-357 and mi.load_file in doppler_tutorials/src/program_runner.py:142).
 * `param_names/values` are the -Dname=value substitutions (src/mitsuba/mitsuba.cpp:241-248). */
int dtof_scene_load_file(const char *path, const char *const *param_names, const char *const *param_values,
                         int n_params, dtof_scene **out);
int dtof_scene_load_string(const char *xml, const char *const *param_names, const char *const *param_values,
                           int n_params, dtof_scene **out);
void dtof_scene_destroy(dtof_scene *scene);

/* Plugin construction: replaces PluginManager::create_object -> new DopplerToFPathIntegrator(props)
 * (src/integrators/dopplertofpath.cpp:19-57 + bases src/render/integrator.cpp:22-28,54-100,568-585) and
 * new CorrelatedSampler(props) (src/samplers/correlated.cpp:17-23, src/render/sampler.cpp:11-20), and
 * mi.load_dict({'type':'dopplertofpath', ...}) of doppler_tutorials/src/program_runner.py:127-141.
 * Properties are given as parallel arrays; `types[i]` is one of 'f' (float), 'i' (integer), 'b' (boolean,
 * value "true"/"false"), 's' (string).  The plugin name goes in `plugin`: integrators "dopplertofpath", "path"
 * (src/integrators/path.cpp), "velocity" (src/integrators/velocity.cpp:125-142); samplers "correlated", "independent"
 * (src/samplers/independent.cpp) and "timestratified" (src/samplers/timestratified.cpp:67-129).
 * Unknown plugin names, wrong types and unreferenced properties fail like the reference's loader. */
int dtof_scene_set_integrator(dtof_scene *scene, const char *plugin, const char *const *names,
                              const char *types, const char *const *values, int n);
int dtof_scene_set_sampler(dtof_scene *scene, const char *plugin, const char *const *names,
                           const char *types, const char *const *values, int n);

/* Scene-independent plugin objects, as the reference constructs them: PluginManager::create_object -> `new T(props)`
 * (src/core/plugin.cpp:174-208; mi.load_dict({...}), program_runner.py:142).  The constructor validates the properties exactly
 * like dtof_scene_set_integrator / _sampler; dtof_integrator_render is Integrator::render(scene, sensor, seed, spp)
 * (include/mitsuba/render/integrator.h:74-79): it installs the integrator (and, if given, the sampler -- NULL keeps the one of
 * the scene file) on `scene` and renders.  Destroy with the matching *_destroy. */
typedef struct dtof_integrator dtof_integrator;
typedef struct dtof_sampler_plugin dtof_sampler_plugin;
int  dtof_integrator_create(const char *plugin, const char *const *names, const char *types, const char *const *values, int n,
                            dtof_integrator **out);
void dtof_integrator_destroy(dtof_integrator *integrator);
int  dtof_sampler_plugin_create(const char *plugin, const char *const *names, const char *types, const char *const *values, int n,
                                dtof_sampler_plugin **out);
void dtof_sampler_plugin_destroy(dtof_sampler_plugin *sampler);

typedef struct {
    int32_t  film_width, film_height, crop_x, crop_y, crop_width, crop_height;
    uint32_t sample_count;          /* Sampler::sample_count() */
    uint32_t n_shapes, n_groups, n_objects, n_emitters, n_triangles, n_bvh_nodes;
    uint32_t scene_blob_bytes;
    /* constructor-rounded plugin parameters (for parity checks of the constructors) */
    float    time, w_g, g_1, g_0, w_s, phase_offset, hetero_frequency, antithetic_shift;
    int32_t  wave_type, low_frequency_component_only, time_sampling, stratify_each_interval;
    uint32_t path_correlation_depth, max_depth, rr_depth, base_seed;
    int32_t  time_correlate_number, path_correlate_number;
    uint32_t bvh_stack_depth;       /* entries a traversal stack can need: TLAS depth + deepest per-mesh BLAS */
    /* reconstruction filter (ReconstructionFilter::radius(), include/mitsuba/render/rfilter.h) and the rows a splat can reach beyond
     * the pixel of its sample: ceil(radius - 0.5) (ImageBlock::put, src/render/imageblock.cpp:423-426; 0 for the box filter, which
     * splats at the lane's own pixel, integrator.cpp:540-541).  A row-band shard must carry `filter_halo` padding rows on each side. */
    float    filter_radius;
    int32_t  filter_halo;
    /* hdrfilm pixel_format = rgba (FilmFlags::Alpha, src/films/hdrfilm.cpp:172-177): develop() returns R, G, B, A.  The host-buffer render calls then write
     * FOUR floats per pixel, and the device-film calls (dtof_render_rows / _stripes) accumulate the alpha film -- (A, 0, 0, W) -- as one more RGBW plane
     * behind the n_offsets colour films of `d_film_rgbw`: they REFUSE an rgba scene until the caller has declared a film of n_offsets + 1 planes
     * (dtof_scene_set_film_layout). */
    int32_t  has_alpha;
} dtof_scene_info;
/* What Film::crop_size / Sampler::sample_count / the plugins' to_string() report (src/films/hdrfilm.cpp:235-279, src/render/sampler.cpp:13-14,
 * src/integrators/dopplertofpath.cpp:315-328), plus the sizes of the packed scene. */
int dtof_scene_get_info(const dtof_scene *scene, dtof_scene_info *info);

/* Flat float32 export of what the loader produced (parity of the XML semantics, row X1):
 * kind 0: object keyframes  -> per object 2+32 floats (t0,t1, key0[16], key1[16]) , rows of `out`
 * kind 1: shape transforms  -> per shape 32 floats (to_world[16], to_object[16])
 * kind 2: sensor            -> to_world[16], x_fov, near, far, shutter_open, shutter_close, sensor kind (0 perspective, 1 thinlens, 2 orthographic), aperture_radius, focus_distance
 * kind 3: emitters          -> per emitter position[3], intensity[3]
 * kind 4..7: baked mesh data -> positions / vertex normals / texcoords / faces (uint32 bit patterns) of all mesh
 *                             shapes (cube, obj, ply) concatenated in shape order (cube.cpp:114-160, obj.cpp, ply.cpp)
 * kind 8: spheres           -> per sphere m_center[3], m_radius, m_inv_surface_area, flip_normals (sphere.cpp:138-160);
 *                             their composed to_world / to_object are in kind 1
 * kind 9: BSDF records      -> per shape 24 floats: kind (0 diffuse, 1 conductor, 2 dielectric, 3 plastic, 4 roughconductor), twosided, eta,
 *                             nonlinear, 1/eta^2, fdr_int, specular sampling weight, reflectance[3], specular_reflectance[3],
 *                             specular_transmittance[3], conductor eta[3], k[3], alpha_u, alpha_v
 *                             (src/bsdfs/{diffuse,conductor,dielectric,plastic,roughconductor,roughplastic}.cpp; 5 = roughplastic, 6 = thindielectric, 7 = roughdielectric,
 *                             whose fdr_int slot carries m_internal_reflectance)
 * kind 11: spot emitters   -> per spot 22 floats: position[3], intensity[3], world-to-local[12], cutoff angle (rad), cos(cutoff), cos(beam width),
 *                             1 / (cutoff - beam width) (src/emitters/spot.cpp:75-100)
 * kind 12: microfacet distribution of the rough BSDFs -> per shape 1 float: 0 beckmann, 1 ggx (MicrofacetType, include/mitsuba/render/microfacet.h:30-36)
 * kind 13: textures        -> per texture (in order of appearance) 17 floats: kind (0 checkerboard, 1 bitmap), filter (0 nearest, 1 bilinear), wrap (0 repeat,
 *                             1 mirror, 2 clamp), channels, width, height, to_uv 2x2, color0[3], color1[3], mean (src/textures/{checkerboard,bitmap}.cpp)
 * kind 18: per emitter 10 floats: kind, position[3], intensity | radiance | irradiance[3], direction of travel[3] (directional emitters)
 * kind 17: per shape 1 float: 1 if its rough BSDF samples all normals (sample_visible = false), else 0
 * kind 16: the environment map (src/emitters/envmap.cpp) as packed: w, h, levels, scale, bounding sphere[4], to_world[12], to_local[12], m_data[h*w*3], then
 *          per level of the Hierarchical2D warp (distr_2d.h:376-482): width, count, values[count]
 * kind 14: texels          -> the linear float32 texels of all bitmap textures, concatenated; kind 15: per shape the index of the texture on its
 *                             reflectance / diffuse_reflectance, -1 = a colour
 * kind 19: per shape 4 floats: indices of the textures on specular_reflectance, specular_transmittance, alpha_u, alpha_v (-1 = a constant)
 * kind 20: per shape 3 floats: inside a `mask` (0 / 1), its opacity (the constant, or the texture's mean), index of the opacity texture (src/bsdfs/mask.cpp)
 * kind 21: per shape 1 float: index of the texture of its `normalmap` / `bumpmap`, -1 = none; kind 22: per shape 2 floats: is a `bumpmap`, its scale
 * kind 23: per shape 5 floats: is a `blendbsdf`, its weight, index of the weight texture, BSDF kind and two-sidedness of bsdf_1 (bsdf_0 is what kind 9 reports)
 * kind 24: per shape 1 float: index of the texture on its area emitter's radiance, -1 = a constant colour
 * kind 25: the shading frames of a small rectangle-only scene's flat table (empty for any other scene) -> per top-level object 13 floats: instance mark (0 plain
 *                             rectangle, 1 instance, 2 instance of one rectangle), the rectangle's n[3] and dp_du[3], and the tangents sh_s[3], sh_t[3] of its shading frame
 *                             (initialize_sh_frame, include/mitsuba/render/interaction.h:258-268) as precomputed for the kernels; zeros for an instance
 * kind 26: what a frame plan takes from the flat table (automatic pipeline, default switches) -> 4 floats: the one instance is the memo object of one rectangle
 *                             (0 / 1), the table's shape is compiled into kernels (0 / 1: at most 8 objects), its object count, the index of the instance
 * kind 27: the triangles in the order the device keeps them -> for every mesh shape (objects ascending, the shapes of a group ascending): its top-level object,
 *                             its index in the object's group, its triangle count, then per triangle IN THE BLAS'S ORDER its face index in the mesh's own order;
 *                             all as uint32 bit patterns.  What maps a face to the `primitive` dtof_surface_eval takes.
 * kind 10: roughplastic tables -> per roughplastic shape the 64 values of m_external_transmittance (roughplastic.cpp:222-257)
 * Returns the number of floats written (<= capacity) through *n_written. */
int dtof_scene_export(const dtof_scene *scene, int kind, float *out, size_t capacity, size_t *n_written);
/* S, world to FILM pixel: the 3 x 4 matrix (rows x, y, w, row-major) with pix(P) = ((S_x . (P, 1)) / (S_w . (P, 1)), (S_y . (P, 1)) / (S_w . (P, 1))) in the
 * coordinates of the sample_pos of dtof_sample_lanes (film pixels, not crop-relative ones).  Rows x, y, w of camera_to_sample o to_world^-1
 * (perspective_projection / orthographic_projection, include/mitsuba/render/sensor.h:226-299) scaled by the film size, computed in double on the host from the
 * loader's float32 sensor.  The depth row is deliberately absent, so near and far clip do not enter.  An orthographic sensor has S_w = (0, 0, 0, 1); a thinlens
 * sensor gives its pinhole (the lens centre).  S_w . (P, 1) <= 0: the point is not in front of the camera.  What it is for: the screen-space motion of a world
 * point between two sensors (harness.camera_flow: the flow of static geometry under a moving camera, the `to_sensor` of the reference's denoiser call).
 * Needs no device.  DTOF_ERR_INVALID: a null argument, a scene without a sensor, a singular to_world. */
int dtof_scene_world_to_pixel(const dtof_scene *scene, double out12[12]);
/* Sensor::sample_ray of the scene's sensor over arrays (src/sensors/perspective.cpp:238-279, thinlens.cpp:257-305, orthographic.cpp:169-196), through the device
 * function the first-bounce kernel generates its primary rays with: per sample the position sample x, y in [0, 1]^2 of the crop window and the aperture sample
 * x, y (4 floats) -> ray origin[3], direction[3], maxt (7 floats).  The ray's time is the sampler's business (render_sample, integrator.cpp:494-496). */
int dtof_camera_rays(dtof_scene *scene, uint32_t n, const float *samples4, float *out7);
/* BSDF::eval_pdf_sample of a shape's BSDF over arrays (src/render/bsdf.cpp:20-29; src/bsdfs/{diffuse,twosided,plastic,conductor,dielectric,thindielectric,rough*,
 * mask,blendbsdf,normalmap,bumpmap,null}.cpp), through the very device function the shade kernels call at every path vertex.  The interaction has the flat local
 * frame (n = sh_n = +z, dp_du = s = +x): per query wi[3], wo[3] (local), sample1, sample2[2], uv[2] (11 floats) -> value * cos(theta_o)[3], pdf(wo), the sampled
 * direction[3], its pdf, eta, 1 if the sampled lobe is a delta lobe, weight[3], 1 if it is a null lobe (14 floats).  `shape_index` counts the scene's shapes in
 * file order (the shapes of a shapegroup included). */
int dtof_bsdf_eval(dtof_scene *scene, uint32_t shape_index, uint32_t n, const float *in11, float *out14);
/* The same over a general interaction and through a chosen instantiation of that device function.  Per query 29 floats: the 11 above, then dp_du[3], dp_dv[3], n[3],
 * sh_s[3], sh_t[3], sh_n[3] (what `normalmap` / `bumpmap` build their frames from; wi and wo stay local to sh_s, sh_t, sh_n) -> the same 14 floats.  `spec` names the
 * instantiation the shade kernels are compiled in: 0 = the diffuse-only kernels, 1 = every BSDF / texture / adapter, 2 = ... and blendbsdf / two-BSDF twosided;
 * -1 = the one a render of this scene runs.  A `spec` the render path could never run on that shape fails with DTOF_ERR_INVALID and writes nothing: 0 on anything but
 * an untextured diffuse (plain or twosided), 1 on a blendbsdf or a two-BSDF twosided.  dtof_bsdf_eval is spec = 2 with the flat frame. */
int dtof_bsdf_eval_ex(dtof_scene *scene, uint32_t shape_index, int spec, uint32_t n, const float *in29, float *out14);
/* The emitter side of a path vertex over arrays, through the very device functions the shade kernels call (next-event estimation and the two densities that feed MIS).
 * mode 0: Scene::sample_emitter_direction without its visibility test (src/render/scene.cpp:171-189,235-291; src/emitters/{point,spot,directional,constant,envmap,
 *         area}.cpp; Shape / Sphere::sample_direction; Mesh::sample_position; Texture::sample_position).  Per query 5 floats: the reference point p[3] and the two
 *         draws e1 (emitter pick, reused) and e2 -> 14 floats: sampled point[3], direction[3], distance, density (times the pick's probability), 1 for a delta
 *         emitter, weight[3] (times the reciprocal of the pick's probability), 1 if the sample is usable (density != 0 and the emitter faces p), the picked emitter.
 * mode 1: the emitter-hit density, DirectionSample(scene, si, prev_si) + Scene::pdf_emitter_direction (area.cpp:161-180, sphere.cpp:298-310) behind a lobe that is
 *         not a delta.  Per query 11 floats: the previous vertex[3], the hit point[3], its shading normal[3], its uv[2], on shape `shape_or_minus1` -> 5 floats:
 *         distance, direction[3], density.
 * mode 2: the environment seen by a ray that left the scene (constant.cpp:150-155, envmap.cpp:299-310,408-425).  Per query the ray's direction[3] -> 4 floats:
 *         density, value[3].
 * `level` names the (AREA, MESH, SPEC) instantiation of the shade kernels whose code runs: 0 (no, no, 0), 1 (yes, no, 0), 2 (no, yes, 0), 3 (yes, yes, 0),
 * 4 (yes, yes, 1), 5 (yes, yes, 2), 6 = level 0 as the kernels compiled for scenes with exactly one emitter take it; -1 = the one a render of this scene runs.
 * The call fails with DTOF_ERR_INVALID and writes nothing
 *   - for a level the render path could never run on this scene: levels 0, 2 and 6 need point emitters only (6: exactly one), level 1 point emitters and untextured
 *     rectangle lights only, levels 0 - 3 and 6 no spot, directional, constant or envmap emitter and no textured radiance;
 *   - for a scene without emitters (mode 0), a shape without an emitter (mode 1), a scene without an environment (mode 2), an index out of range;
 *   - if ANY float of a query is not finite, or a draw lies outside [0, 1).  The table searches of the mesh, texture and environment-map samplers index by their
 *     sample, and the samplers produce [0, 1 - 2^-24] only: no other value reaches the device. */
int dtof_emitter_eval(dtof_scene *scene, int mode, int level, int32_t shape_or_minus1, uint32_t n, const float *in, float *out);

/* ---------------------------------------------------------------- rendering
 * Replaces Integrator::render(Scene*, uint32_t sensor_index, uint32_t seed, uint32_t spp, bool develop,
 * bool evaluate) (include/mitsuba/render/integrator.h:74-79; src/render/integrator.cpp:104-347), i.e.
 * integrator.render(scene, seed=i, spp=n) of program_runner.py:15,23.  spp == 0 uses the sampler's
 * sample_count (integrator.cpp:121-124).  Passes: the integrator's `samples_per_pass` property, or a wavefront of more than
 * 2^32 - 1 lanes, splits the render into spp / spp_per_pass passes exactly as integrator.cpp:121-135,227-245 does -- the sampler is
 * seeded once, its streams run on from pass to pass (Sampler::advance, sampler.cpp:52-55), the film accumulates all passes. */
typedef struct {
    uint64_t n_paths;            /* W*H*spp lanes evaluated by this call */
    uint64_t n_bounces;          /* closest-hit rays traced (path-bounces through the trace+shade loop) */
    uint64_t n_shadow_rays;      /* occlusion rays traced */
    double   ms_total;           /* generate .. develop, HIP events on the library's stream */
    double   ms_generate, ms_trace, ms_shade, ms_shadow, ms_splat;   /* per-stage sums (HIP events) */
    uint32_t n_launches_trace, n_launches_shade, n_launches_shadow;
    uint32_t n_batches;
    /* fused pipeline: the first-bounce launches (lane generation + primary ray + bounce 0 in one kernel) are also counted
     * in ms_shade / n_launches_shade; these two fields single them out */
    uint32_t n_launches_first;
    double   ms_first;
    /* the first-bounce kernel runs up to four iterations of the bounce loop itself, the path state in registers: iterations covered by
     * the first-bounce launches (summed over the batches) and the path-bounces among n_bounces that ran there */
    uint32_t n_inline_iterations;
    uint64_t n_bounces_inline;
    /* first-bounce launches that also splatted their samples (the wave reduces the footprint values of its 64 samples and issues the film atomics itself: 64 spp, one
     * film, radius-1 tent, the whole path inline).  The sums of a pixel's samples are then taken in another ORDER than the splat kernels': films of the two paths
     * differ in the last bits, so checksums compare only between runs with the same value here */
    uint32_t n_fused_splat_launches;
    /* first-bounce launches that ran a kernel compiled with the frame plan's constants (single pass, Doppler integrator + correlated sampler, whole path inline, ...:
     * every fact of the kernel's mask held) instead of the generic one; DTOF_PLAN_FACTS=0 keeps it at 0.  The results are the same bits either way */
    uint32_t n_plan_facts_launches;
} dtof_render_stats;

/* out_rgb: caller-owned host buffer, crop_height*crop_width*3 float32, developed (RGB / W). */
int dtof_render(dtof_scene *scene, uint32_t sensor_index, uint32_t seed, uint32_t spp,
                float *out_rgb, dtof_render_stats *stats);

/* Integrator::render on a scene-independent plugin object (include/mitsuba/render/integrator.h:74-79): the integrator created by
 * dtof_integrator_create renders `scene` with its own parameters and, if given, the sampler plugin object's (else the scene's). */
int dtof_integrator_render(const dtof_integrator *integrator, const dtof_sampler_plugin *sampler_or_null, dtof_scene *scene,
                           uint32_t sensor_index, uint32_t seed, uint32_t spp, float *out_rgb, dtof_render_stats *stats);

/* Tile / shard entry point (no reference counterpart: the reference is single-device).
 * Renders pixel rows [row_begin,row_end) of the crop window and ACCUMULATES the undeveloped R,G,B,W
 * film (hdrfilm.cpp:235-279 channel layout) into `d_film_rgbw`, a DEVICE buffer of
 * crop_height*crop_width*4 float32 the caller zeroed (rows row_begin-r..row_end+r receive splats,
 * r = filter footprint).  n_offsets > 1 evaluates several `hetero_offset` values (in units of 2*pi
 * like the plugin property) in ONE traversal; film k lives at d_film_rgbw + k*crop_h*crop_w*4
 * (dtof_render_rows_variants: several hetero_frequency values as well).
 * offsets == NULL / n_offsets == 0 uses the integrator's own phase offset. */
int dtof_render_rows(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                     const float *offsets, int n_offsets, float *d_film_rgbw, dtof_render_stats *stats);
/* Frames WITHOUT a host synchronisation per frame (a caller that renders frame after frame -- bench.py, an animation -- otherwise leaves the GPU idle while the host
 * reads counters and sets up the next call): dtof_render_rows_async enqueues what dtof_render_rows enqueues on the scene's stream and returns; HIP events around the
 * frame and its stages are kept; the bounce / shadow-ray counters are not read back.  dtof_clear_async / dtof_develop_async put a memset / the film development
 * (HDRFilm::develop, hdrfilm.cpp:305-406) on the same stream.  dtof_async_collect waits for the stream, sums the event times and launch counters of the frames
 * enqueued since the last collect into `sum` (n_bounces / n_shadow_rays stay 0), writes the duration of each frame to frame_ms[0 .. capacity) and their number to
 * *n_frames.  Frames whose pipeline needs counters on the host between bounces (paths that leave the fused first-bounce kernel) still wait there. */
int dtof_render_rows_async(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end, const float *offsets, int n_offsets, float *d_film);
int dtof_clear_async(dtof_scene *scene, void *d_ptr, size_t bytes);
int dtof_develop_async(dtof_scene *scene, const float *d_film, float *d_rgb, int64_t n_pixels);
int dtof_async_collect(dtof_scene *scene, dtof_render_stats *sum, double *frame_ms, uint32_t capacity, uint32_t *n_frames);

/* Interleaved shards (load balance when the cost of a row depends on what it sees): renders the stripes of rows
 * [first_row + k * stripe_period, first_row + k * stripe_period + stripe_rows), k = 0, 1, ..., below crop_height and accumulates
 * like dtof_render_rows.  Rank r of N uses first_row = r * stripe_rows, stripe_period = N * stripe_rows; the union over the
 * ranks is the full frame, lane for lane what a single device renders. */
int dtof_render_stripes(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                        const float *offsets, int n_offsets, float *d_film_rgbw, dtof_render_stats *stats);
/* The stream the library enqueues on.  By default every scene owns one; a caller that has work of its own to order against the renders -- the film exchange of
 * a multi-GPU frame (torch.distributed / RCCL), torch operations on the films -- hands in ITS stream (hipStream_t; torch.cuda.current_stream().cuda_stream) and can
 * then queue clear -> render -> exchange -> develop for many frames without a host wait in between.  NULL goes back to the scene's own stream.  LIFETIME: the library
 * keeps the handle, not the stream -- the caller keeps the stream alive until it has handed it back (another dtof_scene_set_stream call; frames in flight are collected
 * first); handing back a stream that no longer exists is tolerated, every other call on a dead handle fails with DTOF_ERR_HIP.  The reference has
 * no counterpart (Dr.Jit owns the one CUDA stream of a thread, drjit-core/src/init.cpp). */
int dtof_scene_set_stream(dtof_scene *scene, void *hip_stream);
/* dtof_render_stripes without the host synchronisation at its end (see dtof_render_rows_async). */
int dtof_render_stripes_async(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                              const float *offsets, int n_offsets, float *d_film_rgbw);
/* The layout of the caller's device film for the device-film calls (dtof_render_rows / _stripes and their _async forms): `planes` RGBW planes of crop_height * crop_width * 4
 * floats, `plane_stride_floats` apart (0 = dense).  Film k of the batched offsets is plane k; the alpha film of an rgba scene (dtof_scene_info::has_alpha,
 * FilmFlags::Alpha, src/films/hdrfilm.cpp:172-177; ImageBlock::put of aovs[3], integrator.cpp:528-533) is plane n_offsets.  A call that would write more planes than were
 * declared fails with DTOF_ERR_INVALID instead of writing past the buffer; planes = 0 (the default) declares nothing: rgb scenes write their n_offsets planes, rgba scenes
 * are refused.  A band shard that renders into a padded slab (pointer = slab + halo rows) passes the slab's size as the stride.  The planes must not overlap: when a
 * call writes more than one plane and a stride is declared, the stride must hold every film row the call can write -- rows [max(first - h, 0), min(last + 1 + h,
 * crop_height)) for its first and last rendered rows (the band of dtof_render_rows, the first and last stripe row of dtof_render_stripes) and the filter's halo h
 * (dtof_scene_info::filter_halo) -- times crop_width * 4 floats; a smaller stride fails with DTOF_ERR_INVALID before anything is launched.  The layout is state of
 * the scene: it holds for every later call until it is declared again. */
int dtof_scene_set_film_layout(dtof_scene *scene, int32_t planes, uint64_t plane_stride_floats);
/* HDRFilm::develop (src/films/hdrfilm.cpp:305-406) on device buffers: rgb = RGB / (W == 0 ? 1 : W). */
int dtof_develop(const float *d_film_rgbw, float *d_rgb, int64_t n_pixels);
/* ... enqueued on the caller's stream without a host wait (hipStream_t; NULL = the null stream): the develop of a frame whose film exchange runs on a stream of its
 * own, beside the next frame's render (bench.py: the exchange of frame i overlaps the render of frame i + 1). */
int dtof_develop_on_stream(const float *d_film_rgbw, float *d_rgb, int64_t n_pixels, void *hip_stream);
/* ... of an rgba film: rgba = (R, G, B) / W of the colour film and A / W of the alpha film (the plane behind the colour films, see dtof_scene_info::has_alpha). */
int dtof_develop_rgba(const float *d_film_rgbw, const float *d_alpha_film, float *d_rgba, int64_t n_pixels);
/* Same as dtof_render but with n_offsets batched modulation offsets; out_rgb holds n_offsets images. */
int dtof_render_offsets(dtof_scene *scene, uint32_t seed, uint32_t spp, const float *offsets, int n_offsets,
                        float *out_rgb, dtof_render_stats *stats);

/* ---------------------------------------------------------------- modulation variants
 * A modulation variant is a pair (hetero_frequency, hetero_offset), both in the units of the plugin properties of the same names
 * (src/integrators/dopplertofpath.cpp:26-32).  Only eval_modulation_weight (:60-77) reads either of them -- sampler, time draw, camera ray, traversal, BSDF
 * sampling, MIS and roulette do not -- so up to four variants are evaluated in ONE traversal, one film each: film k is, bit for bit per lane, the render of a scene
 * whose integrator carries hetero_frequency = variants[k].hetero_frequency and hetero_offset = variants[k].hetero_offset (the constructor's roundings:
 * w_d = (float) (2 pi / time * f), phase = (float) ((double) (o * 2) * pi)).  Waveform, low_frequency_component_only, w_g, g_0, g_1 and time stay the
 * integrator's.  A homodyne / heterodyne pair of doppler_tutorials/src/utils/image_utils.py:140-199 -- (0, o) and (1, o) -- thus shares its paths.
 * In every entry point below: variants == NULL or n_variants == 0 means the integrator's own pair; n_variants > 4, or any variants with an integrator other than
 * `dopplertofpath`, fails with DTOF_ERR_INVALID before anything is launched.  The dtof_*_offsets / `offsets` forms are variants at the integrator's own frequency. */
typedef struct { float hetero_frequency, hetero_offset; } dtof_modulation;
/* dtof_render_offsets with variants: out_rgb holds n_variants developed images (replaces n_variants calls of Integrator::render, integrator.h:74-79, on n_variants
 * integrators, program_runner.py:82-153). */
int dtof_render_variants(dtof_scene *scene, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants,
                         float *out_rgb, dtof_render_stats *stats);
/* dtof_render_rows / _rows_async / _stripes / _stripes_async with variants (no reference counterpart: the reference is single-device).  The film layout
 * is the one of the offsets forms: plane k of `d_film_rgbw` is variant k, the alpha film of an rgba scene is plane n_variants, and dtof_scene_set_film_layout is
 * checked in the same way (a call that needs more planes than declared is refused and writes nothing). */
int dtof_render_rows_variants(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                              const dtof_modulation *variants, int n_variants, float *d_film_rgbw, dtof_render_stats *stats);
int dtof_render_rows_variants_async(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                                    const dtof_modulation *variants, int n_variants, float *d_film_rgbw);
int dtof_render_stripes_variants(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                                 const dtof_modulation *variants, int n_variants, float *d_film_rgbw, dtof_render_stats *stats);
int dtof_render_stripes_variants_async(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                                       const dtof_modulation *variants, int n_variants, float *d_film_rgbw);

/* ---------------------------------------------------------------- radial-velocity map
 * The tail of a Doppler time-of-flight render -- the passes' mean, the ToF images and the velocity map of the homodyne / heterodyne ratio -- on the device, from films
 * that never leave it.  The results are, bit for bit, what numpy computes on the host from the same films (NaNs are NaNs there and here; payloads are not specified):
 *   sum     acc = img if acc is None else acc + img over the developed passes, float32 (render_multi_pass, doppler_tutorials/src/program_runner.py:11-31)
 *   ToF     mean = sum / (float) n_passes; ((0.2126f r + 0.7152f g) + 0.0722f b) * (float) exposure_time, no fused multiply-add
 *           (to_tof_image on a float32 image, doppler_tutorials/src/utils/image_utils.py:20-31)
 *   map     in double: ratio = |hom| > 0 ? het / hom : 0; conf = |hom| + 1e-5 * 0.0015 (that exposure time is hard-coded there); the ratios' conf-weighted mean,
 *           summed from 0.0 in pair order; clipped to [-1, 0.999] (a NaN stays a NaN, as with np.clip); dw = (ratio * (1 / T)) / (ratio - 1);
 *           v = -(((0.5 dw) 3e8) / (w_g 1e6))   (calc_velocity_from_homo_hetero / _heteros, image_utils.py:140-199)
 * exposure_time (seconds) and w_g_mhz are the DOUBLES the tutorials hand to those functions; they are not read from the integrator, whose `time` is rounded to float32.
 * Every entry below fails with DTOF_ERR_INVALID before anything is enqueued or written: null arguments, n_pairs / n_offsets outside [1, 16], a plane index outside the
 * sum, n_passes = 0, an exposure_time or w_g_mhz that is not finite or not > 0, negative sizes, film or sum pointers that are not 16- / 4-byte aligned. */

/* HDRFilm::develop (src/films/hdrfilm.cpp:305-406) of `planes` RGBW film planes of n_pixels * 4 floats, `plane_stride_floats` apart (0 = dense; else a multiple of 4
 * and >= n_pixels * 4), stored into (first != 0: the first pass assigns, so that a -0.0 survives) or added to (first == 0) the dense running sum
 * d_rgb_sum[planes][n_pixels][3] (render_multi_pass, doppler_tutorials/src/program_runner.py:11-31), the input of dtof_velocity_map_async
 * (doppler_tutorials/src/utils/image_utils.py:20-31,140-199).  Enqueued on the scene's stream without a host wait. */
int dtof_develop_accumulate_async(dtof_scene *scene, const float *d_film_rgbw, int32_t planes, uint64_t plane_stride_floats, float *d_rgb_sum, int64_t n_pixels,
                                  int first);
/* The mean of render_multi_pass (doppler_tutorials/src/program_runner.py:11-31: acc / n_passes), then to_tof_image + calc_velocity_from_homo_heteros
 * (doppler_tutorials/src/utils/image_utils.py:20-31,140-199) over the sum of n_passes passes.  d_rgb_sum holds 2 * n_pairs planes
 * [2 * n_pairs][n_pixels][3]; pair k is (homodyne_planes[k], heterodyne_planes[k]), indices into those planes (host arrays, read before the call returns).
 * d_velocity[n_pixels] double: the combined map; d_velocity_pairs_or_null[n_pairs][n_pixels] double: the map of every pair alone (calc_velocity_from_homo_hetero,
 * image_utils.py:140-168); d_tof_or_null[2 * n_pairs][n_pixels] float32: the ToF image of every plane.  Enqueued on the scene's stream without a host wait. */
int dtof_velocity_map_async(dtof_scene *scene, const float *d_rgb_sum, int n_pairs, const int32_t *homodyne_planes, const int32_t *heterodyne_planes,
                            uint32_t n_passes, double exposure_time, double w_g_mhz, int64_t n_pixels, float *d_tof_or_null, double *d_velocity_pairs_or_null,
                            double *d_velocity);
/* The films one traversal renders for a velocity map: offsets are grouped two per traversal, group (o0, o1) as the variants (0, o0), (0, o1), (1, o0), (1, o1) -- the
 * homodyne films (hetero_frequency 0), then the heterodyne ones (1) -- so a pair never straddles two traversals; an odd last offset is the group (0, o), (1, o).
 * Writes the 2 * n_offsets variants of all groups in order (no device needed). */
int dtof_velocity_map_variants(const float *offsets, int n_offsets, dtof_modulation *out_variants);
/* The whole loop of the tutorials' velocity-map experiment (render_multi_pass, doppler_tutorials/src/program_runner.py:11-31, per film;
 * doppler_tutorials/src/utils/image_utils.py:20-31,140-199) into host buffers:
 * per group of two offsets (dtof_velocity_map_variants) and pass i = 0 .. n_passes - 1, the library's own film is cleared, rendered with seed i and `spp` samples per
 * pixel (0 = the sampler's sample count) like dtof_render_rows_variants_async, and accumulated; then one reconstruction, one copy per requested output and ONE host
 * synchronisation (pipelines that need a host wait inside a frame keep theirs).  out_velocity[H * W] double; out_velocity_pairs_or_null[n_offsets][H * W] double, in
 * the order of `offsets`; out_tof_or_null[2 * n_offsets][H * W] float32, plane k the ToF image of variant k of dtof_velocity_map_variants.  `stats` (may be NULL)
 * sums the traversals like dtof_async_collect: n_paths = W * H * spp * n_passes * ceil(n_offsets / 2), n_bounces and n_shadow_rays stay 0.  The alpha film of an
 * rgba scene is rendered and ignored.  The caller's dtof_scene_set_film_layout state is neither read nor changed.  An integrator other than `dopplertofpath` fails
 * with DTOF_ERR_INVALID. */
int dtof_render_velocity_map(dtof_scene *scene, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                             double *out_velocity, double *out_velocity_pairs_or_null, float *out_tof_or_null, dtof_render_stats *stats);

/* ---------------------------------------------------------------- float64 film (opt-in)
 * A Doppler ToF image is a sum of large terms of both signs, and a float32 film adds them in whatever order the atomics arrive: pixels that cancel to a small fraction
 * of their terms differ from run to run and from the order-independent value of the film.  The entries below render into a film of DOUBLES.  Every splat
 * term is still the float32 product ImageBlock::put forms (src/render/imageblock.cpp:414-531: value * (wx * wy), wx * wy for the weight channel; the box filter adds
 * the value itself and 1) -- it is converted to double and only double additions follow; HDRFilm::develop (src/films/hdrfilm.cpp:305-406) is
 * (float) (sum / (W == 0 ? 1 : W)) with the division in double.  Nothing else differs from the float32 entries: same lanes, same samplers, same kernels up to the splat
 * (the first-bounce kernel never splats into this film: dtof_render_stats::n_fused_splat_launches stays 0).  A film plane is crop_height * crop_width * 4 doubles
 * (R, G, B, W); plane k is variant k, the alpha film of an rgba scene lies behind the colour planes.  Refusals are those of the float32 entries (null arguments, more
 * than four variants, variants under an integrator other than `dopplertofpath`, a film layout too small for the call): DTOF_ERR_INVALID before any device call. */

/* dtof_render_variants with the library's own float64 film (ImageBlock::put, src/render/imageblock.cpp:414-531, and HDRFilm::develop, src/films/hdrfilm.cpp:305-406,
 * with a double accumulator -- the accumulator type is all that differs).  n_variants == 0: the integrator's own pair, one plane.  out_images: n_variants developed
 * images (rgb, or rgba for an rgba film); out_films_or_null: the raw film, n_variants (+ 1 for rgba: the alpha film) planes of crop_height * crop_width * 4 doubles. */
int dtof_render_variants_f64(dtof_scene *scene, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants,
                             float *out_images, double *out_films_or_null, dtof_render_stats *stats);
/* dtof_render_rows_variants into the caller's float64 DEVICE film (ImageBlock::put, src/render/imageblock.cpp:414-531; develop it with dtof_develop_f64_async,
 * src/films/hdrfilm.cpp:305-406 -- the accumulator type is all that differs).  The layout is an argument of the call, not state of the scene: `planes` planes,
 * `plane_stride_doubles` apart (0 = dense; else a multiple of 4 and at least one film row).  Fewer planes than the call writes (n_variants, + 1 for an rgba scene),
 * or -- when it writes more than one -- a stride smaller than the film rows it can reach (its rows and the filter's halo, see dtof_scene_set_film_layout) fails with
 * DTOF_ERR_INVALID before anything is launched.  The film must be 8-byte aligned and zeroed by the caller; the call accumulates and waits for the stream. */
int dtof_render_rows_variants_f64(dtof_scene *scene, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                                  const dtof_modulation *variants, int n_variants, double *d_film64_rgbw, int32_t planes, uint64_t plane_stride_doubles,
                                  dtof_render_stats *stats);
/* dtof_develop_async of a float64 film plane (HDRFilm::develop, src/films/hdrfilm.cpp:305-406, of what ImageBlock::put, src/render/imageblock.cpp:414-531, summed in
 * double -- the accumulator type is all that differs): d_rgb[n_pixels][3] = (float) (RGB / (W == 0 ? 1 : W)), the division in double.  Enqueued on the scene's stream. */
int dtof_develop_f64_async(dtof_scene *scene, const double *d_film64_rgbw, float *d_rgb, int64_t n_pixels);
/* ... of an rgba film (dtof_develop_rgba; src/films/hdrfilm.cpp:305-406 over the sums of src/render/imageblock.cpp:414-531 in double -- the accumulator type is all
 * that differs): (R, G, B) / W of the colour plane and A / W of the alpha plane.  d_rgba is 16-byte aligned. */
int dtof_develop_rgba_f64_async(dtof_scene *scene, const double *d_film64_rgbw, const double *d_alpha_film64, float *d_rgba, int64_t n_pixels);
/* dtof_render_velocity_map over the library's own float64 film: the same groups, passes, seeds and outputs, but every pass is splatted in double
 * (src/render/imageblock.cpp:414-531) and developed in double, rounded to float once (src/films/hdrfilm.cpp:305-406), before it enters the same float32 running sum --
 * the accumulator type is all that differs.  The map is, bit for bit, what numpy computes from the images of dtof_render_variants_f64 with the same seeds. */
int dtof_render_velocity_map_f64(dtof_scene *scene, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                                 double *out_velocity, double *out_velocity_pairs_or_null, float *out_tof_or_null, dtof_render_stats *stats);

/* ---------------------------------------------------------------- modulation frequency per variant (opt-in)
 * The illumination frequency w_g is in the position of hetero_frequency and hetero_offset: it enters eval_modulation_weight (src/integrators/dopplertofpath.cpp:60-77)
 * through two prefactors, w_g itself and phi = 2 pi w_g / 300 * path_length, and nothing else of a path reads it.  The `_freq` entries below take one frequency per
 * variant, w_g_mhz[n_variants] in MHz like the plugin property: film k is, bit for bit per lane, the render of a scene whose integrator carries
 * hetero_frequency = variants[k].hetero_frequency, hetero_offset = variants[k].hetero_offset and w_g = w_g_mhz[k] (the constructor's roundings, :62-69:
 * w_g = (float) (2 pi (double) f 1e6), phi_coef = (float) ((2 pi (double) f) / 300), f a float32).  w_g_mhz_or_null == NULL makes each of them the entry without
 * `_freq`, bit for bit.  Refusals, DTOF_ERR_INVALID before any device call: those of the variants forms; frequencies without variants (variants == NULL or
 * n_variants <= 0); a frequency that is not finite or not > 0.
 * Out of scope: the device-film entries (rows, stripes and their async forms), the moment, pixel-list and adaptive entries and dtof_render_velocity_map keep the
 * integrator's single w_g. */

/* dtof_render_variants with a frequency per film (Integrator::render, include/mitsuba/render/integrator.h:74-79, on n_variants integrators that differ in w_g too). */
int dtof_render_variants_freq(dtof_scene *scene, uint32_t seed, uint32_t spp, const dtof_modulation *variants, const float *w_g_mhz_or_null, int n_variants,
                              float *out_rgb, dtof_render_stats *stats);
/* dtof_render_variants_f64 with a frequency per film (ImageBlock::put, src/render/imageblock.cpp:414-531, and HDRFilm::develop, src/films/hdrfilm.cpp:305-406, with a
 * double accumulator -- the accumulator type is all that differs). */
int dtof_render_variants_freq_f64(dtof_scene *scene, uint32_t seed, uint32_t spp, const dtof_modulation *variants, const float *w_g_mhz_or_null, int n_variants,
                                  float *out_images, double *out_films_or_null, dtof_render_stats *stats);
/* dtof_sample_lanes_variants with a frequency per film (render_sample, src/render/integrator.cpp:476-530, per lane and film). */
int dtof_sample_lanes_variants_freq(dtof_scene *scene, uint32_t seed, uint32_t spp, const dtof_modulation *variants, const float *w_g_mhz_or_null, int n_variants,
                                    uint64_t lane_begin, uint64_t n, float *out_lanes12, uint32_t *out_valid, float *out_rgb);

/* ---------------------------------------------------------------- depth map (opt-in)
 * The range half of a correlation time-of-flight camera: the wrapped phase of the homodyne I / Q films at every modulation frequency, and with two or more frequencies
 * the unwrapped path length, on the device.  With the sinusoidal low-pass weight amp * cos(phase + phi) (dopplertofpath.cpp:60-77, waveform_utils.h:36-62) the film at
 * hetero_offset 0 is A cos(phi) and the one at 0.25 is -A sin(phi), phi = 2 pi w_g / 300 * path_length: hence the minus sign below.  Other waveforms are accepted;
 * the harmonic error they put into the phase is a property of the camera, not of this code.  Per pixel, with F frequencies (every output EQUALS this, word for word;
 * NaN payloads are unspecified):
 *   I_j, Q_j  the float32 ToF values of planes i_planes[j], q_planes[j] of the sum: sum / (float) n_passes, ((0.2126f r + 0.7152f g) + 0.0722f b) * (float) exposure_time
 *             (to_tof_image, doppler_tutorials/src/utils/image_utils.py:20-31, as dtof_velocity_map_async forms it)
 *   ph_j      = atan2(-Q_j, I_j) in float32 (the kernels' atan2, bit for bit the oracle's orc_atan2f); p = (double) ph_j, + 2 pi (6.283185307179586) if p < 0;
 *             frac_j = p / 2 pi;  amp_j = sqrt((double) I_j (double) I_j + (double) Q_j (double) Q_j)
 *   L_j       = 300.0 / w_g_mhz[j] (the constant of dopplertofpath.cpp:64), w_j = frac_j * L_j
 *   F == 1    path = w_0, wraps 0, residual 0
 *   F > 1     for n = 0 .. N - 1, N = (int64) floor(max_path_length / L_0) + 1: c = w_0 + (double) n * L_0; for j >= 1 in order m_j = rint((c - w_j) / L_j)
 *             (ties to even; negative: 0), e_j = w_j + m_j * L_j, r_j = e_j - c; err = sum of r_j * r_j from 0.0 in j order.  The candidate with the smallest err wins,
 *             the first on ties, a NaN never; if none wins every output of the pixel is NaN and its wraps are -1.
 *             S = amp_0 + amp_1 + ...; path = S > 0 ? (amp_0 * c + amp_1 * e_1 + ...) / S : 0, both summed left to right
 *   outputs   depth = 0.5 * path, residual = sqrt(err), wraps[j] (n, m_1, ...), amplitude[j] = amp_j, phase[j] = ph_j
 * A max_path_length of exactly the unambiguous range (300 / gcd of whole-MHz frequencies) admits the first candidate of the NEXT period, which agrees with the other
 * frequencies as well as n = 0 does up to rounding: pass a length just below the range to stay inside the first period.
 * Refusals (DTOF_ERR_INVALID before any device call): null arguments, n_frequencies outside [1, 4], frequencies that are not finite, not > 0 or not distinct, a plane
 * index outside the 2 * n_frequencies planes, n_passes = 0, an exposure_time that is not finite or not > 0, with two or more frequencies a max_path_length for which
 * N is outside [1, 4096], negative sizes, misaligned buffers. */

/* The films a depth map needs: frequency j contributes (0, 0) and (0, 0.25) at w_g_mhz[j]; frequencies are grouped two per traversal -- (0, 0, f0), (0, .25, f0),
 * (0, 0, f1), (0, .25, f1) -- so an I / Q pair never straddles two traversals; an odd last frequency is a group of two films.  Writes the 2 * n_frequencies variants and
 * their frequencies in order: I of frequency j is film 2 j, Q is film 2 j + 1 (dopplertofpath.cpp:26-35,60-77; no device needed). */
int dtof_depth_map_variants(const float *w_g_mhz, int n_frequencies, dtof_modulation *out_variants, float *out_w_g_mhz);
/* The reconstruction above over the sum of n_passes developed passes (render_multi_pass, doppler_tutorials/src/program_runner.py:11-31; to_tof_image,
 * doppler_tutorials/src/utils/image_utils.py:20-31): d_rgb_sum[2 * n_frequencies][n_pixels][3] as dtof_develop_accumulate_async leaves it; i_planes, q_planes and
 * w_g_mhz are host arrays read before the call returns.  d_depth[n_pixels] double; d_residual_or_null[n_pixels] double; d_wraps_or_null[n_frequencies][n_pixels] int32;
 * d_amplitude_or_null[n_frequencies][n_pixels] double; d_phase_or_null[n_frequencies][n_pixels] float32.  Enqueued on the scene's stream without a host wait. */
int dtof_depth_map_async(dtof_scene *scene, const float *d_rgb_sum, int n_frequencies, const int32_t *i_planes, const int32_t *q_planes, const double *w_g_mhz,
                         uint32_t n_passes, double exposure_time, double max_path_length, int64_t n_pixels,
                         double *d_depth, double *d_residual_or_null, int32_t *d_wraps_or_null, double *d_amplitude_or_null, float *d_phase_or_null);
/* The loop of dtof_render_velocity_map (render_multi_pass, doppler_tutorials/src/program_runner.py:11-31, per film) with the groups of dtof_depth_map_variants: per
 * group and pass i = 0 .. n_passes - 1 the library's own film (film64 != 0: its float64 film, as dtof_render_velocity_map_f64) is cleared, rendered with seed i and
 * developed into the running sum; then one reconstruction, one copy per requested output and ONE host synchronisation.  out_depth[H * W] double and the optional
 * outputs as in dtof_depth_map_async; out_tof_or_null[2 * n_frequencies][H * W] float32, plane k the ToF image of film k of dtof_depth_map_variants.  `stats` sums the
 * traversals: n_paths = W * H * spp * n_passes * ceil(n_frequencies / 2).  The caller's dtof_scene_set_film_layout state is neither read nor changed.  An integrator
 * other than `dopplertofpath` fails with DTOF_ERR_INVALID. */
int dtof_render_depth_map(dtof_scene *scene, uint32_t n_passes, uint32_t spp, const float *w_g_mhz, int n_frequencies, double exposure_time, double max_path_length,
                          int film64, double *out_depth, double *out_residual_or_null, int32_t *out_wraps_or_null, double *out_amplitude_or_null,
                          float *out_phase_or_null, float *out_tof_or_null, dtof_render_stats *stats);

/* ---------------------------------------------------------------- moment film (opt-in)
 * What the reference's `moment` integrator records (src/integrators/moment.cpp:85-104): besides the image, the XYZ of every sample (srgb_to_xyz,
 * include/mitsuba/core/spectrum.h:396-402) and its square, as AOVs that ImageBlock::put filters like the image (src/render/imageblock.cpp:414-531) -- here for every
 * variant of one traversal, plus the cross moment Y_j * Y_k of every pair of variants, which the reference has no counterpart of: the variants share their paths, so
 * the covariance of a homodyne / heterodyne pair (and with it a standard error of their ratio, the velocity map) is a by-product of the render.  Per lane and variant,
 * in float32 without fused multiply-adds: X = (0.412453 r + 0.357580 g) + 0.180423 b, Y = (0.212671 r + 0.715160 g) + 0.072169 b,
 * Z = (0.019334 r + 0.119193 g) + 0.950227 b, the squares X X, Y Y, Z Z and the products Y_j Y_k.  Every value is splatted with the footprint and the float32 weights
 * of the float64 film: the term value * (wx * wy) is a float32 product (the box filter adds the value itself and 1), converted to double and added in double.
 * The P(K) = 1 + 6 K + K (K - 1) / 2 planes of K variants, H * W doubles each:
 *   0                       sum w (shared by all planes)
 *   1 + 6 k + 0 .. 2        sum w X_k, w Y_k, w Z_k           k = 0 .. K - 1
 *   1 + 6 k + 3 .. 5        sum w X_k^2, w Y_k^2, w Z_k^2
 *   1 + 6 K + ...           sum w Y_j Y_k for (j, k) = (0,1), (0,2), (0,3), (1,2), (1,3), (2,3) restricted to k < K, in that order
 * The moments are those of the colour channels: the alpha film of an rgba scene is not part of them (such a scene is accepted, its alpha is not accumulated).  The
 * first-bounce kernel never splats into this film: dtof_render_stats::n_fused_splat_launches stays 0. */

/* P(K) of the moment film (the AOV count of src/integrators/moment.cpp:57-65 per integrator, filtered by src/render/imageblock.cpp:414-531, plus the weight and the pair
 * planes): n_variants 0 counts as 1 (the integrator's own pair); n_variants < 0 or > 4: -1.  Needs no device. */
int dtof_moment_planes(int n_variants);
/* The moment film of n_passes traversals (src/integrators/moment.cpp:85-104 through ImageBlock::put, src/render/imageblock.cpp:414-531, with a double accumulator):
 * the library's own film is zeroed ONCE, pass i is rendered with seed + i and `spp` samples per pixel (0 = the sampler's sample count) and all passes accumulate into
 * it -- the raw sums add across passes.  developed != 0: every plane but plane 0 is divided in double by (W == 0 ? 1 : W) on the device (the weighted means
 * E[X], E[X^2], E[Y_j Y_k] that HDRFilm::develop would make of the AOVs, src/films/hdrfilm.cpp:305-406); developed == 0: the raw sums.  out_planes: P(n_variants) planes
 * of crop_height * crop_width doubles.  variants == NULL with n_variants == 0: the integrator's own pair (K = 1).  `stats` (may be NULL) sums the passes.
 * DTOF_ERR_INVALID before any device call: a null scene or output, n_passes == 0, n_variants outside 0 .. 4, n_variants > 0 without variants, variants under an integrator
 * other than `dopplertofpath`.  Without a device: DTOF_ERR_HIP. */
int dtof_render_moments(dtof_scene *scene, uint32_t seed, uint32_t spp, uint32_t n_passes, const dtof_modulation *variants_or_null, int n_variants, int developed,
                        double *out_planes, dtof_render_stats *stats);

/* ---------------------------------------------------------------- geometry channels of the `aov` integrator (opt-in)
 * What the reference's `aov` integrator records (src/integrators/aov.cpp:196-330): the camera ray of every sample is intersected once
 * (scene->ray_intersect(ray, RayFlags::All, ...), :206-207), the interaction is zeroed on a miss (:208) and its fields become channels that ImageBlock::put filters
 * like the image (src/render/imageblock.cpp:414-531).  The types of aov.cpp:118-171 this library writes, their channels and the suffixes of their names:
 *   DTOF_AOV_DEPTH        1  si.t, 0 on a miss (:247-249)                                  name.T
 *   DTOF_AOV_POSITION     3  si.p (:251-255)                                               name.X name.Y name.Z
 *   DTOF_AOV_UV           2  si.uv (:257-260)                                              name.U name.V
 *   DTOF_AOV_GEO_NORMAL   3  si.n (:262-266)                                               name.X name.Y name.Z
 *   DTOF_AOV_SH_NORMAL    3  si.sh_frame.n (:268-272): the shape's shading normal, before any normalmap / bumpmap adapter of its BSDF        name.X name.Y name.Z
 *   DTOF_AOV_DP_DU        3  si.dp_du (:278-282)                                           name.X name.Y name.Z
 *   DTOF_AOV_DP_DV        3  si.dp_dv (:284-288)                                           name.X name.Y name.Z
 *   DTOF_AOV_PRIM_INDEX   1  (float) si.prim_index (:300-302)                              name.I
 *   DTOF_AOV_SHAPE_INDEX  1  see below (:304-306)                                          name.I
 * Every channel is +0 on a miss.  SHAPE INDEX: the reference writes the bits of a registry id or of a pointer (:305), which no other build can reproduce.  Here the
 * value is 1 + the index of the hit shape's record in the scene's shape table, which holds the shapes in the order in which the scene file declares them: a
 * scene-level shape where it stands, the shapes of a shapegroup where the group is declared, an animated shape (which loads as a group of one and its instance,
 * src/core/xml.cpp:1165-1195) where it stands; 0 on a miss.  As in the reference, where si.shape is the shape inside the group and
 * si.instance the instance (src/shapes/instance.cpp:247), every instance of a group reports the shape of the group.
 * Refused with DTOF_ERR_INVALID and a message that names the type: `albedo` (:229-246 needs BSDF::eval_diffuse_reflectance of every BSDF), `boundary_test` (:274-276),
 * `duv_dx` and `duv_dy` (:290-298: this build carries no ray differentials).  Any other type fails with the reference's `Invalid AOV type "x"!` (:173).
 * THE LANES ARE THE SCENE INTEGRATOR'S OWN: lane i of an aov render has the sample position, the time and the camera ray (with its maxt) that dtof_sample_lanes reports
 * for the same seed and spp -- the Doppler branch of render_sample for `dopplertofpath`, the plain branch for `path` and `velocity` (src/render/integrator.cpp:409-543)
 * -- and the ray is intersected at its own time.  (The reference's `aov` is no Doppler integrator and would draw the rays of a nested `dopplertofpath` through the
 * plain branch; with a nested `path` the lanes are the reference's own.)  The RGBA channels of the nested integrator (aov.cpp:308-323) are not part of this film: the
 * image comes from dtof_render.
 * FILM: 1 + C planes of crop_height * crop_width doubles, plane 0 the sum of the filter weights, plane 1 + c channel c in the order of the types; C <= 31.  Terms are
 * formed like the moment film's: value * (wx * wy) is a float32 product (the box filter adds the value itself and 1), converted to double, then only double additions. */
#define DTOF_AOV_DEPTH        0
#define DTOF_AOV_POSITION     1
#define DTOF_AOV_UV           2
#define DTOF_AOV_GEO_NORMAL   3
#define DTOF_AOV_SH_NORMAL    4
#define DTOF_AOV_DP_DU        5
#define DTOF_AOV_DP_DV        6
#define DTOF_AOV_PRIM_INDEX   7
#define DTOF_AOV_SHAPE_INDEX  8
#define DTOF_AOV_MAX_CHANNELS 31

/* The constructor's parse of the `aovs` property (src/integrators/aov.cpp:109-175): tokens split at ',' and ' ' (string::tokenize, include/mitsuba/core/string.h:104-106;
 * empty tokens are dropped), each token split at ':' into <name>:<type>.  types[0 .. *n_types) receives the DTOF_AOV_* constants, names_buf the channel names in film
 * order, each followed by a NUL (aov.cpp:118-171), *n_channels their number.  types / names_buf may be NULL (only the counts are wanted); otherwise a capacity too small
 * for the result is an error.  An empty spec is 0 types (the reference warns, :192-193).  A token that is not <name>:<type> is an error here (the reference warns and
 * then reads item[1] out of range, :115-118).  DTOF_ERR_INVALID with the messages above.  Needs no device. */
int dtof_aov_parse(const char *spec, int32_t *types, int capacity, int *n_types, char *names_buf, size_t names_capacity, int *n_channels);
/* The `aovs` string of a scene whose integrator is <integrator type="aov"> (src/integrators/aov.cpp:109-110), NUL-terminated into buf; the empty string for every other
 * scene.  Returns DTOF_ERR_INVALID if capacity cannot hold it.  Such a scene has exactly one nested <integrator> (aov.cpp:177-190), which is the scene's integrator
 * with all its properties: dtof_render returns its image. */
int dtof_scene_get_aovs(const dtof_scene *scene, char *buf, size_t capacity);
/* The aov film of n_passes traversals of the camera rays (src/integrators/aov.cpp:196-330 through ImageBlock::put, src/render/imageblock.cpp:414-531, with a double
 * accumulator): the library's own film is zeroed ONCE, pass i generates its lanes with seed + i and `spp` samples per pixel (0 = the sampler's sample count) and all
 * passes accumulate into it, as in dtof_render_moments.  developed != 0: every plane but plane 0 is divided in double by (W == 0 ? 1 : W) on the device (what
 * HDRFilm::develop makes of the channels, src/films/hdrfilm.cpp:305-406); developed == 0: the raw sums.  out_planes: 1 + C planes of crop_height * crop_width doubles.
 * `stats` (may be NULL) sums the passes: n_paths counts the lanes, n_fused_splat_launches stays 0, the kernel's time is ms_trace.
 * DTOF_ERR_INVALID before any device call: a null argument, n_passes == 0, n_types < 1, a type outside the DTOF_AOV_* constants, more than 31 channels.  Without a
 * device: DTOF_ERR_HIP. */
int dtof_render_aovs(dtof_scene *scene, uint32_t seed, uint32_t spp, uint32_t n_passes, const int32_t *types, int n_types, int developed, double *out_planes,
                     dtof_render_stats *stats);
/* The per-lane entry beside dtof_sample_lanes, through the same kernel without its splat (src/integrators/aov.cpp:196-330 per sample): out_lanes12 as
 * dtof_sample_lanes writes it (the sample position, time and camera ray are those the aov kernel read; rgb is the scene integrator's), out_values[n][C] the channels
 * of every lane in the order of the types.  Refusals as above. */
int dtof_sample_aov_lanes(dtof_scene *scene, uint32_t seed, uint32_t spp, const int32_t *types, int n_types, uint64_t lane_begin, uint64_t n, float *out_lanes12,
                          float *out_values);

/* ---------------------------------------------------------------- the flow film: motion vectors of the camera rays (opt-in)
 * The producer of the `flow` the denoiser's temporal stage takes, for scenes whose OBJECTS move: the scene carries every object's motion over the shutter as the
 * two keyframes of its <animation>, and this film exposes it as screen-space motion vectors.  It is not one of the reference's aov types (DTOF_AOV_* and
 * dtof_aov_parse are not extended); it runs through the aov film's kernel, compiled with two more values per lane, and through its splat, cells and develop.
 * Per lane the camera ray is the scene integrator's own, with its own time t, exactly as for the aov film.  A miss, or a hit on an object with fewer than two
 * keyframes, gives flow (+0, +0).  Otherwise everything is in double, formed from float32 inputs -- the hit position p, the keyframes key0, key1 (3 x 4 affine,
 * row-major) and times t0, t1 of the hit object -- without fused multiply-add, in exactly this order (tests/flow_ref.py is the numpy restatement the tests hold):
 *   u      x = (t - t0) / (t1 - t0); u = x > 0 ? x : 0; u = u < 1 ? u : 1
 *   M      M[i] = key0[i] * (1 - u) + key1[i] * u for the 12 words; a_rc = M[4 r + c]
 *   M^-1   c00 = a11 a22 - a12 a21, c01 = a12 a20 - a10 a22, c02 = a10 a21 - a11 a20; det = (a00 c00 + a01 c01) + a02 c02; id = 1 / det;
 *          i00 = c00 id, i01 = (a02 a21 - a01 a22) id, i02 = (a01 a12 - a02 a11) id; i10 = c01 id, i11 = (a00 a22 - a02 a20) id, i12 = (a02 a10 - a00 a12) id;
 *          i20 = c02 id, i21 = (a01 a20 - a00 a21) id, i22 = (a00 a11 - a01 a10) id; with t = (M[3], M[7], M[11]): i_r3 = -((i_r0 t_x + i_r1 t_y) + i_r2 t_z)
 *   point  a point (x, y, z) through a row (m0, m1, m2, m3) is ((m0 x + m1 y) + m2 z) + m3
 *   q      = M^-1 p: the hit point in the object's own frame; P0 = key0 q, P1 = key1 q: its positions at shutter open and at shutter close
 *   pix    with S of dtof_scene_world_to_pixel: w = S_w . P, pix(P) = ((S_x . P) / w, (S_y . P) / w)
 *   flow   = pix(P1) - pix(P0), each component rounded to float32 once.  If not (w0 > 0 and w1 > 0): both words are the NaN 0x7fc00000, which the temporal stage
 *          reads as "no history"
 * flow is the pixel motion over ONE shutter interval, pointing from the earlier position to the later one; a caller whose frame interval differs from the exposure
 * scales it.  For static geometry under a moving camera see dtof_scene_world_to_pixel.
 * dtof_render_flow: three planes of crop_height * crop_width doubles -- weight, flow x, flow y -- accumulated, developed and refused exactly as dtof_render_aovs
 * does with a two-channel film (a NaN lane makes its pixels NaN).  dtof_sample_flow_lanes: the per-lane entry, through the same kernel without its splat, as
 * dtof_sample_aov_lanes: out_lanes12 as dtof_sample_lanes writes it, out_flow2[n][2].
 * Out of scope: flow in the sharded renders and on the command line, and fusing this traversal with the images'. */
int dtof_render_flow(dtof_scene *scene, uint32_t seed, uint32_t spp, uint32_t n_passes, int developed, double *out_planes, dtof_render_stats *stats);
int dtof_sample_flow_lanes(dtof_scene *scene, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out_lanes12, float *out_flow2);

/* ---------------------------------------------------------------- denoiser
 * The counterpart of the reference's OptixDenoiser (src/render/python/optixdenoiser_v.cpp; its tests: src/render/tests/test_optixdenoiser.py), written from scratch:
 * an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) whose luminance term is normalised by the per-pixel variance (the spatial pass of SVGF), over
 * n_planes colour planes that share ONE set of weights -- the four films of a velocity map's traversal, so that the heterodyne / homodyne ratio of a pixel stays a
 * ratio of identically weighted neighbourhoods.  All in double, no fused multiply-add; tests/denoise_ref.py is the definition:
 *   level l = 0 .. levels - 1, step s = 2^l, reads the result of level l - 1 (level 0: the inputs converted to double); the guides never change
 *   taps    q = p + s (i, j), i, j in -2 .. 2, j outer, i inner; taps outside the image and invalid taps are skipped
 *   valid   every colour word of every plane, every variance and every present guide word of the pixel is finite; an invalid centre is copied through
 *   weight  w = (b[i] b[j]) exp(-((dn + dx) + dl)), b = (1/16, 1/4, 3/8, 1/4, 1/16); dn = |n_p - n_q|^2 / sigma_normal^2, dx = |x_p - x_q|^2 / sigma_position^2
 *           (squared norms (a a + b b) + c c; 0 without the guide); dl = max_k d_k (0 without a variance) with Y_k = (0.2126 r + 0.7152 g) + 0.0722 b,
 *           den_k = sigma_luminance sqrt(max(var_k(p), 0)) at the CENTRE, d_k = |Y_k(p) - Y_k(q)| / den_k if den_k > 0, else 0 for equal luminances and +inf
 *   result  c'_k(p) = (sum_q w c_k(q)) / (sum_q w), var'_k(p) = (sum_q w^2 var_k(q)) / (sum_q w)^2
 * colour[n_planes][height][width][3] float32; variance_or_null[n_planes][height][width] double, the variance of plane k's luminance estimate;
 * normal_or_null, position_or_null [height][width][3] float32.  out_colour[n_planes][height][width][3] double; out_variance_or_null[n_planes][height][width] double.
 * DTOF_ERR_INVALID before any HIP call, with no output touched: n_planes outside 1 .. 4, levels outside 1 .. 6, width or height < 1 (or > 65535), a sigma of a
 * present guide that is not finite or not > 0 (or whose square is not), a null colour, output or params pointer, out_variance without variance, a misaligned
 * buffer, an output that overlaps an input.  With valid arguments and no device: DTOF_ERR_HIP.  There is no CPU fallback. */
typedef struct {
    int32_t levels;                                          /* 1 .. 6 */
    double sigma_normal, sigma_position, sigma_luminance;    /* read only when the guide is present */
} dtof_denoise_params;
/* DEVICE pointers; 1 + levels launches on the scene's stream, no host wait.  Scratch comes from a per-scene cache. */
int dtof_denoise_async(dtof_scene *scene, const float *d_colour, int n_planes, int32_t width, int32_t height, const double *d_variance_or_null,
                       const float *d_normal_or_null, const float *d_position_or_null, const dtof_denoise_params *params, double *d_out_colour,
                       double *d_out_variance_or_null);
/* The same with HOST pointers and no scene: uploads, runs, downloads and synchronises once. */
int dtof_denoise(const float *colour, int n_planes, int32_t width, int32_t height, const double *variance_or_null, const float *normal_or_null,
                 const float *position_or_null, const dtof_denoise_params *params, double *out_colour, double *out_variance_or_null);

/* ---------------------------------------------------------------- denoiser, temporal stage (opt-in)
 * The other half of the reference's OptixDenoiser(input_size, albedo, normals, temporal) called with `flow` and `previous_denoised`
 * (src/render/python/optixdenoiser_v.cpp), written from scratch after SVGF's temporal accumulation: the previous frame's ACCUMULATED films are reprojected through a
 * screen-space flow field, history that belongs to another surface is rejected per bilinear tap, and mean and variance are blended.  It runs in FRONT of the spatial
 * levels above: the variance it hands them is the variance of the accumulated estimate.  All in double, no fused multiply-add, no epsilon;
 * tests/temporal_ref.py is the definition.  For pixel p = (x, y), n_planes = K colour planes sharing one set of tap weights:
 *   cur_ok   every colour word of every plane, every variance and every present guide word (normal, ids) of p is finite.  If not: the outputs are the converted
 *            inputs and o_length = 0 (later frames take no history from this pixel)
 *   taps     rx = x - (double) flow_x, ry = y - (double) flow_y; x0 = floor(rx), a = rx - x0; y0 = floor(ry), b = ry - y0; q = (x0 + i, y0 + j), i, j in {0, 1},
 *            j outer; wt = (i ? a : 1 - a) * (j ? b : 1 - b).  flow points from the pixel's earlier position to its current one, in pixels
 *   accepted iff ALL hold: a history is present; both flow words are finite; wt > 0; q lies in the image (decided on the doubles); h_length(q) > 0; every history
 *            colour, variance and guide word at q is finite; h_ids(q) == ids(p); |n_p - n_q|^2 <= tau_normal^2 (squared norm (a a + b b) + c c of the double
 *            differences)
 *   sums     over the accepted taps in tap order: sw += wt; sc_k += wt * h_colour_k(q) per channel; sv_k += wt * h_variance_k(q); sn += wt * (double) h_length(q)
 *   sw == 0  the outputs are the converted inputs and o_length = 1
 *   else     hc = sc / sw, hv = sv / sw, hn = sn / sw; n = min(hn + 1, max_length); alpha = max(1 / n, alpha_min);
 *            o_colour = (1 - alpha) * hc + alpha * colour; o_variance = ((1 - alpha) * (1 - alpha)) * hv + (alpha * alpha) * variance (the frames are independent
 *            estimates); o_length = (float) n
 * Scaling colour and h_colour by a power of two c and the variances by c^2 scales the outputs by exactly c and c^2.
 * The caller keeps the current normal / ids as the next frame's h_normal / h_ids; the stage copies none.  Out of scope: a world-space position test of the history
 * (it would need the point's previous position as a plane) and SVGF's 3 x 3 variance prefilter.
 * DTOF_ERR_INVALID before any HIP call, with no output touched: n_planes outside 1 .. 4; width or height < 1 or > 65535; a null buffers, params, colour, flow,
 * o_colour or o_length pointer; a history that is only partly present (with a history: h_colour, h_length and the history of every present variance / normal / ids);
 * a history buffer whose current buffer is absent; o_variance present without variance or absent with it; a misaligned buffer; an output that overlaps an input or
 * another output; alpha_min outside (0, 1], max_length < 1, tau_normal <= 0 with normals (or its square not a finite double > 0), or any of them not finite.
 * With valid arguments and no device: DTOF_ERR_HIP.  There is no CPU fallback. */
typedef struct {
    double alpha_min;      /* (0, 1]: the least weight of the current frame */
    double max_length;     /* >= 1: the history length is clamped to it */
    double tau_normal;     /* > 0; read only when normals are present */
} dtof_temporal_params;
typedef struct {
    /* the current frame */
    const float *colour;            /* [K][H][W][3] */
    const double *variance;         /* [K][H][W] or NULL */
    const float *normal;            /* [H][W][3] or NULL */
    const float *ids;               /* [H][W] or NULL, e.g. the aov film's shape_index plane */
    const float *flow;              /* [H][W][2] */
    /* the history: all NULL for a first frame, otherwise h_colour, h_length and the counterpart of every present buffer above */
    const double *h_colour;         /* [K][H][W][3]: o_colour of the previous call */
    const double *h_variance;       /* [K][H][W]: o_variance of the previous call */
    const float *h_normal, *h_ids;  /* normal, ids of the previous call */
    const float *h_length;          /* [H][W]: o_length of the previous call */
    /* outputs */
    double *o_colour;               /* [K][H][W][3] */
    double *o_variance;             /* [K][H][W]; present iff variance is */
    float *o_length;                /* [H][W] */
    float *o_colour_f32;            /* [K][H][W][3] or NULL: o_colour rounded once, what dtof_denoise_async takes as its colour */
} dtof_temporal_buffers;
/* DEVICE pointers in *d_buffers (the struct itself is host memory); one launch on the scene's stream, no host wait, no scratch. */
int dtof_denoise_temporal_async(dtof_scene *scene, const dtof_temporal_buffers *d_buffers, int n_planes, int32_t width, int32_t height,
                                const dtof_temporal_params *params);
/* The same with HOST pointers and no scene: uploads, runs, downloads and synchronises once. */
int dtof_denoise_temporal(const dtof_temporal_buffers *buffers, int n_planes, int32_t width, int32_t height, const dtof_temporal_params *params);

/* ---------------------------------------------------------------- denoised renders on the device (opt-in)
 * The denoised images and the denoised velocity map from ONE traversal per pass, with nothing but the requested results crossing to the host.  A pass renders the
 * float64 film, the moment film and the aov film of "p:position,n:sh_normal" from the same lanes (k_aov, the bounce loop, the splat stage); the films of the passes
 * (seeds seed, seed + 1, ...) are developed and summed in float32 as dtof_render_velocity_map_f64 sums them, the moment and aov cells accumulate in double.  Then
 *   INPUTS  (tests/denoise_inputs_ref.py is the definition; K planes, pixel i, Wd = (W == 0 ? 1 : W) of the cell film in question)
 *     colour    IMAGE: sum / (float) n_passes per channel.  TOF: ((0.2126f r + 0.7152f g) + 0.0722f b) * (float) exposure_time of that mean, replicated into 3 channels
 *     variance  mean = SY_k / Wd, m2 = SYY_k / Wd of the moment film; v = (m2 - mean * mean) / n_samples, in TOF mode times (exposure_time * exposure_time);
 *               n_samples = (double) n_paths / (double) n_pixels of the traversals.  All in double
 *     guides    position c = (float) (S_c / Wd), normal likewise, of the aov film, the division in double
 *     sigma_position, if automatic: 1 % of the largest per-axis extent (double) max - (double) min of the positions whose three words are finite; 1.0 if that is not > 0
 *   DENOISE  dtof_denoise_async's launches over those arguments (levels, sigma_normal, sigma_luminance of `params`; its sigma_position unless automatic)
 *   MAP      TOF mode: the noisy map is dtof_velocity_map_async's of the sum; the denoised map the same arithmetic from the ratio onwards over channel 0 of the
 *            denoised planes (doubles), i.e. calc_velocity_from_homo_heteros of doppler_tutorials/src/utils/image_utils.py:170-199 of those planes
 * The colour of this route is the FLOAT64 film's image: every pass is dtof_render_variants_f64's image, rounded to float32 once before the float32 pass sum, as in
 * dtof_render_velocity_map_f64.  (Denoising the images of dtof_render_variants on the host reads the float32 film instead.)  An alpha plane is rendered into the float64
 * film of an rgba scene as always, and is neither returned nor denoised.
 * `outputs`: HOST pointers, each NULL or an array of the stated size; only what is named is copied, after one wait at the end.  K = the number of colour planes. */
typedef struct dtof_denoised_outputs {
    double *denoised;            /* required: [K][H][W][3], the denoised colour */
    double *denoised_map;        /* TOF mode: required, [H][W]; IMAGE mode: not read */
    float *sum;                  /* [K][H][W][3]: the float32 sum of the developed passes */
    double *moments;             /* [dtof_moment_planes(K)][H][W]: the raw (undivided) moment planes of dtof_render_moments */
    double *aovs;                /* [7][H][W]: the raw aov planes of dtof_render_aovs for "p:position,n:sh_normal" (weight, position, normal) */
    float *colour;               /* [K][H][W][3]: the denoiser's colour argument */
    double *variance;            /* [K][H][W]: ... its variance argument */
    float *normal, *position;    /* [H][W][3]: ... its guides */
    double *denoised_variance;   /* [K][H][W] */
    double *noisy_map;           /* TOF mode: [H][W]; IMAGE mode: not read */
    double *sigma_position;      /* one double: the sigma_position the denoiser ran with */
} dtof_denoised_outputs;
#define DTOF_DENOISE_INPUTS_IMAGE 0
#define DTOF_DENOISE_INPUTS_TOF   1
/* The INPUTS stage alone over DEVICE pointers: d_rgb_sum [n_planes][n_pixels][3] float32 as dtof_develop_accumulate_async leaves it, d_moment_cells and d_aov_cells
 * n_pixels cells of 32 doubles (cell[p] = raw plane p; the aov cells: weight, position, normal) -> d_colour [n_planes][n_pixels][3] float32, d_variance
 * [n_planes][n_pixels] double, d_normal / d_position [n_pixels][3] float32, and -- if d_extent_or_null is given -- 8 words: the per-axis min (3 float32) and max
 * (3 float32) of the positions whose three words are finite (+inf / -inf without one), their count (uint32) and 0.  One launch, three with the extent, on the
 * scene's stream; no atomics, no host wait.  DTOF_ERR_INVALID before any HIP call: a null pointer (but d_extent_or_null), a mode other than the two, n_planes outside
 * 1 .. 4, n_passes == 0, n_samples not finite or not > 0, in TOF mode an exposure_time not finite or not > 0, n_pixels < 0 or > 2^31 - 1, a misaligned buffer, an output
 * that overlaps an input or another output. */
int dtof_denoise_inputs_async(dtof_scene *scene, int mode, const float *d_rgb_sum, const double *d_moment_cells, const double *d_aov_cells, int n_planes,
                              int64_t n_pixels, uint32_t n_passes, double n_samples, double exposure_time, float *d_colour, double *d_variance, float *d_normal,
                              float *d_position, uint32_t *d_extent_or_null);
/* IMAGE mode: the images of `variants_or_null` / n_variants (NULL / 0: the integrator's own pair, K = 1) and their jointly denoised versions.  sigma_position_auto != 0:
 * params->sigma_position is not read.  stats sums the passes: n_paths = W * H * spp * n_passes, one traversal per pass.
 * DTOF_ERR_INVALID before any device call, with no output touched: a null scene, params, outputs or outputs->denoised; n_passes == 0; more than four variants (or a
 * negative count, or a count without variants); variants under an integrator other than dopplertofpath; levels outside 1 .. 6; a sigma that dtof_denoise refuses
 * (sigma_position only when it is read); a scene without a sensor or with a film wider or higher than 65535 pixels. */
int dtof_render_denoised(dtof_scene *scene, uint32_t seed, uint32_t spp, uint32_t n_passes, const dtof_modulation *variants_or_null, int n_variants,
                         const dtof_denoise_params *params, int sigma_position_auto, const dtof_denoised_outputs *outputs, dtof_render_stats *stats);
/* TOF mode: the four films of dtof_velocity_map_variants for the two `offsets` (planes: (0, o0), (0, o1), (1, o0), (1, o1)), denoised jointly as ToF planes, the noisy
 * velocity map and the map of the denoised planes.  Refused like dtof_render_denoised, and: null offsets or outputs->denoised_map; exposure_time or w_g_mhz not
 * finite or not > 0; an integrator other than dopplertofpath. */
int dtof_render_velocity_map_denoised(dtof_scene *scene, uint32_t seed, uint32_t spp, uint32_t n_passes, const float offsets[2], double exposure_time, double w_g_mhz,
                                      const dtof_denoise_params *params, int sigma_position_auto, const dtof_denoised_outputs *outputs, dtof_render_stats *stats);

/* ---------------------------------------------------------------- adaptive sampling (opt-in)
 * A dense base pass, then further passes only over the pixels whose ESTIMATED error is still above a tolerance; the estimate comes from the moment film of the passes so
 * far.  The reference renders every pixel in every pass (render_multi_pass, doppler_tutorials/src/program_runner.py:11-31); this has no counterpart there.
 * PIXEL LISTS.  A list is n strictly ascending flat indices y * crop_width + x of the crop window.  A render over a list evaluates, for every listed pixel, exactly the
 * lanes pixel * spp + sample of the dense render with the same seed (a lane's streams are functions of the seed and that index alone, src/render/sampler.cpp:115-134,
 * src/samplers/correlated.cpp:38-64), and splats them like the dense render: the films of the FULL list are the dense films.  A list takes the float64 film and the moment
 * film only, and one pass per render: an integrator whose samples_per_pass is below the sample count is refused.
 * SELECTION, all in double without fused multiply-add, in exactly this order.  S = the P(K) raw moment sums of the pixel (see the moment film), count = the samples
 * rendered IN the pixel so far, max(x, y) = (x >= y || x is NaN) ? x : y:
 *   per variant k   Wd = (S[0] == 0 ? 1 : S[0]); mean_k = S[1 + 6 k + 1] / Wd; m2_k = S[1 + 6 k + 4] / Wd; var_k = m2_k - mean_k * mean_k; n = (double) count
 *   image mode      se_k = sqrt(max(var_k, 0) / n); metric = max over k of se_k / max(|mean_k|, floor); selected iff metric > tol; count == 0: metric 0, not selected
 *   velocity mode   per pair (h, t) of a homodyne and a heterodyne variant, the delta method on the ratio the velocity map is made of
 *                   (doppler_tutorials/src/utils/image_utils.py:140-199): a = mean_h, b = mean_t, cov = S[cross(h, t)] / Wd - a * b, r = b / a,
 *                   var_r = ((var_t - (2 r) cov) + (r r) var_h) / ((a a) n), slope = ((0.5 * 3e8) / (w_g_mhz * 1e6)) / (exposure_time * ((r - 1) * (r - 1))),
 *                   se = sqrt(max(var_r, 0)) * slope.  The pair is valid iff a != 0 && r > -1 && r < 0.999 (the open clip interval of the map).  A valid pair with a
 *                   finite se selects the pixel iff se > tol; any other pair selects it iff var_h > 0 || var_t > 0 (no usable estimate, but something varies).  The pixel
 *                   is selected if any pair selects it; metric = the largest finite se over the valid pairs, NaN if there is none.
 * The list of the selected pixels is ascending (wave ballots, block counts, a scan in launches of its own, a scatter: no kernel waits on another block), so a run is
 * reproducible.  count is raised by spp for the selected pixels.
 * BIAS.  Selecting by an estimated variance makes the estimator slightly biased: a pixel whose samples happen to look converged stops early and keeps its chance value.
 * base_passes and spp bound the effect (the estimate that stops a pixel rests on at least base_passes * spp samples).  With a filter wider than the box a pixel's sums hold
 * its neighbours' samples too, so count is the NOMINAL sample count, as with the moment film's statistics. */
#define DTOF_ADAPTIVE_IMAGE    0
#define DTOF_ADAPTIVE_VELOCITY 1
typedef struct {
    int32_t mode;                        /* DTOF_ADAPTIVE_IMAGE | DTOF_ADAPTIVE_VELOCITY */
    int32_t n_pairs;                     /* velocity mode: 1 or 2 pairs */
    int32_t homodyne[2], heterodyne[2];  /* ... variant indices of every pair, homodyne[i] != heterodyne[i] */
    double  tol;                         /* not NaN; +inf selects nothing in image mode */
    double  floor;                       /* image mode: not NaN, >= 0 */
    double  exposure_time, w_g_mhz;      /* velocity mode: finite and > 0 (the doubles of dtof_velocity_map_async) */
} dtof_adaptive_params;
/* The selection over HOST arrays (no scene): planes[P(n_variants)][n_pixels] RAW moment sums (dtof_render_moments with developed == 0), count[n_pixels] read and updated,
 * out_pixels[n_pixels] the ascending list (its first *out_n entries are written), out_metric_or_null[n_pixels].  One upload, the launches, one download.
 * DTOF_ERR_INVALID before any device call: a null argument, n_variants outside 1 .. 4, n_pixels < 0 or > 2^24, spp == 0, an unknown mode, a NaN tol, a floor that is NaN or
 * negative (image), n_pairs outside 1 .. 2, a variant index outside the variants, homodyne == heterodyne, an exposure_time or w_g_mhz that is not finite and > 0
 * (velocity).  Without a device: DTOF_ERR_HIP. */
int dtof_adaptive_select(const double *planes, int64_t n_pixels, int n_variants, const dtof_adaptive_params *params, uint32_t spp, uint32_t *count,
                         uint32_t *out_pixels, uint32_t *out_n, double *out_metric_or_null);
/* ONE traversal of the listed pixels (a HOST list), region-of-interest rendering in its own right: out_moments_or_null receives the P(n_variants) moment planes of
 * crop_height * crop_width doubles (developed != 0: divided by the weight as in dtof_render_moments), out_films_or_null the raw float64 film planes (n_variants, + 1 for an
 * rgba scene: the alpha film, which the moment planes never hold) of crop_height * crop_width * 4 doubles; at least one of the two.  Pixels outside every listed footprint
 * stay 0.  n_pixels == 0 launches nothing.  DTOF_ERR_INVALID before any device call: null arguments, both outputs null, a list that is not strictly ascending or leaves
 * the crop window, the variants refusals of dtof_render_moments, samples_per_pass below the sample count. */
int dtof_render_pixels(dtof_scene *scene, uint32_t seed, uint32_t spp, const uint32_t *pixels, uint32_t n_pixels, const dtof_modulation *variants_or_null, int n_variants,
                       int developed, double *out_moments_or_null, double *out_films_or_null, dtof_render_stats *stats);
/* dtof_sample_lanes_variants over a list: the records of all n_pixels * spp lanes of the listed pixels, pixel by pixel -- record i * spp + j is lane pixels[i] * spp + j
 * of the dense render.  out_lanes12[n_pixels * spp][12], out_valid_or_null[n_pixels * spp], out_rgb_or_null[max(n_variants, 1)][n_pixels * spp][3]. */
int dtof_sample_lanes_pixels(dtof_scene *scene, uint32_t seed, uint32_t spp, const uint32_t *pixels, uint32_t n_pixels, const dtof_modulation *variants_or_null,
                             int n_variants, float *out_lanes12, uint32_t *out_valid_or_null, float *out_rgb_or_null);
/* The adaptive loop.  Passes 0 .. base_passes - 1 are dense, with seeds seed + pass.  Every later pass p < max_passes selects from the cells so far (count = spp * the
 * passes that rendered the pixel); an empty list ends the loop, otherwise the list is rendered with seed + p.  All passes accumulate into ONE moment film and ONE float64
 * film (both splatted from the same traversal).  The host reads 4 bytes per sparse pass: the list's length.
 *   out_moments_or_null  P(n_variants) planes, raw or developed as in dtof_render_moments
 *   out_images_or_null   max(n_variants, 1) float32 images developed from the float64 film (rgb, or rgba for an rgba scene) as dtof_render_variants_f64 develops them
 *   out_films_or_null    the raw float64 film, max(n_variants, 1) (+ 1 for rgba) planes of crop_height * crop_width * 4 doubles
 *   out_count            [crop_height * crop_width] samples rendered in every pixel
 *   out_metric_or_null   [crop_height * crop_width] the metric of the final cells and counts
 *   out_pass_pixels      [max_passes] pixels every pass rendered (a dense pass: all of them; passes that did not run: 0); *out_n_passes: the passes that ran
 *   out_lists_or_null    the lists of the sparse passes one behind the other, at most lists_capacity entries (what does not fit is not written; the lengths tell)
 * `stats` (may be NULL) sums the passes.  DTOF_ERR_INVALID before any device call: null arguments, base_passes == 0, max_passes < base_passes, the refusals of
 * dtof_adaptive_select for `params` and of dtof_render_pixels for the scene and the variants.  Without a device: DTOF_ERR_HIP. */
int dtof_render_adaptive(dtof_scene *scene, uint32_t seed, uint32_t spp, uint32_t base_passes, uint32_t max_passes, const dtof_modulation *variants_or_null,
                         int n_variants, const dtof_adaptive_params *params, int developed, double *out_moments_or_null, float *out_images_or_null,
                         double *out_films_or_null, uint32_t *out_count, double *out_metric_or_null, uint32_t *out_pass_pixels, uint32_t *out_n_passes,
                         uint32_t *out_lists_or_null, uint64_t lists_capacity, dtof_render_stats *stats);

/* Integrator::cancel / should_stop (include/mitsuba/render/integrator.h:96-109). */
void dtof_cancel(dtof_scene *scene);
/* First-bounce launches of this scene, since it was loaded, that ran a kernel compiled with the frame plan's constants (dtof_render_stats::n_plan_facts_launches): the
 * same count for the calls that return no statistics block (the lane dumps). */
uint64_t dtof_scene_plan_facts_launches(const dtof_scene *scene);
/* The FACTS mask (dtof_kernels.h: kFact*) of the first-bounce kernel compiled with plan facts that the scene's last frame launched, 0 if it launched none: tells the
 * instantiations apart, which the count above cannot. */
uint32_t dtof_scene_last_plan_facts(const dtof_scene *scene);
/* Which kernel splatted the last batch of the scene's last frame into the float32 film, and with which shape (csrc/dtof_splat_choice.h: SplatChoice::packed):
 * bits 0-2 the kernel (1 generic, 2 tent3, 3 x8, 4 pixel, 5 the first-bounce kernel itself, "fused"), bits 3-6 the footprint's width in pixels (15: 15 or more),
 * bits 7-11 log2 of the lanes of a segment (tent3: seg, x8: seg8) or of the threads per pixel (pixel: parts), bits 12-31 the samples per thread (pixel: chunk).
 * 0: the frame splatted nothing into a float32 film (no lanes, a lane dump, the float64, moment or aov film).  dtof_render_stats is unchanged. */
uint32_t dtof_scene_last_splat(const dtof_scene *scene);

/* Per-lane debugging entry (SURVEY 8b "dtof_sample_lanes"): evaluates wavefront lanes
 * [lane_begin, lane_begin+n) exactly as dtof_render would (multi-pass renders: index = pass * wavefront_size + lane, a range must stay
 * inside one pass) and returns, per lane,
 * sample_pos[2], time, ray_o[3], ray_d[3], rgb[3] (12 floats) -- the (Spectrum, position) pair that
 * render_sample hands to ImageBlock::put (src/render/integrator.cpp:509-541). */
int dtof_sample_lanes(dtof_scene *scene, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out_lanes12);
/* The same, plus the `valid` half of the (Spectrum, Mask) pair DopplerToFPathIntegrator::sample returns (src/integrators/dopplertofpath.cpp:279-282:
 * valid_ray -- the path met a vertex whose sampled lobe was not BSDFFlags::Null, or the environment is visible): 1 / 0 per lane. */
int dtof_sample_lanes_valid(dtof_scene *scene, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out_lanes12, uint32_t *out_valid);

/* The same through the BATCHED kernels: the lanes are evaluated once for all variants, exactly as dtof_render_variants would, and besides the 12 floats per lane
 * (whose rgb is variant 0's) and the valid flag, out_rgb[n_variants][n][3] receives the result of every lane in every film (max(n_variants, 1) planes) -- per
 * variant the Spectrum that DopplerToFPathIntegrator::sample (src/integrators/dopplertofpath.cpp:79-283) returns with that variant's properties.  out_valid may be NULL. */
int dtof_sample_lanes_variants(dtof_scene *scene, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants,
                               uint64_t lane_begin, uint64_t n, float *out_lanes12, uint32_t *out_valid, float *out_rgb);

/* ---------------------------------------------------------------- sampler surface
 * Array-of-lanes form of the Sampler interface (include/mitsuba/render/sampler.h:99-168) for the
 * correlated sampler; state lives on the GPU, results are copied to caller-owned host arrays of n floats. */
int  dtof_sampler_create(uint32_t sample_count, uint32_t base_seed, int32_t time_correlate_number,
                         int32_t path_correlate_number, dtof_sampler **out);          /* correlated.cpp:17-23 */
void dtof_sampler_destroy(dtof_sampler *s);
int  dtof_sampler_seed(dtof_sampler *s, uint32_t seed, uint32_t wavefront_size);       /* correlated.cpp:38-64 */
int  dtof_sampler_set_samples_per_wavefront(dtof_sampler *s, uint32_t spw);            /* sampler.cpp:75-83 */
int  dtof_sampler_advance(dtof_sampler *s);                                            /* sampler.cpp:52-55 */
int  dtof_sampler_next_1d(dtof_sampler *s, float *out);                                /* correlated.cpp:79-84 */
int  dtof_sampler_next_2d(dtof_sampler *s, float *out_xy);                             /* correlated.cpp:86-90, n*2 */
/* correlate: per-lane flags (n bytes) or NULL to use `correlate_all` for every lane. */
int  dtof_sampler_next_1d_correlate(dtof_sampler *s, const uint8_t *correlate, int correlate_all, float *out);  /* :156-161 */
int  dtof_sampler_next_2d_correlate(dtof_sampler *s, const uint8_t *correlate, int correlate_all, float *out_xy); /* :163-167 */
/* strategy: ETimeSampling (sampler.h:27-34): 0 uniform, 1 stratified, 2 antithetic, 3 antithetic_mirror (time_correlate_number must be 2, correlated.cpp:142),
 * 4 periodic (correlated.cpp:147-150), 5 regular (falls through to `return r`, :152) */
int  dtof_sampler_next_1d_time(dtof_sampler *s, int strategy, float antithetic_shift, int stratify_each_interval, float *out); /* :92-153 */
/* state readback: 7 uint32 per lane = rng.state lo,hi, rng_time.state lo,hi, rng_path.state lo,hi, permutation seed */
int  dtof_sampler_get_state(dtof_sampler *s, uint32_t *out7);
/* Sampler::fork (src/samplers/correlated.cpp:25-32): same configuration, unseeded.  Sampler::clone (:34-36): same configuration and
 * the same per-lane state, so both produce the same numbers from here on.  set_sample_count / seeded: include/mitsuba/render/sampler.h:129,141.
 * (schedule_state / loop_put of the reference are Dr.Jit loop plumbing and have no counterpart here.) */
int  dtof_sampler_fork(const dtof_sampler *s, dtof_sampler **out);
int  dtof_sampler_clone(const dtof_sampler *s, dtof_sampler **out);
int  dtof_sampler_set_sample_count(dtof_sampler *s, uint32_t sample_count);
int  dtof_sampler_seeded(const dtof_sampler *s);
uint32_t dtof_sampler_wavefront_size(const dtof_sampler *s);
uint32_t dtof_sampler_sample_count(const dtof_sampler *s);

/* ---------------------------------------------------------------- modulation functions
 * eval_modulation_weight (dopplertofpath.cpp:60-77) and the waveform library
 * (include/mitsuba/render/waveform_utils.h:24-62) over arrays, evaluated by the same device functions the
 * shade kernel uses.  mode 0: weight(ray_time=t[i], path_length=len[i]) with the scene's integrator;
 * mode 1: eval_modulation_function_value(t[i]); mode 2: ..._low_pass(t[i]). */
int dtof_eval_modulation(dtof_scene *scene, int mode, const float *t, const float *len, float *out, uint32_t n);

/* ---------------------------------------------------------------- ray queries
 * Scene::ray_intersect / Scene::ray_test (include/mitsuba/render/scene.h; src/render/scene.cpp -> scene_embree.inl:202-333,349-426) over
 * arrays, through the same TLAS / BLAS traversal and surface-interaction code the render kernels use.  rays8: per ray o[3], d[3], time,
 * maxt.  out19: t (inf on a miss), p[3], n[3], sh_frame.n[3], sh_frame.s[3], sh_frame.t[3], wi[3]; ids3: object, shape-in-group,
 * primitive (-1 on a miss; a triangle is named by its face index in the mesh's own order, PreliminaryIntersection::prim_index).  dtof_ray_test writes 1 / 0 per ray. */
int dtof_ray_intersect(dtof_scene *scene, uint32_t n, const float *rays8, float *out19, int32_t *ids3);
/* the same, plus uv4 per ray: si.uv[2] (the surface parameterisation, interaction.h) and pi.prim_uv[2] (PreliminaryIntersection::prim_uv: the barycentric
 * coordinates on a triangle, the local position on a rectangle or disk), as the reference's tests of meshes assert them (src/render/tests/test_mesh.py:258-292) */
int dtof_ray_intersect_uv(dtof_scene *scene, uint32_t n, const float *rays8, float *out19, int32_t *ids3, float *uv4);
int dtof_ray_test(dtof_scene *scene, uint32_t n, const float *rays8, int32_t *occluded);
/* The ray query of the fused kernels of FLAT scenes (rectangles only, at most 8 top-level objects: every ray tests them all, no tree) over arrays, through the
 * instantiations of that query the shade kernels carry.  form 0: the generic walk; 1: the one-wall walk (exactly one instance, of one rectangle); 2: the walk compiled
 * for the headline's table (5 rectangles, the wall at index 2).  rays8 as above.  any = 0: closest hit, out3 = t, u, v (inf, 0, 0 on a miss), ids = the object (-1 on a
 * miss); any != 0: occlusion, ids = 1 / 0 (out3 is not written).  DTOF_ERR_INVALID, before anything is launched, for a scene without a flat table, a form whose facts
 * the scene does not meet, and n above 2^24; non-finite ray components are taken as they are. */
int dtof_flat_query(dtof_scene *scene, int form, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids);
/* The same through the PAIR form of the walk of form 2, which a frame's kernel runs where the two lanes of a correlated pair hold the same ray: n is even, rays 2k
 * and 2k + 1 are equal in o, d and maxt bit for bit (their times are their own), and each pair shares the plain rectangles between its two lanes.  Results as above.
 * DTOF_ERR_INVALID, before anything is launched, for an odd n, a pair that differs and a table other than 5 rectangles with the wall at index 2. */
int dtof_flat_query_pairs(dtof_scene *scene, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids);
/* The same through the walk of form 2 with the z rows of its four plain rectangles computed on the matrix cores (six 4x4x1 f32 MFMAs per ray, issued by every lane
 * of a wave in front of the query), which a frame's kernel runs for a vertex's shadow and continuation rays.  Results as above.  zrow8 (may be null): per ray the
 * eight MFMA values -- the local z of the origin in rectangles 0, 1, 3, 4, then that of the direction -- bit for bit the fmaf chains of the other forms.
 * DTOF_ERR_INVALID, before anything is launched, for a table other than 5 rectangles with the wall at index 2 and for n above 2^24. */
int dtof_flat_query_zrow(dtof_scene *scene, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids, float *zrow8);
/* Lane generation of the headline frame's kernel over arrays: lanes [lane_begin, lane_begin + n) of a render with `seed` and `spp`, walked in 512-lane segments of
 * 64-lane chunks as the first-bounce launch walks them.  form 0: every lane generates itself; form 1: what lanes 2k and 2k + 1 share -- path stream, pixel jitter,
 * sample position, camera ray -- is evaluated once per pair, for the pairs of two consecutive chunks at a time, and fetched by both lanes.  out16: 16 words per lane --
 * sample position[2], time, o[3], d[3], maxt (floats), the path stream's state after the two jitter draws (low, high word), its selector, and three zeros.  The first
 * nine equal dtof_sample_lanes.  DTOF_ERR_INVALID, before anything is launched, for a scene or sample count that does not meet the facts the kernels are compiled with
 * (one pass, dopplertofpath with the correlated sampler, stratified pairs, a power-of-two stratum count, spp a power of two >= 64, the perspective camera), for a
 * lane_begin or n that is not a multiple of 64, for n above 2^24 and for a range beyond the wavefront. */
int dtof_pair_setup_lanes(dtof_scene *scene, int form, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, uint32_t *out16);
/* The TLAS / BLAS ray query (every scene with a mesh, a sphere, more than eight objects or a BLAS) over arrays, through the instantiations of it that the ray kernels
 * of a frame carry.  form 0: float nodes and a 32-bit LDS stack (what dtof_ray_intersect runs); 1: half-float nodes, a 16-entry LDS stack with a private overflow
 * array, triangle and rectangle code only; 2: form 1 with the TLAS nodes read from a copy in LDS; 3: the two-launch pair of form 1 -- the TLAS walk puts the meshes
 * behind a BLAS aside, a second walk enters them -- run by one lane on its own candidate list (the same device functions as the two launches, without the queue
 * compaction between them); 4: half-float nodes with every shape's code.  rays8 as above.  any = 0: closest hit, out3 = t, u, v (inf, 0, 0 on a miss), ids3 = object,
 * shape in its group, primitive (-1 on a miss); any != 0: occlusion, ids3[i] = 1 / 0 (one word per ray, out3 is not written).  DTOF_ERR_INVALID, before anything is
 * launched or written, for a form the scene does not meet -- no half-float nodes (forms 1 to 4), an analytic shape, a stack deeper than 64 entries or a TLAS of more
 * than 16 nodes for form 2 (forms 1 to 3) -- and for n above 2^24; non-finite ray components are taken as they are. */
int dtof_tree_query(dtof_scene *scene, int form, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids3);
/* The tree walk that the FUSED shade kernels run themselves, over arrays, with the instance memo and the stack columns laid out as those kernels lay them out.
 * form 0 (classic): one wave per block, float nodes, every shape's code, the blob staged in LDS when it is at most 16 KiB; 1 (classic_rect): form 0 with rectangle
 * code only; 2 (resident): blocks of `waves` waves (8, 12 or 16) whose LDS holds the TLAS as four planes of node pieces and the scene's record block; 3
 * (resident_16): form 2 with 16-bit child references and 16-bit stack columns; 4 (resident_half): form 2 with two planes of half-float node pieces; 5
 * (resident_half_16): form 4 with the 16-bit references.  `waves` is read by forms 2 to 5 only.  Rays and answers as dtof_tree_query.  DTOF_ERR_INVALID, before
 * anything is launched or written and with a message that begins "dtof_fused_query:", for a form the scene does not meet -- a shape other than a rectangle (form
 * 1); no resident layout (a blob above 16 KiB whose record block is within 24 KiB), a mesh behind a BLAS, more than 1 024 nodes (forms 2, 3), no half-float nodes or
 * a node count outside 1 025 .. 2 048 (forms 4, 5), 0x7fff objects or more (forms 3, 4, 5), an LDS total above the device's limit, `waves` other than 8, 12 or 16 --
 * for n above 2^24 and for null arguments; non-finite ray components are taken as they are. */
int dtof_fused_query(dtof_scene *scene, int form, int waves, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids3);
/* The surface-interaction fill (PreliminaryIntersection::compute_surface_interaction, include/mitsuba/render/interaction.h:675-701, through the shapes' and the
 * instance's own, and Interaction::offset_p, :161-165) over arrays of HITS, through the instantiations and argument patterns of it that the kernels of a frame
 * carry.  A hit is given, not traced: in10 = o[3], d[3], time, t, b1, b2 (prim_uv); ids3 = object, shape in its group, primitive -- a triangle by its index IN THE
 * BLAS'S ORDER (dtof_scene_export kind 27 maps faces to it), ignored for any other shape.  form 0: the mesh kernels' instantiation, the instance matrix derived per
 * hit; 1: the rectangle-only kernels', no instance memo; 2: ... with the scene's one instance as the memo object, its matrix from registers and its inverse read
 * back from the lane's LDS column; 3: ... both read back from LDS; 4: the one-wall kernels' with their precomputed frames; 5: form 0 with the memo object's
 * matrices from registers.  want_frame = 0: the form in which a caller reads the cosine wi.z only.  out32 = p, n, sh_frame.n, sh_frame.s, sh_frame.t, wi (3 each),
 * uv[2], dp_du[3], dp_dv[3], offset_p(d)[3], offset_p(-d)[3]; with want_frame = 0 sh_frame.s / .t, dp_du, dp_dv and wi.x / .y are +0, and form 4 reports dp_du =
 * dp_dv = +0 always (no kernel of that form reads them).  DTOF_ERR_INVALID, before anything is launched or written, for a scene without a device blob, a form the
 * scene does not meet -- a shape that is no rectangle or a blob above the 16 KiB LDS stage (forms 1 to 4), no single instance (2, 3, 5), a flat table without the one-wall fact (4) -- an id out of
 * range (object, shape beyond its group, primitive beyond a mesh's triangles) and n above 2^24; non-finite floats are taken as they are. */
int dtof_surface_eval(dtof_scene *scene, int form, int want_frame, uint32_t n, const float *in10, const int32_t *ids3, float *out32);

/* ---------------------------------------------------------------- component evaluation
 * The device functions the shade and splat kernels are built from, evaluated over arrays on the GPU: the counterpart of the
 * free functions / small classes the reference exposes to its unit tests (mi.fresnel, mi.MicrofacetDistribution, mi.warp.*,
 * ReconstructionFilter::eval, ...), so that the reference's own known answers (tests/golden/reference_kats.json.gz) can be held
 * against the GPU code.  Element i reads in[i * in_stride ...] and writes out[i * out_stride ...]; `params` are per-call scalars. */
#define DTOF_COMP_MICROFACET_EVAL          0   /* MicrofacetDistribution::eval (microfacet.h:176-196). params: type (0 beckmann, 1 ggx), alpha_u, alpha_v, sample_visible; in m[3]; out 1 */
#define DTOF_COMP_MICROFACET_PDF           1   /* ::pdf (:219-228); in wi[3], m[3]; out 1 */
#define DTOF_COMP_MICROFACET_G1            2   /* ::smith_g1 (:341-365); in v[3], m[3]; out 1 */
#define DTOF_COMP_MICROFACET_SAMPLE        3   /* ::sample (:240-325); in wi[3], sample[2]; out m[3], pdf */
#define DTOF_COMP_FRESNEL                  4   /* fresnel (fresnel.h:21-63). params: eta; in cos_theta_i; out r, cos_theta_t, eta_it, eta_ti */
#define DTOF_COMP_FRESNEL_CONDUCTOR        5   /* fresnel_conductor (fresnel.h:93-117). params: eta, k; in cos_theta_i; out 1 */
#define DTOF_COMP_RFILTER                  6   /* ReconstructionFilter::eval. params: kind (0 box, 1 tent, 2 gaussian, 3 mitchell, 4 catmullrom, 5 lanczos: radius = lobes), radius, stddev, B, C; in x; out 1 */
#define DTOF_COMP_WARP_COSINE_HEMISPHERE   7   /* warp::square_to_cosine_hemisphere (warp.h:320-344); in sample[2]; out 3 */
#define DTOF_COMP_WARP_DISK_CONCENTRIC     8   /* warp::square_to_uniform_disk_concentric (warp.h:54-90); out 2 */
#define DTOF_COMP_WARP_UNIFORM_TRIANGLE    9   /* warp::square_to_uniform_triangle (warp.h:153-156); out 2 */
#define DTOF_COMP_WARP_UNIFORM_SPHERE     10   /* warp::square_to_uniform_sphere (warp.h:250-255); out 3 */
#define DTOF_COMP_COORDINATE_SYSTEM       11   /* coordinate_system (vector.h:116-136) = Frame3f(n); in n[3]; out s[3], t[3] */
#define DTOF_COMP_TEA_FLOAT32             12   /* sample_tea_float32 (random.h:33-67), 4 rounds; in v0, v1 (uint32 bit patterns); out 1 */
#define DTOF_COMP_MATH                    13   /* restated Dr.Jit math. params: 0 exp, 1 log, 2 tan, 3 erf, 4 erfinv, 5 sin, 6 cos, 7 acos; in x; out 1 */
int dtof_eval_component(int component, const float *params, int n_params, const float *in, int in_stride, float *out, int out_stride, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif
