// dtof_abi_films.hip -- the C ABI (include/dtof.h) of rendering: every entry that renders into a film (the caller's device film, the library's own float32 / float64
// film, the moment and aov cells, lane dumps), develops one, reconstructs the radial-velocity map or denoises -- the denoised renders that do all of that from one
// traversal among them -- and dtof_async_collect.  All of them end in render_rows
// (dtof_render.hip) or in one of the launchers of the small kernel files.
#include "dtof_host.h"
#include "dtof_develop.h"
#include "dtof_reconstruct.h"
#include "dtof_depth.h"
#include "dtof_denoise.h"
#include "dtof_denoise_inputs.h"
#include "dtof_temporal.h"
#include "dtof_world_to_pixel.h"
#include "dtof_moments.h"
#include "dtof_adaptive.h"
#include <cmath>

using namespace dtof;

// film elements (4 per pixel) of the rows a call that renders rows [row_lo, row_hi) can write: the rows and the filter's halo on either side, inside the film
static uint64_t film_rows_reach(const HostSensor &se, int32_t row_lo, int32_t row_hi, int32_t *first = nullptr, int32_t *end = nullptr) {
    const int32_t halo = se.filter == FILTER_BOX ? 0 : (int32_t) std::ceil(se.filter_radius - .5f);
    const int32_t r0 = std::max(row_lo, 0), r1 = std::min(row_hi, se.crop_h);
    const int32_t lo = std::max(r0 - halo, 0), hi = std::min(r1 + halo, se.crop_h);
    if (first) *first = lo;
    if (end) *end = hi;
    return r1 > r0 ? (uint64_t) (hi - lo) * se.crop_w * 4 : 0;   // an empty band writes nothing
}
// ... which a plane stride (0: dense planes) of a film of several planes must hold, or plane k + 1 would be added into plane k; `what` and `unit` name it in the refusal
static void check_stride_reach(const HostSensor &se, uint64_t stride, int32_t row_lo, int32_t row_hi, const char *what, const char *unit) {
    int32_t lo = 0, hi = 0;
    const uint64_t reach = film_rows_reach(se, row_lo, row_hi, &lo, &hi);
    if (stride != 0 && stride < reach)
        throw std::runtime_error(std::string("the ") + what + " of " + std::to_string(stride) + " " + unit + " is smaller than the " + std::to_string(reach) + " " + unit +
                                 " of film rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") this call writes: the planes would overlap");
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
    if (need > 1) check_stride_reach(se, sc->film_plane_stride, row_lo, row_hi, "declared plane stride", "floats");
    return sc->film_plane_stride ? sc->film_plane_stride : (uint64_t) se.crop_w * se.crop_h * 4;
}
// the rows [first, last + 1) that hold the stripes [first_row + k * stripe_period, ... + stripe_rows) below the film's height (the mapping of plan_lanes)
static std::pair<int32_t, int32_t> stripe_span(const dtof_scene *sc, int32_t first_row, int32_t stripe_rows, int32_t stripe_period) {
    const int32_t h = sc->host.sensor.crop_h, first = std::max(first_row, 0);
    const int64_t span = std::max<int64_t>(h - first, 0), v_rows = (span / stripe_period) * stripe_rows + std::min<int64_t>(span % stripe_period, stripe_rows);
    if (v_rows == 0) return {first, first};
    return {first, (int32_t) (first + ((v_rows - 1) / stripe_rows) * stripe_period + (v_rows - 1) % stripe_rows + 1)};
}

// The refusal of an exposure time or a modulation frequency that is a NaN, infinite or not above 0; `name` is how the entry's documentation calls the argument
static bool finite_positive(double v) { return std::isfinite(v) && v > 0; }
static void need_finite_positive(double v, const std::string &name) { if (!finite_positive(v)) throw std::runtime_error(name + " must be finite and > 0"); }

// The variants arguments of the C ABI as a request carries them: NULL / 0 = the integrator's own pair; the count is checked here, before anything is enqueued
static void set_variants(RenderRequest &rq, const dtof_modulation *variants, int n_variants) {
    if (!variants || n_variants <= 0) return;
    if (n_variants > kMaxOffsets) throw std::runtime_error("at most 4 modulation variants can be batched per traversal");
    rq.variants = variants; rq.n_variants = n_variants;
}
// ... and of the `_freq` entries: a frequency per variant, or null = the entry without `_freq`.  Frequencies without variants and a frequency that is not finite or
// not > 0 are refused here, before anything is enqueued
static void set_variants_freq(RenderRequest &rq, const dtof_modulation *variants, const float *w_g_mhz, int n_variants) {
    set_variants(rq, variants, n_variants);
    if (!w_g_mhz) return;
    if (rq.n_variants <= 0) throw std::runtime_error("modulation frequencies come with the variants they belong to: variants is null or n_variants is not positive");
    for (int k = 0; k < n_variants; ++k) need_finite_positive(w_g_mhz[k], "w_g_mhz[" + std::to_string(k) + "]");
    rq.w_g_mhz = w_g_mhz;
}
// The device-film entry points: a rows or stripes request with the call's offsets or variants (their count is refused before a null scene or film is), the null and
// stripe checks, the caller's film layout, and for the async forms the events a refused frame took go back to the pool
static int device_film(dtof_scene *sc, RenderRequest rq, const float *offsets, int n_offsets, const dtof_modulation *variants, int n_variants, float *d_film) {
    return guarded([&] {
        rq.offsets = offsets; rq.n_offsets = n_offsets; rq.film = d_film;
        set_variants(rq, variants, n_variants);
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
    });
}

// The library's own film, float32 or float64: the buffer it lives in, the fields of a request that name it, and whether its host-buffer render asks for the sensor
// before the first HIP call (the float64 one does; the float32 one leaves that to render_rows, behind ensure_device).  Its develop is overloaded (dtof_develop.h)
template <typename T> struct OwnFilm;
template <> struct OwnFilm<float> {
    static constexpr bool sensor_first = false;
    static DevBuf<float> &buf(dtof_scene *sc) { return sc->d_film; }
    static void attach(RenderRequest &rq, float *film, uint64_t stride) { rq.film = film; rq.film_stride = stride; }
};
template <> struct OwnFilm<double> {
    static constexpr bool sensor_first = true;
    static DevBuf<double> &buf(dtof_scene *sc) { return sc->d_film64; }
    static void attach(RenderRequest &rq, double *film, uint64_t stride) { rq.film64 = film; rq.film64_stride = stride; }
};
// The k dense colour planes of an own film of px pixels (the alpha plane of an rgba scene behind them) developed into sc->d_rgb and copied out: [k][px][3 or 4]
template <typename T> static void develop_and_copy(dtof_scene *sc, const T *film, int k, size_t px, float *out) {
    const bool alpha = sc->host.sensor.alpha;   // rgba: four channels out
    const size_t ch = alpha ? 4 : 3;
    sc->d_rgb.ensure(px * ch * k);
    if (alpha) for (int i = 0; i < k; ++i) launch_develop_rgba(film + px * 4 * i, film + px * 4 * k, sc->d_rgb.p + px * 4 * i, (int64_t) px, sc->stream);
    else launch_develop(film, k, 0, sc->d_rgb.p, (int64_t) px, sc->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, sc->d_rgb.p, px * ch * k * sizeof(float), hipMemcpyDeviceToHost, sc->stream));
}
// `planes` planes of the moment cells (sc->d_moments; sc->d_moment_planes is sized by the caller, before its passes) developed and copied out
static void develop_cells_and_copy(dtof_scene *sc, int planes, int developed, size_t px, double *out) {
    launch_develop_moments(sc->d_moments.p, planes, developed != 0, sc->d_moment_planes.p, (int64_t) px, sc->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, sc->d_moment_planes.p, px * planes * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
}

// The host-buffer renders (dtof_render_offsets / _variants / _variants_f64): the library's own film of rq.films() colour planes (and the alpha plane), developed into
// out_rgb; out_films: the raw film planes as well, or null
template <typename T> static void render_host_films(dtof_scene *sc, RenderRequest rq, float *out_rgb, T *out_films = nullptr) {
    using F = OwnFilm<T>;
    if (!sc || !out_rgb) throw std::runtime_error("null argument");
    need_doppler_for(sc, rq.n_variants > 0);   // before the film is cleared
    if (F::sensor_first) need_sensor(sc);
    ensure_device(sc);
    sc->stop = false;
    const int k = rq.films();
    const HostSensor &se = sc->host.sensor;
    const size_t px = (size_t) se.crop_w * se.crop_h;
    const int planes = k + (se.alpha ? 1 : 0);   // rgba: one more film plane for the alpha channel
    F::buf(sc).ensure(px * 4 * planes);
    T *const film = F::buf(sc).p;
    HIP_CHECK(hipMemsetAsync(film, 0, px * 4 * planes * sizeof(T), sc->stream));
    rq.row_begin = 0; rq.row_end = se.crop_h;
    F::attach(rq, film, px * 4);
    render_rows(sc, rq);
    develop_and_copy(sc, film, k, px, out_rgb);
    if (out_films) HIP_CHECK(hipMemcpyAsync(out_films, film, px * 4 * planes * sizeof(T), hipMemcpyDeviceToHost, sc->stream));
    HIP_CHECK(hipStreamSynchronize(sc->stream));
}

extern "C" {

int dtof_render_rows(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                     const float *offsets, int n_offsets, float *d_film, dtof_render_stats *stats) {
    return device_film(sc, rows_request(seed, spp, row_begin, row_end, stats), offsets, n_offsets, nullptr, 0, d_film);
}
int dtof_render_rows_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end, const float *offsets, int n_offsets, float *d_film) {
    return device_film(sc, rows_request(seed, spp, row_begin, row_end, nullptr, true), offsets, n_offsets, nullptr, 0, d_film);
}
int dtof_render_stripes(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                        const float *offsets, int n_offsets, float *d_film, dtof_render_stats *stats) {
    return device_film(sc, stripes_request(seed, spp, first_row, stripe_rows, stripe_period, stats), offsets, n_offsets, nullptr, 0, d_film);
}
int dtof_render_stripes_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                              const float *offsets, int n_offsets, float *d_film) {
    return device_film(sc, stripes_request(seed, spp, first_row, stripe_rows, stripe_period, nullptr, true), offsets, n_offsets, nullptr, 0, d_film);
}
int dtof_render_rows_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                              const dtof_modulation *variants, int n_variants, float *d_film, dtof_render_stats *stats) {
    return device_film(sc, rows_request(seed, spp, row_begin, row_end, stats), nullptr, 0, variants, n_variants, d_film);
}
int dtof_render_rows_variants_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end,
                                    const dtof_modulation *variants, int n_variants, float *d_film) {
    return device_film(sc, rows_request(seed, spp, row_begin, row_end, nullptr, true), nullptr, 0, variants, n_variants, d_film);
}
int dtof_render_stripes_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                                 const dtof_modulation *variants, int n_variants, float *d_film, dtof_render_stats *stats) {
    return device_film(sc, stripes_request(seed, spp, first_row, stripe_rows, stripe_period, stats), nullptr, 0, variants, n_variants, d_film);
}
int dtof_render_stripes_variants_async(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t first_row, int32_t stripe_rows, int32_t stripe_period,
                                       const dtof_modulation *variants, int n_variants, float *d_film) {
    return device_film(sc, stripes_request(seed, spp, first_row, stripe_rows, stripe_period, nullptr, true), nullptr, 0, variants, n_variants, d_film);
}

int dtof_render_offsets(dtof_scene *sc, uint32_t seed, uint32_t spp, const float *offsets, int n_offsets, float *out_rgb, dtof_render_stats *stats) {
    return guarded([&] { RenderRequest rq = rows_request(seed, spp, 0, 0, stats); rq.offsets = offsets; rq.n_offsets = n_offsets; render_host_films<float>(sc, rq, out_rgb); });
}
int dtof_render_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants, float *out_rgb, dtof_render_stats *stats) {
    return guarded([&] { RenderRequest rq = rows_request(seed, spp, 0, 0, stats); set_variants(rq, variants, n_variants); render_host_films<float>(sc, rq, out_rgb); });
}
int dtof_render_variants_f64(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants, float *out_images, double *out_films,
                             dtof_render_stats *stats) {
    return guarded([&] { RenderRequest rq = rows_request(seed, spp, 0, 0, stats); set_variants(rq, variants, n_variants); render_host_films<double>(sc, rq, out_images, out_films); });
}
int dtof_render_variants_freq(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, const float *w_g_mhz, int n_variants, float *out_rgb,
                              dtof_render_stats *stats) {
    return guarded([&] { RenderRequest rq = rows_request(seed, spp, 0, 0, stats); set_variants_freq(rq, variants, w_g_mhz, n_variants); render_host_films<float>(sc, rq, out_rgb); });
}
int dtof_render_variants_freq_f64(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, const float *w_g_mhz, int n_variants, float *out_images,
                                  double *out_films, dtof_render_stats *stats) {
    return guarded([&] { RenderRequest rq = rows_request(seed, spp, 0, 0, stats); set_variants_freq(rq, variants, w_g_mhz, n_variants); render_host_films<double>(sc, rq, out_images, out_films); });
}
int dtof_render(dtof_scene *sc, uint32_t sensor_index, uint32_t seed, uint32_t spp, float *out_rgb, dtof_render_stats *stats) {
    if (sensor_index != 0) { g_last_error = "Scene::render(): sensor index " + std::to_string(sensor_index) + " is out of bounds!"; return DTOF_ERR_INVALID; }
    return dtof_render_offsets(sc, seed, spp, nullptr, 0, out_rgb, stats);
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
        launch_develop(d_film, 1, 0, d_rgb, n_pixels, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
// one frame's statistics added to a sum: every field of dtof_render_stats
static void add_stats(dtof_render_stats &sum, const dtof_render_stats &f) {
    sum.n_paths += f.n_paths; sum.n_bounces += f.n_bounces; sum.n_shadow_rays += f.n_shadow_rays;
    sum.ms_total += f.ms_total; sum.ms_generate += f.ms_generate; sum.ms_trace += f.ms_trace; sum.ms_shade += f.ms_shade; sum.ms_shadow += f.ms_shadow; sum.ms_splat += f.ms_splat;
    sum.n_launches_trace += f.n_launches_trace; sum.n_launches_shade += f.n_launches_shade; sum.n_launches_shadow += f.n_launches_shadow; sum.n_batches += f.n_batches;
    sum.n_launches_first += f.n_launches_first; sum.ms_first += f.ms_first; sum.n_inline_iterations += f.n_inline_iterations; sum.n_bounces_inline += f.n_bounces_inline;
    sum.n_fused_splat_launches += f.n_fused_splat_launches; sum.n_plan_facts_launches += f.n_plan_facts_launches;
}
// one finished deferred frame added to a statistics block (its stream has been waited for); returns the frame's duration.  The frame's counters (render_rows: paths,
// batches and launches; the ray counts, which a deferred frame does not read back, hold 0) with the times its events give
static float add_deferred_frame(dtof_render_stats *sum, const dtof_scene::DeferredFrame &f) {
    float t = 0; HIP_CHECK(hipEventElapsedTime(&t, f.ev0, f.ev1));
    dtof_render_stats frame = f.counters;
    frame.ms_total = t;
    frame.ms_generate = stage_ms(f.ev[kStageGenerate]); frame.ms_trace = stage_ms(f.ev[kStageTrace]); frame.ms_first = stage_ms(f.ev[kStageFirst]);
    frame.ms_shade = stage_ms(f.ev[kStageShade]) + frame.ms_first; frame.ms_shadow = stage_ms(f.ev[kStageShadow]); frame.ms_splat = stage_ms(f.ev[kStageSplat]);
    add_stats(*sum, frame);
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
    need_finite_positive(exposure_time, "exposure_time");
    need_finite_positive(w_g_mhz, "w_g_mhz");
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
        check_plane_stride(plane_stride_floats, (uint64_t) n_pixels * 4, "floats", "n_pixels * 4");
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
}  // extern "C"
// The deferred frames a call enqueues itself, from this object's construction on: the passes of a reconstructed map, which run without a host wait in between.
// collect() is the call's one synchronisation and hands their sum out; leaving the scope, by return or by exception, takes them off sc->deferred (after a wait if they
// may still be in flight) and gives their events back to the pool once no frame is left.  Frames the caller has not collected yet stay theirs.
struct OwnFrames {
    dtof_scene *const sc; const size_t first; bool waited = false;
    explicit OwnFrames(dtof_scene *scene) : sc(scene), first(scene->deferred.size()) {}
    OwnFrames(const OwnFrames &) = delete;
    void collect(dtof_render_stats *stats) {
        HIP_CHECK(hipStreamSynchronize(sc->stream));
        waited = true;
        dtof_render_stats sum; memset(&sum, 0, sizeof sum);
        for (size_t i = first; i < sc->deferred.size(); ++i) add_deferred_frame(&sum, sc->deferred[i]);
        if (stats) *stats = sum;
    }
    ~OwnFrames() {
        if (sc->deferred.size() > first) { if (!waited) (void) hipStreamSynchronize(sc->stream); sc->deferred.resize(first); }
        if (sc->deferred.empty()) sc->events_used = 0;
    }
};
// What both reconstructed maps render: n_films variants (w_g_mhz: a frequency for each, or null) in groups of at most kMaxOffsets films, n_passes passes each (seed =
// pass), into the library's own float32 or float64 film; every pass is developed and added into sc->d_vm_sum [n_films][px][3].  Every frame is deferred (the caller
// holds an OwnFrames); the library's own film: the caller's declared layout is not consulted
template <typename T> static void render_passes_into_sum(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const dtof_modulation *variants, const float *w_g_mhz, int n_films) {
    using F = OwnFilm<T>;
    const HostSensor &se = sc->host.sensor;
    const size_t px = (size_t) se.crop_w * se.crop_h;
    const int alpha = se.alpha ? 1 : 0;
    F::buf(sc).ensure(px * 4 * (kMaxOffsets + alpha));
    sc->d_vm_sum.ensure(px * 3 * n_films);
    T *const film = F::buf(sc).p;
    for (int g = 0; g < n_films; g += kMaxOffsets) {
        const int films = std::min(kMaxOffsets, n_films - g);
        for (uint32_t pass = 0; pass < n_passes; ++pass) {
            HIP_CHECK(hipMemsetAsync(film, 0, px * 4 * (films + alpha) * sizeof(T), sc->stream));
            dtof_render_stats frame;
            RenderRequest rq = rows_request(pass, spp, 0, se.crop_h, &frame, true);
            F::attach(rq, film, px * 4);
            set_variants_freq(rq, variants + g, w_g_mhz ? w_g_mhz + g : nullptr, films);
            render_rows(sc, rq);
            launch_develop_accumulate(film, films, 0, sc->d_vm_sum.p + px * 3 * g, (int64_t) px, pass == 0, sc->stream);   // the alpha plane behind them is left out
        }
    }
}
// dtof_render_velocity_map / _f64 over the library's own float32 or float64 film: the homodyne / heterodyne films of dtof_velocity_map_variants, k_velocity_map
template <typename T> static void velocity_map_render(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                                                      double *out_velocity, double *out_velocity_pairs, float *out_tof, dtof_render_stats *stats) {
    if (!sc || !offsets || !out_velocity) throw std::runtime_error("null argument");
    if (n_offsets < 1 || n_offsets > kMaxVelocityPairs) throw std::runtime_error("between 1 and 16 offsets make a velocity map");
    check_velocity_scalars(n_passes, exposure_time, w_g_mhz);
    need_doppler_for(sc, true);
    need_sensor(sc);
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
    const size_t px = (size_t) sc->host.sensor.crop_w * sc->host.sensor.crop_h;
    sc->d_vm_tof.ensure(px * 2 * n_offsets); sc->d_vm_maps.ensure(px * (n_offsets + 1));
    double *const d_pairs = sc->d_vm_maps.p + px;
    const hipStream_t s = sc->stream;
    OwnFrames frames(sc);
    render_passes_into_sum<T>(sc, n_passes, spp, variants, nullptr, 2 * n_offsets);
    launch_velocity_map(sc->d_vm_sum.p, a, (int64_t) px, out_tof ? sc->d_vm_tof.p : nullptr, out_velocity_pairs ? d_pairs : nullptr, sc->d_vm_maps.p, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out_velocity, sc->d_vm_maps.p, px * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_velocity_pairs) HIP_CHECK(hipMemcpyAsync(out_velocity_pairs, d_pairs, px * n_offsets * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_tof) HIP_CHECK(hipMemcpyAsync(out_tof, sc->d_vm_tof.p, px * 2 * n_offsets * sizeof(float), hipMemcpyDeviceToHost, s));
    frames.collect(stats);
}

// ---------------------------------------------------------------- depth map (dtof_depth.hip)
// The checks the entries share, made before a device is touched: the count, which every entry looks at before it reads an array of that length, and the frequencies
// as the doubles the kernel's wavelengths are formed from
static void check_depth_count(int n_frequencies) {
    if (n_frequencies < 1 || n_frequencies > kMaxDepthFrequencies) throw std::runtime_error("between 1 and 4 modulation frequencies make a depth map");
}
static void check_depth_frequencies(const double *w_g_mhz, int n_frequencies) {
    check_depth_count(n_frequencies);
    for (int j = 0; j < n_frequencies; ++j) {
        need_finite_positive(w_g_mhz[j], "w_g_mhz[" + std::to_string(j) + "]");
        for (int k = 0; k < j; ++k) if (w_g_mhz[k] == w_g_mhz[j]) throw std::runtime_error("the modulation frequencies of a depth map must be distinct");
    }
}
static DepthMapArgs depth_args(int n_frequencies, const int32_t *i_planes, const int32_t *q_planes, const double *w_g_mhz, uint32_t n_passes, double exposure_time,
                               double max_path_length) {
    check_depth_frequencies(w_g_mhz, n_frequencies);
    if (n_passes == 0) throw std::runtime_error("n_passes must be at least 1");
    need_finite_positive(exposure_time, "exposure_time");
    DepthMapArgs a; memset(&a, 0, sizeof a);
    a.n_frequencies = n_frequencies; a.n_candidates = 1;
    for (int j = 0; j < n_frequencies; ++j) {
        if (i_planes[j] < 0 || i_planes[j] >= 2 * n_frequencies || q_planes[j] < 0 || q_planes[j] >= 2 * n_frequencies)
            throw std::runtime_error("frequency " + std::to_string(j) + ": plane index outside the " + std::to_string(2 * n_frequencies) + " planes of the sum");
        a.i_plane[j] = i_planes[j]; a.q_plane[j] = q_planes[j];
        a.wavelength[j] = 300.0 / w_g_mhz[j];
    }
    if (n_frequencies > 1) {   // N = (int64) floor(max_path_length / L_0) + 1 candidates of the first frequency's wrap count
        const double q = std::floor(max_path_length / a.wavelength[0]);
        if (!(q >= 0.0) || !(q <= (double) (kMaxDepthCandidates - 1)))   // a NaN fails both
            throw std::runtime_error("max_path_length must give between 1 and 4096 wrap candidates of the first frequency (floor(max_path_length / (300 / w_g_mhz[0])) + 1)");
        a.n_candidates = (int32_t) ((int64_t) q + 1);
    }
    a.n_passes = (float) n_passes; a.exposure_time = (float) exposure_time;
    return a;
}
// dtof_render_depth_map over the library's own float32 or float64 film: the I / Q films of dtof_depth_map_variants at their frequencies, k_depth_map
template <typename T> static void depth_map_render(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *w_g_mhz, int n_freq, double exposure_time, double max_path_length,
                                                   double *out_depth, double *out_residual, int32_t *out_wraps, double *out_amplitude, float *out_phase, float *out_tof,
                                                   dtof_render_stats *stats) {
    if (!sc || !w_g_mhz || !out_depth) throw std::runtime_error("null argument");
    check_depth_count(n_freq);
    dtof_modulation variants[2 * kMaxDepthFrequencies]; float freq[2 * kMaxDepthFrequencies];
    if (dtof_depth_map_variants(w_g_mhz, n_freq, variants, freq) != DTOF_OK) throw std::runtime_error(g_last_error);
    double f64[kMaxDepthFrequencies]; int32_t ip[kMaxDepthFrequencies], qp[kMaxDepthFrequencies];
    for (int j = 0; j < n_freq; ++j) { f64[j] = (double) w_g_mhz[j]; ip[j] = 2 * j; qp[j] = 2 * j + 1; }
    const DepthMapArgs a = depth_args(n_freq, ip, qp, f64, n_passes, exposure_time, max_path_length);
    need_doppler_for(sc, true);
    need_sensor(sc);
    ensure_device(sc);
    sc->stop = false;
    const size_t px = (size_t) sc->host.sensor.crop_w * sc->host.sensor.crop_h, nf = (size_t) n_freq;
    // the ToF images in the velocity map's buffer; its maps buffer holds depth, residual and the amplitudes (doubles), then wraps and phases (words)
    sc->d_vm_tof.ensure(px * 2 * nf); sc->d_vm_maps.ensure(px * (2 + nf) + (px * 2 * nf + 1) / 2);
    double *const d_depth = sc->d_vm_maps.p, *const d_residual = d_depth + px, *const d_amplitude = d_residual + px;
    int32_t *const d_wraps = (int32_t *) (d_amplitude + px * nf); float *const d_phase = (float *) (d_wraps + px * nf);
    const hipStream_t s = sc->stream;
    OwnFrames frames(sc);
    render_passes_into_sum<T>(sc, n_passes, spp, variants, freq, 2 * n_freq);
    launch_depth_map(sc->d_vm_sum.p, a, (int64_t) px, d_depth, out_residual ? d_residual : nullptr, out_wraps ? d_wraps : nullptr, out_amplitude ? d_amplitude : nullptr,
                     out_phase ? d_phase : nullptr, out_tof ? sc->d_vm_tof.p : nullptr, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out_depth, d_depth, px * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_residual) HIP_CHECK(hipMemcpyAsync(out_residual, d_residual, px * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_wraps) HIP_CHECK(hipMemcpyAsync(out_wraps, d_wraps, px * nf * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (out_amplitude) HIP_CHECK(hipMemcpyAsync(out_amplitude, d_amplitude, px * nf * sizeof(double), hipMemcpyDeviceToHost, s));
    if (out_phase) HIP_CHECK(hipMemcpyAsync(out_phase, d_phase, px * nf * sizeof(float), hipMemcpyDeviceToHost, s));
    if (out_tof) HIP_CHECK(hipMemcpyAsync(out_tof, sc->d_vm_tof.p, px * 2 * nf * sizeof(float), hipMemcpyDeviceToHost, s));
    frames.collect(stats);
}
extern "C" {
int dtof_depth_map_variants(const float *w_g_mhz, int n_frequencies, dtof_modulation *out_variants, float *out_w_g_mhz) {
    return guarded([&] {
        if (!w_g_mhz || !out_variants || !out_w_g_mhz) throw std::runtime_error("null argument");
        check_depth_count(n_frequencies);
        double f64[kMaxDepthFrequencies];
        for (int j = 0; j < n_frequencies; ++j) f64[j] = (double) w_g_mhz[j];
        check_depth_frequencies(f64, n_frequencies);
        for (int j = 0; j < n_frequencies; ++j) {   // two frequencies per traversal are four consecutive films: an I / Q pair never straddles two traversals
            out_variants[2 * j] = dtof_modulation { 0.f, 0.f }; out_variants[2 * j + 1] = dtof_modulation { 0.f, 0.25f };
            out_w_g_mhz[2 * j] = out_w_g_mhz[2 * j + 1] = w_g_mhz[j];
        }
    });
}
int dtof_depth_map_async(dtof_scene *sc, const float *d_rgb_sum, int n_frequencies, const int32_t *i_planes, const int32_t *q_planes, const double *w_g_mhz,
                         uint32_t n_passes, double exposure_time, double max_path_length, int64_t n_pixels,
                         double *d_depth, double *d_residual, int32_t *d_wraps, double *d_amplitude, float *d_phase) {
    return guarded([&] {
        if (!sc || !d_rgb_sum || !i_planes || !q_planes || !w_g_mhz || !d_depth) throw std::runtime_error("null argument");
        check_depth_count(n_frequencies);
        const DepthMapArgs a = depth_args(n_frequencies, i_planes, q_planes, w_g_mhz, n_passes, exposure_time, max_path_length);
        check_grid(n_pixels);
        if ((uintptr_t) d_rgb_sum % 4 != 0 || (uintptr_t) d_depth % 8 != 0 || (uintptr_t) d_residual % 8 != 0 || (uintptr_t) d_wraps % 4 != 0 ||
            (uintptr_t) d_amplitude % 8 != 0 || (uintptr_t) d_phase % 4 != 0)
            throw std::runtime_error("misaligned buffer");
        ensure_device(sc);
        launch_depth_map(d_rgb_sum, a, n_pixels, d_depth, d_residual, d_wraps, d_amplitude, d_phase, nullptr, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
int dtof_render_depth_map(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *w_g_mhz, int n_frequencies, double exposure_time, double max_path_length,
                          int film64, double *out_depth, double *out_residual, int32_t *out_wraps, double *out_amplitude, float *out_phase, float *out_tof,
                          dtof_render_stats *stats) {
    return guarded([&] {
        if (film64) depth_map_render<double>(sc, n_passes, spp, w_g_mhz, n_frequencies, exposure_time, max_path_length, out_depth, out_residual, out_wraps, out_amplitude,
                                             out_phase, out_tof, stats);
        else depth_map_render<float>(sc, n_passes, spp, w_g_mhz, n_frequencies, exposure_time, max_path_length, out_depth, out_residual, out_wraps, out_amplitude, out_phase,
                                     out_tof, stats);
    });
}
int dtof_render_velocity_map(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                             double *out_velocity, double *out_velocity_pairs, float *out_tof, dtof_render_stats *stats) {
    return guarded([&] { velocity_map_render<float>(sc, n_passes, spp, offsets, n_offsets, exposure_time, w_g_mhz, out_velocity, out_velocity_pairs, out_tof, stats); });
}

// ---------------------------------------------------------------- float64 film (dtof_film64.hip)
int dtof_render_velocity_map_f64(dtof_scene *sc, uint32_t n_passes, uint32_t spp, const float *offsets, int n_offsets, double exposure_time, double w_g_mhz,
                                 double *out_velocity, double *out_velocity_pairs, float *out_tof, dtof_render_stats *stats) {
    return guarded([&] { velocity_map_render<double>(sc, n_passes, spp, offsets, n_offsets, exposure_time, w_g_mhz, out_velocity, out_velocity_pairs, out_tof, stats); });
}
int dtof_render_rows_variants_f64(dtof_scene *sc, uint32_t seed, uint32_t spp, int32_t row_begin, int32_t row_end, const dtof_modulation *variants, int n_variants,
                                  double *d_film, int32_t planes, uint64_t plane_stride_doubles, dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || !d_film) throw std::runtime_error("null argument");
        RenderRequest rq = rows_request(seed, spp, row_begin, row_end, stats);
        set_variants(rq, variants, n_variants);
        need_doppler_for(sc, rq.n_variants > 0);
        need_sensor(sc);
        if ((uintptr_t) d_film % 8 != 0) throw std::runtime_error("the film must be 8-byte aligned");
        const HostSensor &se = sc->host.sensor;
        const int need = rq.films() + (se.alpha ? 1 : 0);   // the alpha film lies behind the colour films
        if (planes < need) throw std::runtime_error("the device film has " + std::to_string(planes) + " planes, this call writes " + std::to_string(need));
        check_plane_stride(plane_stride_doubles, (uint64_t) se.crop_w * 4, "doubles", "one film row");
        if (need > 1) check_stride_reach(se, plane_stride_doubles, row_begin, row_end, "plane stride", "doubles");
        rq.film64 = d_film; rq.film64_stride = plane_stride_doubles ? plane_stride_doubles : (uint64_t) se.crop_w * se.crop_h * 4;
        sc->stop = false;
        render_rows(sc, rq);
    });
}

// ---------------------------------------------------------------- moment film (dtof_moments.hip)
int dtof_moment_planes(int n_variants) { return n_variants < 0 || n_variants > kMaxOffsets ? -1 : moment_planes(std::max(n_variants, 1)); }
// dtof_render_moments / _aovs: n_passes frames (seeds rq.seed, + 1, ...) accumulated into the cell film, `planes` planes developed from it and copied out.  rq carries
// what the call's passes render beside that (the variants); aov: the channel table of an aov call, whose film the cells become, or null for the moment film
static void render_cells(dtof_scene *sc, RenderRequest rq, AovArgs *aov, uint32_t n_passes, int planes, int developed, double *out_planes, dtof_render_stats *stats) {
    ensure_device(sc);
    sc->stop = false;
    const HostSensor &se = sc->host.sensor;
    const size_t px = (size_t) se.crop_w * se.crop_h;
    sc->d_moments.ensure(px * kMomentCell); sc->d_moment_planes.ensure(px * planes);
    const hipStream_t s = sc->stream;
    HIP_CHECK(hipMemsetAsync(sc->d_moments.p, 0, px * kMomentCell * sizeof(double), s));   // once: the raw sums of the passes add up
    if (aov) { aov->film = sc->d_moments.p; rq.aov = aov; } else rq.moments = sc->d_moments.p;
    rq.row_begin = 0; rq.row_end = se.crop_h;
    dtof_render_stats sum, frame; memset(&sum, 0, sizeof sum);
    rq.stats = &frame;
    for (uint32_t pass = 0; pass < n_passes; ++pass, ++rq.seed) {
        render_rows(sc, rq);
        add_stats(sum, frame);
    }
    develop_cells_and_copy(sc, planes, developed, px, out_planes);
    HIP_CHECK(hipStreamSynchronize(s));
    if (stats) *stats = sum;
}
int dtof_render_moments(dtof_scene *sc, uint32_t seed, uint32_t spp, uint32_t n_passes, const dtof_modulation *variants, int n_variants, int developed,
                        double *out_planes, dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || !out_planes) throw std::runtime_error("null argument");
        if (n_passes == 0) throw std::runtime_error("the moment film needs at least one pass");
        if (n_variants < 0 || n_variants > kMaxOffsets) throw std::runtime_error("between 0 and 4 modulation variants make a moment film");
        if (n_variants > 0 && !variants) throw std::runtime_error("null argument: n_variants > 0 without variants");
        need_doppler_for(sc, n_variants > 0);
        need_sensor(sc);
        RenderRequest rq = rows_request(seed, spp, 0, 0);
        set_variants(rq, variants, n_variants);
        render_cells(sc, rq, nullptr, n_passes, moment_planes(std::max(n_variants, 1)), developed, out_planes, stats);
    });
}

// ---------------------------------------------------------------- adaptive sampling (dtof_adaptive.hip)
// every refusal of `params` (dtof.h) before a device is touched, and the kernels' argument block for K variants; the caller sets the strides of its cells
static AdaptiveArgs adaptive_args(const dtof_adaptive_params *p, int K, uint32_t spp) {
    if (!p) throw std::runtime_error("null argument");
    if (K < 1 || K > kMaxOffsets) throw std::runtime_error("dtof_adaptive: between 1 and 4 variants make a moment film");
    if (spp == 0) throw std::runtime_error("dtof_adaptive: sample count must be positive");
    if (p->tol != p->tol) throw std::runtime_error("dtof_adaptive: tol must not be NaN");
    AdaptiveArgs a; memset(&a, 0, sizeof a);
    a.mode = p->mode; a.n_variants = K; a.tol = p->tol; a.floor = p->floor; a.exposure_time = p->exposure_time; a.w_g_mhz = p->w_g_mhz; a.spp = spp;
    if (p->mode == DTOF_ADAPTIVE_IMAGE) {
        if (!(p->floor >= 0.0)) throw std::runtime_error("dtof_adaptive: floor must be >= 0 and not NaN");
    } else if (p->mode == DTOF_ADAPTIVE_VELOCITY) {
        if (p->n_pairs < 1 || p->n_pairs > kAdaptiveMaxPairs) throw std::runtime_error("dtof_adaptive: velocity mode takes 1 or 2 (homodyne, heterodyne) pairs");
        a.n_pairs = p->n_pairs;
        for (int i = 0; i < p->n_pairs; ++i) {
            const int32_t h = p->homodyne[i], t = p->heterodyne[i];
            if (h < 0 || h >= K || t < 0 || t >= K) throw std::runtime_error("dtof_adaptive: pair " + std::to_string(i) + " names a variant outside 0 .. " + std::to_string(K - 1));
            if (h == t) throw std::runtime_error("dtof_adaptive: pair " + std::to_string(i) + " needs two different variants (homodyne == heterodyne)");
            a.hom[i] = h; a.het[i] = t; a.cross[i] = adaptive_cross_plane(K, h, t);
        }
        if (!finite_positive(p->exposure_time) || !finite_positive(p->w_g_mhz))
            throw std::runtime_error("dtof_adaptive: exposure_time and w_g_mhz must be finite and > 0");
    } else throw std::runtime_error("dtof_adaptive: mode must be DTOF_ADAPTIVE_IMAGE or DTOF_ADAPTIVE_VELOCITY");
    return a;
}
// a host pixel list: strictly ascending flat indices inside the crop window
static void check_host_list(const dtof_scene *sc, const uint32_t *pixels, uint32_t n) {
    if (n && !pixels) throw std::runtime_error("null argument: n_pixels > 0 without pixels");
    const uint64_t px = (uint64_t) sc->host.sensor.crop_w * sc->host.sensor.crop_h;
    for (uint32_t i = 0; i < n; ++i) {
        if (pixels[i] >= px) throw std::runtime_error("pixel list: entry " + std::to_string(i) + " (" + std::to_string(pixels[i]) + ") lies outside the crop window of " + std::to_string(px) + " pixels");
        if (i && pixels[i] <= pixels[i - 1]) throw std::runtime_error("pixel list: entry " + std::to_string(i) + " is not above the one before it (the list must be strictly ascending)");
    }
}
static void check_variants_of_cells(const dtof_scene *sc, const dtof_modulation *variants, int n_variants) {
    if (n_variants < 0 || n_variants > kMaxOffsets) throw std::runtime_error("between 0 and 4 modulation variants make a moment film");
    if (n_variants > 0 && !variants) throw std::runtime_error("null argument: n_variants > 0 without variants");
    need_doppler_for(sc, n_variants > 0);
    need_sensor(sc);
}
// The list form's refusals for an entry that has no device buffers yet: the facts of the request it will send (pixel_list_refusal, dtof_pixel_list.h)
static void check_list_entry(const dtof_scene *sc, uint32_t spp, uint32_t n_pixels, bool moments, bool film64, bool dump = false, uint64_t dump_n = 0) {
    PixelListFacts f = pixel_list_facts(sc, spp, n_pixels);
    f.moments = moments; f.film64 = film64; f.lane_dump = dump; f.dump_n = dump_n;
    refuse_pixel_list(f);
}
// the words of sc->d_adaptive for a film of px pixels: count[px] | list[px] | the list's length (2 words) | the selection's scratch
struct AdaptiveWords { uint32_t *count, *list, *n, *scratch; };
static AdaptiveWords adaptive_words(dtof_scene *sc, size_t px) {
    sc->d_adaptive.ensure(2 * px + 2 + adaptive_scratch_words((uint32_t) px));
    uint32_t *w = sc->d_adaptive.p;
    return { w, w + px, w + 2 * px, w + 2 * px + 2 };
}
// the cells and the float64 film of a call, zeroed; planes / fplanes: moment planes, film planes (the alpha film included)
static void clear_cells_and_film(dtof_scene *sc, size_t px, bool cells, int planes, bool film, int fplanes) {
    if (cells) { sc->d_moments.ensure(px * kMomentCell); sc->d_moment_planes.ensure(px * planes); HIP_CHECK(hipMemsetAsync(sc->d_moments.p, 0, px * kMomentCell * sizeof(double), sc->stream)); }
    if (film) { sc->d_film64.ensure(px * 4 * fplanes); HIP_CHECK(hipMemsetAsync(sc->d_film64.p, 0, px * 4 * fplanes * sizeof(double), sc->stream)); }
}

int dtof_adaptive_select(const double *planes, int64_t n_pixels, int n_variants, const dtof_adaptive_params *params, uint32_t spp, uint32_t *count,
                         uint32_t *out_pixels, uint32_t *out_n, double *out_metric) {
    return guarded([&] {
        if (!planes || !count || !out_pixels || !out_n) throw std::runtime_error("null argument");
        if (n_pixels < 0 || n_pixels > (int64_t) kAdaptiveMaxPixels) throw std::runtime_error("dtof_adaptive_select: between 0 and 2^24 pixels");
        AdaptiveArgs a = adaptive_args(params, n_variants, spp);
        const size_t n = (size_t) n_pixels, P = (size_t) moment_planes(n_variants);
        a.pixel_stride = 1; a.plane_stride = (int64_t) n;
        DevBuf<double> d_planes, d_metric; DevBuf<uint32_t> d_words;   // count[n] | list[n] | length (2 words) | scratch
        d_planes.ensure(std::max<size_t>(P * n, 1)); d_metric.ensure(std::max<size_t>(out_metric ? n : 0, 1));
        d_words.ensure(2 * n + 2 + adaptive_scratch_words((uint32_t) n));
        uint32_t *d_count = d_words.p, *d_list = d_words.p + n, *d_n = d_words.p + 2 * n;
        if (n) { HIP_CHECK(hipMemcpy(d_planes.p, planes, P * n * sizeof(double), hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(d_count, count, n * 4, hipMemcpyHostToDevice)); }
        launch_adaptive_select(a, d_planes.p, (uint32_t) n, d_count, d_list, d_n, out_metric ? d_metric.p : nullptr, d_n + 2, nullptr);
        HIP_CHECK(hipGetLastError());
        uint32_t m = 0;
        HIP_CHECK(hipMemcpy(&m, d_n, 4, hipMemcpyDeviceToHost));
        if (m > n) throw HipError("dtof_adaptive_select: the device reported more selected pixels than there are");
        if (m) HIP_CHECK(hipMemcpy(out_pixels, d_list, (size_t) m * 4, hipMemcpyDeviceToHost));
        if (n) HIP_CHECK(hipMemcpy(count, d_count, n * 4, hipMemcpyDeviceToHost));
        if (n && out_metric) HIP_CHECK(hipMemcpy(out_metric, d_metric.p, n * sizeof(double), hipMemcpyDeviceToHost));
        *out_n = m;
    });
}
int dtof_render_pixels(dtof_scene *sc, uint32_t seed, uint32_t spp, const uint32_t *pixels, uint32_t n_pixels, const dtof_modulation *variants, int n_variants,
                       int developed, double *out_moments, double *out_films, dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || (!out_moments && !out_films)) throw std::runtime_error("null argument");
        check_variants_of_cells(sc, variants, n_variants);
        check_host_list(sc, pixels, n_pixels);
        dtof_render_stats frame; memset(&frame, 0, sizeof frame);
        RenderRequest rq = rows_request(seed, spp, 0, 0, &frame);
        set_variants(rq, variants, n_variants);
        check_list_entry(sc, spp, n_pixels, out_moments != nullptr, out_films != nullptr);
        ensure_device(sc);
        sc->stop = false;
        const HostSensor &se = sc->host.sensor;
        const size_t px = (size_t) se.crop_w * se.crop_h;
        const int K = rq.films(), planes = moment_planes(K), fplanes = K + (se.alpha ? 1 : 0);
        const hipStream_t s = sc->stream;
        const AdaptiveWords w = adaptive_words(sc, px);
        if (n_pixels) HIP_CHECK(hipMemcpyAsync(w.list, pixels, (size_t) n_pixels * 4, hipMemcpyHostToDevice, s));
        clear_cells_and_film(sc, px, out_moments != nullptr, planes, out_films != nullptr, fplanes);
        rq.pixels = w.list; rq.n_pixels = n_pixels;
        rq.moments = out_moments ? sc->d_moments.p : nullptr;
        if (out_films) { rq.film64 = sc->d_film64.p; rq.film64_stride = px * 4; }
        render_rows(sc, rq);
        if (out_moments) develop_cells_and_copy(sc, planes, developed, px, out_moments);
        if (out_films) HIP_CHECK(hipMemcpyAsync(out_films, sc->d_film64.p, px * 4 * fplanes * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (stats) *stats = frame;
    });
}
int dtof_render_adaptive(dtof_scene *sc, uint32_t seed, uint32_t spp, uint32_t base_passes, uint32_t max_passes, const dtof_modulation *variants, int n_variants,
                         const dtof_adaptive_params *params, int developed, double *out_moments, float *out_images, double *out_films, uint32_t *out_count,
                         double *out_metric, uint32_t *out_pass_pixels, uint32_t *out_n_passes, uint32_t *out_lists, uint64_t lists_capacity, dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || !params || !out_count || !out_pass_pixels || !out_n_passes) throw std::runtime_error("null argument");
        if (base_passes == 0) throw std::runtime_error("dtof_render_adaptive: base_passes must be at least 1 (the selection needs the moments of a dense pass)");
        if (max_passes < base_passes) throw std::runtime_error("dtof_render_adaptive: max_passes must be at least base_passes");
        check_variants_of_cells(sc, variants, n_variants);
        const uint32_t spp_each = spp ? spp : sc->pp.sample_count;
        AdaptiveArgs a = adaptive_args(params, std::max(n_variants, 1), spp_each);
        a.pixel_stride = kMomentCell; a.plane_stride = 1;
        dtof_render_stats sum, frame; memset(&sum, 0, sizeof sum);
        RenderRequest dense = rows_request(seed, spp, 0, 0, &frame);
        set_variants(dense, variants, n_variants);
        check_list_entry(sc, spp, 0, true, true);
        const HostSensor &se = sc->host.sensor;
        const size_t px = (size_t) se.crop_w * se.crop_h;
        if (px > kAdaptiveMaxPixels) throw std::runtime_error("dtof_render_adaptive: the selection handles films of up to 2^24 pixels");
        if ((uint64_t) spp_each * max_passes > 0xffffffffull) throw std::runtime_error("dtof_render_adaptive: spp * max_passes must fit 32 bits (the count map)");
        ensure_device(sc);
        sc->stop = false;
        const int K = dense.films(), planes = moment_planes(K), fplanes = K + (se.alpha ? 1 : 0);
        const hipStream_t s = sc->stream;
        const AdaptiveWords w = adaptive_words(sc, px);
        sc->d_adaptive_metric.ensure(px);
        clear_cells_and_film(sc, px, true, planes, true, fplanes);
        dense.moments = sc->d_moments.p; dense.film64 = sc->d_film64.p; dense.film64_stride = px * 4;
        for (uint32_t p = 0; p < max_passes; ++p) out_pass_pixels[p] = 0;
        uint32_t pass = 0;
        for (; pass < base_passes; ++pass) {   // the dense passes: every pixel, seeds seed + pass
            RenderRequest rq = dense; rq.seed = seed + pass; rq.row_end = se.crop_h;
            render_rows(sc, rq);
            add_stats(sum, frame);
            out_pass_pixels[pass] = (uint32_t) px;
        }
        {
            const std::vector<uint32_t> filled(px, spp_each * base_passes);
            HIP_CHECK(hipMemcpyAsync(w.count, filled.data(), px * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipStreamSynchronize(s));   // (the vector goes out of scope)
        }
        uint64_t listed = 0;
        for (; pass < max_passes; ++pass) {   // the sparse passes: select from the cells so far, read the list's length, render the list
            launch_adaptive_select(a, sc->d_moments.p, (uint32_t) px, w.count, w.list, w.n, nullptr, w.scratch, s);
            HIP_CHECK(hipGetLastError());
            uint32_t m = 0;
            HIP_CHECK(hipMemcpyAsync(&m, w.n, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            if (m > px) throw HipError("dtof_render_adaptive: the device reported more selected pixels than the film has");
            if (m == 0) break;
            if (out_lists && listed < lists_capacity)
                HIP_CHECK(hipMemcpyAsync(out_lists + listed, w.list, (size_t) std::min<uint64_t>(m, lists_capacity - listed) * 4, hipMemcpyDeviceToHost, s));
            listed += m;
            RenderRequest rq = dense; rq.seed = seed + pass; rq.pixels = w.list; rq.n_pixels = m;
            render_rows(sc, rq);   // (ends with a wait for the stream: the list may be overwritten by the next selection)
            add_stats(sum, frame);
            out_pass_pixels[pass] = m;
        }
        *out_n_passes = pass;
        if (out_metric) {
            launch_adaptive_metric(a, sc->d_moments.p, (uint32_t) px, w.count, sc->d_adaptive_metric.p, w.scratch, s);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(out_metric, sc->d_adaptive_metric.p, px * sizeof(double), hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipMemcpyAsync(out_count, w.count, px * 4, hipMemcpyDeviceToHost, s));
        if (out_moments) develop_cells_and_copy(sc, planes, developed, px, out_moments);
        if (out_images) develop_and_copy(sc, sc->d_film64.p, K, px, out_images);   // the images of dtof_render_variants_f64, from the film all passes accumulated into
        if (out_films) HIP_CHECK(hipMemcpyAsync(out_films, sc->d_film64.p, px * 4 * fplanes * sizeof(double), hipMemcpyDeviceToHost, s));
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
    need_sensor(sc);
    AovArgs a; memset(&a, 0, sizeof a);
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
        render_cells(sc, rows_request(seed, spp, 0, 0), &a, n_passes, 1 + (int) a.n_channels, developed, out_planes, stats);
    });
}
// the per-lane entries of the aov and the flow film: the channels of `a` for lanes [lane_begin, lane_begin + n)
static void sample_channel_lanes(dtof_scene *sc, AovArgs a, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out_lanes12, float *out_values) {
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
}
int dtof_sample_aov_lanes(dtof_scene *sc, uint32_t seed, uint32_t spp, const int32_t *types, int n_types, uint64_t lane_begin, uint64_t n, float *out_lanes12,
                          float *out_values) {
    return guarded([&] {
        if (!sc || !out_lanes12 || !out_values) throw std::runtime_error("null argument");
        sample_channel_lanes(sc, aov_args(sc, types, n_types), seed, spp, lane_begin, n, out_lanes12, out_values);
    });
}

// ---------------------------------------------------------------- the flow film (k_aov<LDS, FLOW = true>, dtof_aov.hip)
// the request of both entries: the aov request with the private channel table (20, 21) and S
static AovArgs flow_args(const dtof_scene *sc) {
    need_sensor(sc);
    AovArgs a; memset(&a, 0, sizeof a);
    a.n_channels = 2; a.slots[0] = (uint64_t) kAovSlots | ((uint64_t) (kAovSlots + 1) << 5u);
    a.flow = 1;
    world_to_pixel(sc->host.sensor, a.S);
    return a;
}
int dtof_render_flow(dtof_scene *sc, uint32_t seed, uint32_t spp, uint32_t n_passes, int developed, double *out_planes, dtof_render_stats *stats) {
    return guarded([&] {
        if (!sc || !out_planes) throw std::runtime_error("null argument");
        if (n_passes == 0) throw std::runtime_error("the flow film needs at least one pass");
        AovArgs a = flow_args(sc);
        render_cells(sc, rows_request(seed, spp, 0, 0), &a, n_passes, 3, developed, out_planes, stats);
    });
}
int dtof_sample_flow_lanes(dtof_scene *sc, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out_lanes12, float *out_flow2) {
    return guarded([&] {
        if (!sc || !out_lanes12 || !out_flow2) throw std::runtime_error("null argument");
        sample_channel_lanes(sc, flow_args(sc), seed, spp, lane_begin, n, out_lanes12, out_flow2);
    });
}

int dtof_develop_f64_async(dtof_scene *sc, const double *d_film64, float *d_rgb, int64_t n_pixels) {
    return guarded([&] {
        if (!sc || !d_film64 || !d_rgb) throw std::runtime_error("null argument");
        check_grid(n_pixels);
        if ((uintptr_t) d_film64 % 8 != 0 || (uintptr_t) d_rgb % 4 != 0) throw std::runtime_error("the film must be 8-byte aligned, the image 4-byte aligned");
        ensure_device(sc);
        launch_develop(d_film64, 1, 0, d_rgb, n_pixels, sc->stream);
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
        launch_develop_rgba(d_film64, d_alpha_film64, d_rgba, n_pixels, sc->stream);
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
        DevBuf<double> d_scratch; d_scratch.ensure(denoise_scratch_doubles(a));
        round_trip({ { colour, k * n * 3 * sizeof(float) }, { variance, variance ? k * n * sizeof(double) : 0 }, { normal, normal ? n * 3 * sizeof(float) : 0 }, { position, position ? n * 3 * sizeof(float) : 0 } },
                   { { out_colour, k * n * 3 * sizeof(double) }, { out_variance, out_variance ? k * n * sizeof(double) : 0 } }, [&](void *const *in, void *const *out) {
            launch_denoise(a, (const float *) in[0], (const double *) in[1], (const float *) in[2], (const float *) in[3], (double *) out[0], (double *) out[1], d_scratch.p, nullptr);
        });
    });
}

// ---------------------------------------------------------------- denoiser, temporal stage (dtof_temporal.hip)
// every refusal of the two entries (temporal_check, dtof_temporal_args.h), before a device is touched
static TemporalArgs temporal_args(const dtof_temporal_buffers *b, int n_planes, int32_t width, int32_t height, const dtof_temporal_params *p) {
    if (!b) throw std::runtime_error("dtof_denoise_temporal: null argument");
    const TemporalBuffers t { b->colour, b->variance, b->normal, b->ids, b->flow, b->h_colour, b->h_variance, b->h_normal, b->h_ids, b->h_length,
                              b->o_colour, b->o_variance, b->o_length, b->o_colour_f32 };
    TemporalArgs a;
    const std::string err = temporal_check(t, n_planes, width, height, p == nullptr, p ? p->alpha_min : 0.0, p ? p->max_length : 0.0, p ? p->tau_normal : 0.0, &a);
    if (!err.empty()) throw std::runtime_error("dtof_denoise_temporal: " + err);
    return a;
}
int dtof_denoise_temporal_async(dtof_scene *sc, const dtof_temporal_buffers *b, int n_planes, int32_t width, int32_t height, const dtof_temporal_params *params) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null argument");
        const TemporalArgs a = temporal_args(b, n_planes, width, height, params);
        ensure_device(sc);
        const TemporalDeviceBuffers d { b->colour, b->variance, b->normal, b->ids, b->flow, b->h_colour, b->h_variance, b->h_normal, b->h_ids, b->h_length,
                                        b->o_colour, b->o_variance, b->o_length, b->o_colour_f32 };
        launch_temporal(a, d, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
int dtof_denoise_temporal(const dtof_temporal_buffers *b, int n_planes, int32_t width, int32_t height, const dtof_temporal_params *params) {
    return guarded([&] {
        const TemporalArgs a = temporal_args(b, n_planes, width, height, params);
        const size_t n = (size_t) width * height, k = (size_t) n_planes;
        auto sized = [](const void *p, size_t bytes) { return HostArray { p, p ? bytes : 0 }; };
        round_trip({ sized(b->colour, k * n * 12), sized(b->variance, k * n * 8), sized(b->normal, n * 12), sized(b->ids, n * 4), sized(b->flow, n * 8),
                     sized(b->h_colour, k * n * 24), sized(b->h_variance, k * n * 8), sized(b->h_normal, n * 12), sized(b->h_ids, n * 4), sized(b->h_length, n * 4) },
                   { sized(b->o_colour, k * n * 24), sized(b->o_variance, k * n * 8), sized(b->o_length, n * 4), sized(b->o_colour_f32, k * n * 12) },
                   [&](void *const *in, void *const *out) {
            const TemporalDeviceBuffers d { (const float *) in[0], (const double *) in[1], (const float *) in[2], (const float *) in[3], (const float *) in[4],
                                            (const double *) in[5], (const double *) in[6], (const float *) in[7], (const float *) in[8], (const float *) in[9],
                                            (double *) out[0], (double *) out[1], (float *) out[2], (float *) out[3] };
            launch_temporal(a, d, nullptr);
        });
    });
}

// ---------------------------------------------------------------- denoised renders on the device (dtof_denoise_inputs.hip)
int dtof_denoise_inputs_async(dtof_scene *sc, int mode, const float *d_rgb_sum, const double *d_moment_cells, const double *d_aov_cells, int n_planes, int64_t n_pixels,
                              uint32_t n_passes, double n_samples, double exposure_time, float *d_colour, double *d_variance, float *d_normal, float *d_position,
                              uint32_t *d_extent) {
    return guarded([&] {
        if (!sc) throw std::runtime_error("null argument");
        const DenoiseInputsBuffers b { d_rgb_sum, d_moment_cells, d_aov_cells, d_colour, d_variance, d_normal, d_position, d_extent };
        DenoiseInputsArgs a;
        const std::string err = denoise_inputs_check(b, mode, n_planes, n_pixels, n_passes, n_samples, exposure_time, &a);
        if (!err.empty()) throw std::runtime_error("dtof_denoise_inputs: " + err);
        ensure_device(sc);
        if (d_extent) sc->d_denoise_extent.ensure((size_t) (kMaxDenoiseExtentBlocks + 1) * kDenoiseExtentWords);
        launch_denoise_inputs(a, d_rgb_sum, d_moment_cells, d_aov_cells, d_colour, d_variance, d_normal, d_position, sc->stream);
        if (d_extent) launch_position_extent(d_position, n_pixels, sc->d_denoise_extent.p, d_extent, sc->stream);
        HIP_CHECK(hipGetLastError());
    });
}
// What the two denoised renders are refused for before any device call (include/dtof.h lists it), beside what only the TOF entry takes
static void check_denoised_call(const dtof_scene *sc, uint32_t n_passes, const dtof_modulation *variants, int n_variants, bool doppler_only, const dtof_denoise_params *params,
                                bool sigma_auto, const dtof_denoised_outputs *out) {
    if (!sc || !params || !out || !out->denoised) throw std::runtime_error("null argument");
    if (n_passes == 0) throw std::runtime_error("n_passes must be at least 1");
    if (n_variants < 0 || n_variants > kMaxOffsets) throw std::runtime_error("between 0 and 4 modulation variants can be denoised jointly");
    if (n_variants > 0 && !variants) throw std::runtime_error("null argument: n_variants > 0 without variants");
    need_doppler_for(sc, doppler_only || n_variants > 0);
    // levels and the sigmas exactly as the denoiser's entries refuse them: denoise_check over a 1 x 1 image of every guide (an automatic sigma_position is not read)
    alignas(8) static const char dummy[6][128] = {};
    const DenoiseBuffers b { dummy[0], dummy[1], dummy[2], dummy[3], dummy[4], dummy[5] };
    DenoiseArgs a;
    const std::string err = denoise_check(b, std::max(n_variants, 1), 1, 1, false, params->levels, params->sigma_normal, sigma_auto ? 1.0 : params->sigma_position,
                                          params->sigma_luminance, &a);
    if (!err.empty()) throw std::runtime_error("dtof_denoise: " + err);
    need_sensor(sc);
    if (sc->host.sensor.crop_w > kMaxDenoiseExtent || sc->host.sensor.crop_h > kMaxDenoiseExtent) throw std::runtime_error("dtof_denoise: width and height must not exceed 65535");
}
// Both entries behind their checks.  mode: kDenoiseInputsImage | kDenoiseInputsTof; variants / n_variants: the request's (null / 0: the integrator's own pair);
// exposure_time, w_g_mhz: read in TOF mode only.  Every buffer is sized before the first launch: nothing is freed while the passes are in flight.
static void denoised_render(dtof_scene *sc, int mode, uint32_t seed, uint32_t spp, uint32_t n_passes, const dtof_modulation *variants, int n_variants, double exposure_time,
                            double w_g_mhz, const dtof_denoise_params *params, bool sigma_auto, const dtof_denoised_outputs *out, dtof_render_stats *stats) {
    const bool tof = mode == kDenoiseInputsTof;
    const int32_t types[2] = { DTOF_AOV_POSITION, DTOF_AOV_SH_NORMAL };
    AovArgs aov = aov_args(sc, types, 2);
    ensure_device(sc);
    sc->stop = false;
    const HostSensor &se = sc->host.sensor;
    const size_t px = (size_t) se.crop_w * se.crop_h, K = (size_t) std::max(n_variants, 1);
    const int alpha = se.alpha ? 1 : 0, planes = moment_planes((int) K), aov_planes = 1 + (int) aov.n_channels;
    const uint32_t spp_each = spp ? spp : sc->pp.sample_count;
    const double n_samples = (double) ((uint64_t) px * spp_each * n_passes) / (double) px;   // n_paths / n_pixels of the traversals, as the host route forms it
    int32_t hom[2] = { 0, 1 }, het[2] = { 2, 3 };
    VelocityMapArgs va; memset(&va, 0, sizeof va);
    if (tof) va = velocity_args(2, hom, het, n_passes, exposure_time, w_g_mhz);
    const DenoiseInputsArgs ia = denoise_inputs_pack(mode, (int) K, (int64_t) px, n_passes, n_samples, exposure_time);
    // the denoiser's arguments and results, the maps (doubles), then the float32 arrays
    sc->d_film64.ensure(px * 4 * (K + alpha)); sc->d_vm_sum.ensure(px * 3 * K);
    sc->d_moments.ensure(px * kMomentCell); sc->d_aov_cells.ensure(px * kMomentCell);
    if (out->moments || out->aovs) sc->d_moment_planes.ensure(px * (size_t) (planes + aov_planes));
    sc->d_denoise_io.ensure(K * px * 5 + 2 * px + (K * px * 3 + 6 * px + 1) / 2);
    sc->d_denoise_extent.ensure((size_t) (kMaxDenoiseExtentBlocks + 1) * kDenoiseExtentWords);
    double *const d_out_colour = sc->d_denoise_io.p, *const d_out_variance = d_out_colour + K * px * 3, *const d_variance = d_out_variance + K * px;
    double *const d_noisy_map = d_variance + K * px, *const d_denoised_map = d_noisy_map + px;
    float *const d_colour = (float *) (d_denoised_map + px), *const d_normal = d_colour + K * px * 3, *const d_position = d_normal + px * 3;
    uint32_t *const d_extent = sc->d_denoise_extent.p + (size_t) kMaxDenoiseExtentBlocks * kDenoiseExtentWords;
    {
        DenoiseArgs sized; memset(&sized, 0, sizeof sized);
        sized.width = se.crop_w; sized.height = se.crop_h; sized.n_planes = (int32_t) K; sized.has_variance = 1;
        sc->d_denoise.ensure(denoise_scratch_doubles(sized));
    }
    const hipStream_t s = sc->stream;
    double *const film = sc->d_film64.p;
    HIP_CHECK(hipMemsetAsync(sc->d_moments.p, 0, px * kMomentCell * sizeof(double), s));   // once: the raw sums of the passes add up
    HIP_CHECK(hipMemsetAsync(sc->d_aov_cells.p, 0, px * kMomentCell * sizeof(double), s));
    aov.film = sc->d_aov_cells.p;
    OwnFrames frames(sc);
    for (uint32_t pass = 0; pass < n_passes; ++pass) {   // one traversal per pass: the float64 film, the moment cells and the aov cells from the same lanes
        HIP_CHECK(hipMemsetAsync(film, 0, px * 4 * (K + alpha) * sizeof(double), s));
        dtof_render_stats frame;
        RenderRequest rq = rows_request(seed + pass, spp, 0, se.crop_h, &frame, true);
        rq.film64 = film; rq.film64_stride = px * 4; rq.moments = sc->d_moments.p; rq.aov = &aov;
        set_variants(rq, variants, n_variants);
        render_rows(sc, rq);
        launch_develop_accumulate(film, (int32_t) K, 0, sc->d_vm_sum.p, (int64_t) px, pass == 0, s);   // the alpha plane behind them is left out
    }
    launch_denoise_inputs(ia, sc->d_vm_sum.p, sc->d_moments.p, sc->d_aov_cells.p, d_colour, d_variance, d_normal, d_position, s);
    HIP_CHECK(hipGetLastError());
    double sigma_position = params->sigma_position;
    if (sigma_auto) {   // a copy of a few words and one wait
        launch_position_extent(d_position, (int64_t) px, sc->d_denoise_extent.p, d_extent, s);
        HIP_CHECK(hipGetLastError());
        uint32_t words[kDenoiseExtentWords];
        HIP_CHECK(hipMemcpyAsync(words, d_extent, sizeof words, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        sigma_position = denoise_sigma_position_of(words);
    }
    dtof_denoise_params used = *params;
    used.sigma_position = sigma_position;
    const DenoiseArgs da = denoise_args(d_colour, (int) K, se.crop_w, se.crop_h, d_variance, d_normal, d_position, &used, d_out_colour, d_out_variance);
    launch_denoise(da, d_colour, d_variance, d_normal, d_position, d_out_colour, d_out_variance, sc->d_denoise.p, s);
    HIP_CHECK(hipGetLastError());
    if (tof) {
        launch_velocity_map(sc->d_vm_sum.p, va, (int64_t) px, nullptr, nullptr, d_noisy_map, s);
        launch_velocity_map_planes(d_out_colour, va, (int64_t) px, d_denoised_map, s);
        HIP_CHECK(hipGetLastError());
    }
    const auto copy_out = [&](void *host, const void *dev, size_t bytes) { if (host) HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s)); };
    copy_out(out->denoised, d_out_colour, K * px * 3 * sizeof(double));
    copy_out(out->denoised_variance, d_out_variance, K * px * sizeof(double));
    copy_out(out->sum, sc->d_vm_sum.p, K * px * 3 * sizeof(float));
    copy_out(out->colour, d_colour, K * px * 3 * sizeof(float));
    copy_out(out->variance, d_variance, K * px * sizeof(double));
    copy_out(out->normal, d_normal, px * 3 * sizeof(float));
    copy_out(out->position, d_position, px * 3 * sizeof(float));
    if (tof) { copy_out(out->denoised_map, d_denoised_map, px * sizeof(double)); copy_out(out->noisy_map, d_noisy_map, px * sizeof(double)); }
    if (out->moments) {
        launch_develop_moments(sc->d_moments.p, planes, false, sc->d_moment_planes.p, (int64_t) px, s);
        copy_out(out->moments, sc->d_moment_planes.p, px * planes * sizeof(double));
    }
    if (out->aovs) {
        double *const d_planes = sc->d_moment_planes.p + px * (size_t) planes;
        launch_develop_moments(sc->d_aov_cells.p, aov_planes, false, d_planes, (int64_t) px, s);
        copy_out(out->aovs, d_planes, px * aov_planes * sizeof(double));
    }
    HIP_CHECK(hipGetLastError());
    frames.collect(stats);
    if (out->sigma_position) *out->sigma_position = sigma_position;
}
int dtof_render_denoised(dtof_scene *sc, uint32_t seed, uint32_t spp, uint32_t n_passes, const dtof_modulation *variants, int n_variants, const dtof_denoise_params *params,
                         int sigma_position_auto, const dtof_denoised_outputs *outputs, dtof_render_stats *stats) {
    return guarded([&] {
        check_denoised_call(sc, n_passes, variants, n_variants, false, params, sigma_position_auto != 0, outputs);
        denoised_render(sc, kDenoiseInputsImage, seed, spp, n_passes, variants, n_variants, 0.0, 0.0, params, sigma_position_auto != 0, outputs, stats);
    });
}
int dtof_render_velocity_map_denoised(dtof_scene *sc, uint32_t seed, uint32_t spp, uint32_t n_passes, const float offsets[2], double exposure_time, double w_g_mhz,
                                      const dtof_denoise_params *params, int sigma_position_auto, const dtof_denoised_outputs *outputs, dtof_render_stats *stats) {
    return guarded([&] {
        if (!offsets || !outputs || !outputs->denoised_map) throw std::runtime_error("null argument");
        dtof_modulation variants[4];
        if (dtof_velocity_map_variants(offsets, 2, variants) != DTOF_OK) throw std::runtime_error(g_last_error);
        check_denoised_call(sc, n_passes, variants, 4, true, params, sigma_position_auto != 0, outputs);
        check_velocity_scalars(n_passes, exposure_time, w_g_mhz);
        denoised_render(sc, kDenoiseInputsTof, seed, spp, n_passes, variants, 4, exposure_time, w_g_mhz, params, sigma_position_auto != 0, outputs, stats);
    });
}

int dtof_develop(const float *d_film, float *d_rgb, int64_t n_pixels) {
    return guarded([&] {
        if (!d_film || !d_rgb) throw std::runtime_error("null argument");
        launch_develop(d_film, 1, 0, d_rgb, n_pixels, nullptr);
        HIP_CHECK(hipGetLastError()); HIP_CHECK(hipStreamSynchronize(nullptr));
    });
}

// the lane dumps: lanes [lane_begin, lane_begin + n) of rq's render into out (12 floats each) and valid, and with out_rgb the rgb of every film of theirs
static void dump_lanes(dtof_scene *sc, RenderRequest rq, uint64_t lane_begin, uint64_t n, float *out, uint32_t *valid, float *out_rgb) {
    static_assert(sizeof(LaneDebug) == 52, "LaneDebug is 13 floats");
    sc->stop = false;
    if (n == 0) return;
    std::vector<LaneDebug> lanes(n);
    std::vector<float4> planes(out_rgb ? (size_t) rq.films() * n : 0);
    rq.lane_dump = lanes.data(); rq.dump_begin = lane_begin; rq.dump_n = n; rq.lane_planes = out_rgb ? planes.data() : nullptr;
    render_rows(sc, rq);
    for (uint64_t i = 0; i < n; ++i) { memcpy(out + 12 * i, &lanes[i], 48); if (valid) valid[i] = lanes[i].valid != 0.f ? 1u : 0u; }
    for (size_t i = 0; i < planes.size(); ++i) { out_rgb[3 * i] = planes[i].x; out_rgb[3 * i + 1] = planes[i].y; out_rgb[3 * i + 2] = planes[i].z; }
}
int dtof_sample_lanes_valid(dtof_scene *sc, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out, uint32_t *valid) {
    return guarded([&] {
        if (!sc || !out) throw std::runtime_error("null argument");
        dump_lanes(sc, rows_request(seed, spp, 0, 0), lane_begin, n, out, valid, nullptr);
    });
}
int dtof_sample_lanes_variants(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, int n_variants,
                               uint64_t lane_begin, uint64_t n, float *out, uint32_t *valid, float *out_rgb) {
    return guarded([&] {
        if (!sc || !out || !out_rgb) throw std::runtime_error("null argument");
        RenderRequest rq = rows_request(seed, spp, 0, 0);
        set_variants(rq, variants, n_variants);
        need_doppler_for(sc, rq.n_variants > 0);
        dump_lanes(sc, rq, lane_begin, n, out, valid, out_rgb);
    });
}
int dtof_sample_lanes_variants_freq(dtof_scene *sc, uint32_t seed, uint32_t spp, const dtof_modulation *variants, const float *w_g_mhz, int n_variants,
                                    uint64_t lane_begin, uint64_t n, float *out, uint32_t *valid, float *out_rgb) {
    return guarded([&] {
        if (!sc || !out || !out_rgb) throw std::runtime_error("null argument");
        RenderRequest rq = rows_request(seed, spp, 0, 0);
        set_variants_freq(rq, variants, w_g_mhz, n_variants);
        need_doppler_for(sc, rq.n_variants > 0);
        dump_lanes(sc, rq, lane_begin, n, out, valid, out_rgb);
    });
}
int dtof_sample_lanes_pixels(dtof_scene *sc, uint32_t seed, uint32_t spp, const uint32_t *pixels, uint32_t n_pixels, const dtof_modulation *variants, int n_variants,
                             float *out, uint32_t *valid, float *out_rgb) {
    return guarded([&] {
        if (!sc || !out) throw std::runtime_error("null argument");
        check_variants_of_cells(sc, variants, n_variants);
        check_host_list(sc, pixels, n_pixels);
        RenderRequest rq = rows_request(seed, spp, 0, 0);
        set_variants(rq, variants, n_variants);
        const uint64_t n = (uint64_t) n_pixels * (spp ? spp : sc->pp.sample_count);
        check_list_entry(sc, spp, n_pixels, false, false, true, n);   // the dump as dump_lanes will ask for it
        ensure_device(sc);
        const AdaptiveWords w = adaptive_words(sc, (size_t) sc->host.sensor.crop_w * sc->host.sensor.crop_h);
        if (n_pixels) HIP_CHECK(hipMemcpy(w.list, pixels, (size_t) n_pixels * 4, hipMemcpyHostToDevice));
        rq.pixels = w.list; rq.n_pixels = n_pixels;
        dump_lanes(sc, rq, 0, n, out, valid, out_rgb);
    });
}
int dtof_sample_lanes(dtof_scene *sc, uint32_t seed, uint32_t spp, uint64_t lane_begin, uint64_t n, float *out) {
    return dtof_sample_lanes_valid(sc, seed, spp, lane_begin, n, out, nullptr);
}
int dtof_develop_on_stream(const float *d_film, float *d_rgb, int64_t n_pixels, void *hip_stream) {
    return guarded([&] {
        if (!d_film || !d_rgb) throw std::runtime_error("null argument");
        launch_develop(d_film, 1, 0, d_rgb, n_pixels, (hipStream_t) hip_stream);
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

}  // extern "C"
