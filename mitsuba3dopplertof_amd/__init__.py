"""mitsuba3dopplertof_amd -- host-side mirror (ctypes over the C ABI in include/dtof.h) of the slice of
Mitsuba 3's Python interface that the Doppler-ToF hot path is driven through:

    import mitsuba3dopplertof_amd as mi
    scene = mi.load_file("scene.xml", resx=512, resy=512)            # mi.load_file (program_runner.py:142)
    integrator = mi.load_dict({'type': 'dopplertofpath', ...})      # mi.load_dict (program_runner.py:127-141)
    img = integrator.render(scene, seed=0, spp=64)                  # Integrator.render (integrator.h:74-79)

All compute happens in hand-written HIP kernels inside libdtof.so (csrc/); nothing here falls back to the
CPU: without the built library the import of any compute entry point raises, and without a GPU every
render call raises DtofError.
"""
import ctypes as C
import os

import numpy as np

__all__ = ["load_file", "load_string", "load_dict", "Scene", "Integrator", "Sampler", "DtofError", "render",
           "render_multi_pass", "to_tof_image", "lib_path", "ETimeSampling", "velocity_map_variants", "MOMENT_PLANES", "aov_channels", "AOV_TYPES", "Denoiser", "adaptive_select",
           "ADAPTIVE_MODES"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class DtofError(RuntimeError):
    pass


class ETimeSampling:   # include/mitsuba/render/sampler.h:27-34
    UNIFORM, STRATIFIED, ANTITHETIC, ANTITHETIC_MIRROR, PERIODIC, REGULAR = 0, 1, 2, 3, 4, 5


class _Stats(C.Structure):
    _fields_ = [("n_paths", C.c_uint64), ("n_bounces", C.c_uint64), ("n_shadow_rays", C.c_uint64),
                ("ms_total", C.c_double), ("ms_generate", C.c_double), ("ms_trace", C.c_double),
                ("ms_shade", C.c_double), ("ms_shadow", C.c_double), ("ms_splat", C.c_double),
                ("n_launches_trace", C.c_uint32), ("n_launches_shade", C.c_uint32), ("n_launches_shadow", C.c_uint32),
                ("n_batches", C.c_uint32), ("n_launches_first", C.c_uint32), ("ms_first", C.c_double),
                ("n_inline_iterations", C.c_uint32), ("n_bounces_inline", C.c_uint64), ("n_fused_splat_launches", C.c_uint32),
                ("n_plan_facts_launches", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class _Info(C.Structure):
    _fields_ = [("film_width", C.c_int32), ("film_height", C.c_int32), ("crop_x", C.c_int32), ("crop_y", C.c_int32),
                ("crop_width", C.c_int32), ("crop_height", C.c_int32), ("sample_count", C.c_uint32),
                ("n_shapes", C.c_uint32), ("n_groups", C.c_uint32), ("n_objects", C.c_uint32), ("n_emitters", C.c_uint32),
                ("n_triangles", C.c_uint32), ("n_bvh_nodes", C.c_uint32), ("scene_blob_bytes", C.c_uint32),
                ("time", C.c_float), ("w_g", C.c_float), ("g_1", C.c_float), ("g_0", C.c_float), ("w_s", C.c_float),
                ("phase_offset", C.c_float), ("hetero_frequency", C.c_float), ("antithetic_shift", C.c_float),
                ("wave_type", C.c_int32), ("low_frequency_component_only", C.c_int32), ("time_sampling", C.c_int32),
                ("stratify_each_interval", C.c_int32), ("path_correlation_depth", C.c_uint32), ("max_depth", C.c_uint32),
                ("rr_depth", C.c_uint32), ("base_seed", C.c_uint32), ("time_correlate_number", C.c_int32),
                ("path_correlate_number", C.c_int32), ("bvh_stack_depth", C.c_uint32),
                ("filter_radius", C.c_float), ("filter_halo", C.c_int32), ("has_alpha", C.c_int32)]


# dtof_kernels.h: kFlatShapeFields -- the presence bit, the object count (bits 19 .. 22) and the wall's index (bits 23 .. 25)
_FLAT_SHAPE_FIELDS = 1 << 18 | 0xf << 19 | 0x7 << 23
# dtof_kernels.h: kFactPairSamples -- above the shape fields: not a fact of the plan's own but work the kernel lets the two lanes of a pair share
_PAIR_SAMPLES = 1 << 26


def lib_path():
    return os.environ.get("DTOF_LIB") or os.path.join(_HERE, "libdtof.so")   # DTOF_LIB: A/B timing of two builds (tools/ab_time.sh)


def _lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    try:
        # PyTorch wheels ship their own HIP runtime (torch/lib/libamdhip64.so).  One process can host only one
        # runtime, so when torch is installed it must be the first to load it; libdtof.so then binds to the same
        # runtime by soname.  (torch is plumbing for device buffers / torch.distributed, never compute.)
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise ImportError("%s is missing -- build it with `make -C %s/csrc` (or __graft_entry__.build()); "
                          "there is no CPU fallback" % (path, _HERE))
    L = C.CDLL(path)
    cpp = C.POINTER(C.c_char_p)
    vp = C.c_void_p
    L.dtof_version.restype = C.c_char_p
    L.dtof_last_error.restype = C.c_char_p
    L.dtof_scene_load_file.argtypes = [C.c_char_p, cpp, cpp, C.c_int, C.POINTER(vp)]
    L.dtof_scene_load_string.argtypes = [C.c_char_p, cpp, cpp, C.c_int, C.POINTER(vp)]
    L.dtof_scene_destroy.argtypes = [vp]
    L.dtof_scene_destroy.restype = None
    L.dtof_scene_set_integrator.argtypes = [vp, C.c_char_p, cpp, C.c_char_p, cpp, C.c_int]
    L.dtof_scene_set_sampler.argtypes = [vp, C.c_char_p, cpp, C.c_char_p, cpp, C.c_int]
    L.dtof_integrator_create.argtypes = [C.c_char_p, cpp, C.c_char_p, cpp, C.c_int, C.POINTER(C.c_void_p)]
    L.dtof_sampler_plugin_create.argtypes = [C.c_char_p, cpp, C.c_char_p, cpp, C.c_int, C.POINTER(C.c_void_p)]
    L.dtof_integrator_destroy.argtypes = [vp]; L.dtof_integrator_destroy.restype = None
    L.dtof_sampler_plugin_destroy.argtypes = [vp]; L.dtof_sampler_plugin_destroy.restype = None
    L.dtof_integrator_render.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(_Stats)]
    L.dtof_scene_get_info.argtypes = [vp, C.POINTER(_Info)]
    L.dtof_scene_export.argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dtof_render.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(_Stats)]
    L.dtof_render_rows.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, vp, C.c_int, vp, C.POINTER(_Stats)]
    L.dtof_render_stripes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int, vp, C.POINTER(_Stats)]
    L.dtof_develop.argtypes = [vp, vp, C.c_int64]
    L.dtof_render_offsets.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_int, vp, C.POINTER(_Stats)]
    L.dtof_cancel.argtypes = [vp]
    L.dtof_cancel.restype = None
    if hasattr(L, "dtof_scene_plan_facts_launches"):   # (an older build timed through DTOF_LIB has no such entry)
        L.dtof_scene_plan_facts_launches.argtypes = [vp]
        L.dtof_scene_plan_facts_launches.restype = C.c_uint64
    if hasattr(L, "dtof_scene_last_plan_facts"):
        L.dtof_scene_last_plan_facts.argtypes = [vp]
        L.dtof_scene_last_plan_facts.restype = C.c_uint32
    if hasattr(L, "dtof_scene_last_splat"):
        L.dtof_scene_last_splat.argtypes = [vp]
        L.dtof_scene_last_splat.restype = C.c_uint32
    L.dtof_sample_lanes.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp]
    L.dtof_sample_lanes_valid.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp]
    L.dtof_develop_rgba.argtypes = [vp, vp, vp, C.c_int64]
    L.dtof_develop_on_stream.argtypes = [vp, vp, C.c_int64, vp]
    L.dtof_sampler_create.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.dtof_sampler_destroy.argtypes = [vp]
    L.dtof_sampler_destroy.restype = None
    L.dtof_sampler_seed.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.dtof_sampler_set_samples_per_wavefront.argtypes = [vp, C.c_uint32]
    L.dtof_sampler_advance.argtypes = [vp]
    L.dtof_sampler_next_1d.argtypes = [vp, vp]
    L.dtof_sampler_next_2d.argtypes = [vp, vp]
    L.dtof_sampler_next_1d_correlate.argtypes = [vp, vp, C.c_int, vp]
    L.dtof_sampler_next_2d_correlate.argtypes = [vp, vp, C.c_int, vp]
    L.dtof_sampler_next_1d_time.argtypes = [vp, C.c_int, C.c_float, C.c_int, vp]
    L.dtof_sampler_get_state.argtypes = [vp, vp]
    L.dtof_sampler_wavefront_size.argtypes = [vp]
    L.dtof_sampler_wavefront_size.restype = C.c_uint32
    L.dtof_sampler_sample_count.argtypes = [vp]
    L.dtof_sampler_sample_count.restype = C.c_uint32
    L.dtof_sampler_fork.argtypes = [vp, C.POINTER(vp)]
    L.dtof_sampler_clone.argtypes = [vp, C.POINTER(vp)]
    L.dtof_sampler_set_sample_count.argtypes = [vp, C.c_uint32]
    L.dtof_sampler_seeded.argtypes = [vp]
    L.dtof_eval_modulation.argtypes = [vp, C.c_int, vp, vp, vp, C.c_uint32]
    L.dtof_eval_component.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_uint32]
    L.dtof_render_rows_async.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, vp, C.c_int, vp]
    L.dtof_clear_async.argtypes = [vp, vp, C.c_size_t]
    L.dtof_camera_rays.argtypes = [vp, C.c_uint32, vp, vp]
    L.dtof_bsdf_eval.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp]
    L.dtof_bsdf_eval_ex.argtypes = [vp, C.c_uint32, C.c_int, C.c_uint32, vp, vp]
    L.dtof_scene_set_stream.argtypes = [vp, vp]
    L.dtof_scene_set_film_layout.argtypes = [vp, C.c_int32, C.c_uint64]
    L.dtof_render_stripes_async.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int, vp]
    L.dtof_develop_async.argtypes = [vp, vp, vp, C.c_int64]
    L.dtof_async_collect.argtypes = [vp, vp, vp, C.c_uint32, vp]
    L.dtof_ray_intersect.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.dtof_ray_intersect_uv.argtypes = [vp, C.c_uint32, vp, vp, vp, vp]
    L.dtof_ray_test.argtypes = [vp, C.c_uint32, vp, vp]
    rows, stripes = [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, vp, C.c_int, vp], [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int, vp]
    for name, args in (("dtof_render_variants", [vp, C.c_uint32, C.c_uint32, vp, C.c_int, vp, C.POINTER(_Stats)]),
                       ("dtof_render_rows_variants", rows + [C.POINTER(_Stats)]), ("dtof_render_rows_variants_async", rows),
                       ("dtof_render_stripes_variants", stripes + [C.POINTER(_Stats)]), ("dtof_render_stripes_variants_async", stripes),
                       ("dtof_sample_lanes_variants", [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp]),
                       ("dtof_emitter_eval", [vp, C.c_int, C.c_int, C.c_int32, C.c_uint32, vp, vp]),
                       ("dtof_flat_query", [vp, C.c_int, C.c_int, C.c_uint32, vp, vp, vp]),
                       ("dtof_flat_query_pairs", [vp, C.c_int, C.c_uint32, vp, vp, vp]),
                       ("dtof_tree_query", [vp, C.c_int, C.c_int, C.c_uint32, vp, vp, vp]),
                       ("dtof_pair_setup_lanes", [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp]),
                       ("dtof_develop_accumulate_async", [vp, vp, C.c_int32, C.c_uint64, vp, C.c_int64, C.c_int]),
                       ("dtof_velocity_map_async", [vp, vp, C.c_int, vp, vp, C.c_uint32, C.c_double, C.c_double, C.c_int64, vp, vp, vp]),
                       ("dtof_velocity_map_variants", [vp, C.c_int, vp]),
                       ("dtof_render_velocity_map", [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_double, C.c_double, vp, vp, vp, C.POINTER(_Stats)]),
                       ("dtof_render_velocity_map_f64", [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_double, C.c_double, vp, vp, vp, C.POINTER(_Stats)]),
                       ("dtof_render_variants_f64", [vp, C.c_uint32, C.c_uint32, vp, C.c_int, vp, vp, C.POINTER(_Stats)]),
                       ("dtof_render_rows_variants_f64", rows[:-1] + [vp, C.c_int32, C.c_uint64, C.POINTER(_Stats)]),
                       ("dtof_develop_f64_async", [vp, vp, vp, C.c_int64]), ("dtof_develop_rgba_f64_async", [vp, vp, vp, vp, C.c_int64]),
                       ("dtof_moment_planes", [C.c_int]),
                       ("dtof_render_moments", [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_int, vp, C.POINTER(_Stats)]),
                       ("dtof_aov_parse", [C.c_char_p, vp, C.c_int, C.POINTER(C.c_int), vp, C.c_size_t, C.POINTER(C.c_int)]),
                       ("dtof_scene_get_aovs", [vp, vp, C.c_size_t]),
                       ("dtof_render_aovs", [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_int, vp, C.POINTER(_Stats)]),
                       ("dtof_sample_aov_lanes", [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_uint64, C.c_uint64, vp, vp]),
                       ("dtof_denoise_async", [vp, vp, C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]),
                       ("dtof_denoise", [vp, C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]),
                       ("dtof_denoise_temporal_async", [vp, vp, C.c_int, C.c_int32, C.c_int32, vp]),
                       ("dtof_denoise_temporal", [vp, C.c_int, C.c_int32, C.c_int32, vp]),
                       ("dtof_scene_world_to_pixel", [vp, vp]),
                       ("dtof_render_flow", [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, C.POINTER(_Stats)]),
                       ("dtof_sample_flow_lanes", [vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp]),
                       ("dtof_adaptive_select", [vp, C.c_int64, C.c_int, vp, C.c_uint32, vp, vp, vp, vp]),
                       ("dtof_render_pixels", [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_int, C.c_int, vp, vp, C.POINTER(_Stats)]),
                       ("dtof_sample_lanes_pixels", [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_int, vp, vp, vp]),
                       ("dtof_render_adaptive", [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64,
                                                 C.POINTER(_Stats)])):
        if hasattr(L, name):   # a DTOF_LIB build from before the variants (A/B timing against an older commit) loads; calling what it lacks still raises
            getattr(L, name).argtypes = args
    _LIB = L
    return L


FLAT_GEOMETRY = np.array([[1, 0, 0,  0, 1, 0,  0, 0, 1,  1, 0, 0,  0, 1, 0,  0, 0, 1]], np.float32)   # dp_du, dp_dv, n, sh_s, sh_t, sh_n of dtof_bsdf_eval


def _check(rc):
    if rc != 0:
        raise DtofError(_lib().dtof_last_error().decode("utf-8", "replace"))


def _kv(params):
    names = [str(k).encode() for k in params]
    values = [str(v).encode() for v in params.values()]
    n = len(names)
    return (C.c_char_p * max(n, 1))(*names), (C.c_char_p * max(n, 1))(*values), n


def _plugin_args(d):
    """{'type': 'dopplertofpath', 'max_depth': 4, ...} -> (plugin, names, types, values, n) for the C ABI"""
    d = dict(d)
    plugin = d.pop("type", "")
    if plugin == "aov":      # likewise: a nested plugin beside its `aovs` string
        raise DtofError('the "aov" integrator wraps a nested integrator, which a property dictionary cannot carry here: declare it in the scene file '
                        '(<integrator type="aov"><string name="aovs" value="..."/><integrator type="dopplertofpath"> ... </integrator></integrator>) or set the '
                        'nested integrator itself; the channels come from Scene.render_aovs(aovs=...) either way')
    if plugin == "moment":   # its one property is a nested plugin, which these flat arrays cannot carry
        raise DtofError('the "moment" integrator wraps a nested integrator, which a property dictionary cannot carry here: declare it in the scene file '
                        '(<integrator type="moment"><integrator type="dopplertofpath"> ... </integrator></integrator>) or set the nested integrator itself; '
                        'the moments come from Scene.render_moments either way')
    names, types, values = [], [], []
    for k, v in d.items():
        names.append(str(k).encode())
        if isinstance(v, (bool, np.bool_)):
            types.append("b"); values.append(b"true" if v else b"false")
        elif isinstance(v, (int, np.integer)):
            types.append("i"); values.append(str(int(v)).encode())
        elif isinstance(v, (float, np.floating)):
            types.append("f"); values.append(repr(float(v)).encode())
        elif isinstance(v, str):
            types.append("s"); values.append(v.encode())
        else:
            raise DtofError('unsupported value type for property "%s"' % k)
    n = len(names)
    return (plugin.encode(), (C.c_char_p * max(n, 1))(*names), "".join(types).encode(), (C.c_char_p * max(n, 1))(*values), n)


class _Modulation(C.Structure):   # dtof_modulation
    _fields_ = [("hetero_frequency", C.c_float), ("hetero_offset", C.c_float)]


MAX_VARIANTS = 4   # modulation variants (films) one traversal evaluates (kMaxOffsets)


def _variant_array(variants):
    """[(hetero_frequency, hetero_offset), ...] -> (n, 2) float32 array laid out like dtof_modulation[n]"""
    v = np.ascontiguousarray(variants, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 2:
        raise DtofError("variants must be a sequence of (hetero_frequency, hetero_offset) pairs")
    return v


def _batch_args(offsets, variants):
    """The (array to keep alive, pointer, count) of a call's `offsets` or `variants` argument, and whether it is the variants form"""
    if offsets is not None and variants is not None:
        raise DtofError("pass either offsets or variants, not both")
    if variants is not None:
        v = _variant_array(variants)
        return v, v.ctypes.data, len(v), True
    if offsets is not None:
        o = np.ascontiguousarray(offsets, dtype=np.float32)
        return o, o.ctypes.data, len(o), False
    return None, None, 0, False


FILMS = ("float32", "float64")   # the film's accumulator: float32 atomics (the default), or the opt-in float64 film (dtof_film64.hip)


def _film64(film):
    """the `film=` argument of the render calls -> whether it names the float64 film; anything but the two names is refused"""
    if film not in FILMS:
        raise DtofError('film must be "float32" or "float64", not %r' % (film,))
    return film == "float64"


def MOMENT_PLANES(n_variants=1):
    """planes of the moment film of `n_variants` variants (dtof_moment_planes): 1 + 6 K + K (K - 1) / 2, 0 counting as 1; -1 outside 0 .. 4"""
    return int(_lib().dtof_moment_planes(int(n_variants)))


_MOMENT_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))   # the order of the cross planes (dtof.h), restricted to k < K


def _moment_dict(planes, k):
    """the dict of Scene.render_moments from the (P(k), H, W) planes of the C ABI"""
    h, w = planes.shape[1:]
    per = planes[1:1 + 6 * k].reshape(k, 6, h, w)
    cross = np.zeros((k, k, h, w), np.float64)
    for a in range(k):
        cross[a, a] = per[a, 4]
    slot = 1 + 6 * k
    for a, b in _MOMENT_PAIRS:
        if b < k:
            cross[a, b] = cross[b, a] = planes[slot]
            slot += 1
    return {"weight": planes[0].copy(), "mean": np.ascontiguousarray(np.moveaxis(per[:, 0:3], 1, -1)),
            "m2": np.ascontiguousarray(np.moveaxis(per[:, 3:6], 1, -1)), "cross": cross}


class _AdaptiveParams(C.Structure):   # dtof_adaptive_params
    _fields_ = [("mode", C.c_int32), ("n_pairs", C.c_int32), ("homodyne", C.c_int32 * 2), ("heterodyne", C.c_int32 * 2),
                ("tol", C.c_double), ("floor", C.c_double), ("exposure_time", C.c_double), ("w_g_mhz", C.c_double)]


ADAPTIVE_MODES = ("image", "velocity")   # DTOF_ADAPTIVE_IMAGE, DTOF_ADAPTIVE_VELOCITY


def _adaptive_params(mode, tol, floor, pairs, exposure_time, w_g):
    if mode not in ADAPTIVE_MODES:
        raise DtofError('adaptive mode must be "image" or "velocity", not %r' % (mode,))
    p = _AdaptiveParams()
    p.mode, p.tol, p.floor, p.exposure_time, p.w_g_mhz = ADAPTIVE_MODES.index(mode), float(tol), float(floor), float(exposure_time), float(w_g)
    if mode == "velocity":
        pairs = [(int(h), int(t)) for h, t in (pairs if pairs is not None else ())]
        if not 1 <= len(pairs) <= 2:
            raise DtofError("velocity mode takes 1 or 2 (homodyne, heterodyne) pairs of variant indices")
        p.n_pairs = len(pairs)
        for i, (h, t) in enumerate(pairs):
            p.homodyne[i], p.heterodyne[i] = h, t
    return p


def adaptive_select(planes, count, spp, mode="image", tol=0.0, floor=1e-3, pairs=None, exposure_time=0.0015, w_g=30):
    """The selection step of adaptive sampling over arrays (dtof_adaptive_select; include/dtof.h has the definition): `planes` (P(K), n) or (P(K), H, W) RAW moment
    sums (Scene.render_moments(raw=True) stacked in plane order, or the planes of the C ABI), `count` the samples every pixel has had.  mode "image": relative standard
    error of Y, max over the variants, against `tol` with the denominator floored at `floor`; mode "velocity": standard error of the velocity map of the (homodyne,
    heterodyne) variant index `pairs`.  Returns (ascending flat indices of the selected pixels (uint32), metric map (n,) float64, updated count (n,) uint32: + spp where
    selected)."""
    pl = np.ascontiguousarray(planes, dtype=np.float64)
    pl = pl.reshape(pl.shape[0], -1)
    k = {MOMENT_PLANES(v): v for v in (1, 2, 3, 4)}.get(pl.shape[0])
    if k is None:
        raise DtofError("adaptive_select: %d planes are not the moment planes of 1 .. 4 variants (7, 14, 22, 31)" % pl.shape[0])
    n = pl.shape[1]
    cnt = np.array(count, dtype=np.uint32).reshape(-1)
    if cnt.size != n:
        raise DtofError("adaptive_select: count must hold one entry per pixel")
    prm = _adaptive_params(mode, tol, floor, pairs, exposure_time, w_g)
    out, out_n, metric = np.zeros(max(n, 1), np.uint32), C.c_uint32(0), np.zeros(max(n, 1), np.float64)
    _check(_lib().dtof_adaptive_select(pl.ctypes.data, n, k, C.byref(prm), int(spp), cnt.ctypes.data, out.ctypes.data, C.byref(out_n), metric.ctypes.data))
    return out[:out_n.value].copy(), metric[:n], cnt


def _pixel_list(pixels):
    p = np.ascontiguousarray(pixels, dtype=np.int64).reshape(-1)
    if len(p) and (p.min() < 0 or p.max() > 0xffffffff):
        raise DtofError("pixel list: indices must be flat indices y * width + x of the crop window")
    return p.astype(np.uint32)


AOV_TYPES = ("depth", "position", "uv", "geo_normal", "sh_normal", "dp_du", "dp_dv", "prim_index", "shape_index")   # the DTOF_AOV_* constants, in their order


_AOV_CHANNELS = (1, 3, 2, 3, 3, 3, 3, 1, 1)   # channels per type


def _aov_parse(spec):
    """dtof_aov_parse -> (types int32 array, channel names)"""
    text = str(spec).encode()
    nt, nc = C.c_int(0), C.c_int(0)
    _check(_lib().dtof_aov_parse(text, None, 0, C.byref(nt), None, 0, C.byref(nc)))
    types = np.zeros(max(nt.value, 1), np.int32)
    buf = C.create_string_buffer(len(text) * 3 + 16 * max(nc.value, 1))      # a channel name is its token's name and a two-character suffix
    _check(_lib().dtof_aov_parse(text, types.ctypes.data, nt.value, C.byref(nt), buf, len(buf), C.byref(nc)))
    names = buf.raw.split(b"\0")[:nc.value]
    return types[:nt.value], [n.decode() for n in names]


def aov_channels(spec):
    """The channel names of an `aovs` string as the reference's `aov` integrator names them (dtof_aov_parse): "dd:depth,nn:sh_normal" ->
    ["dd.T", "nn.X", "nn.Y", "nn.Z"].  Raises DtofError for an unknown or unsupported type and for a token that is not <name>:<type>."""
    return _aov_parse(spec)[1]


MAX_VELOCITY_OFFSETS = 16   # offsets one velocity map combines (kMaxVelocityPairs)


def velocity_map_variants(offsets):
    """The (hetero_frequency, hetero_offset) films of a velocity map in the order they are rendered (dtof_velocity_map_variants): offsets are grouped two per
    traversal, group (o0, o1) as (0, o0), (0, o1), (1, o0), (1, o1), so a homodyne / heterodyne pair never straddles two traversals -> (2 * len(offsets), 2) float32"""
    o = np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1)
    out = np.zeros((2 * len(o), 2), np.float32)
    _check(_lib().dtof_velocity_map_variants(o.ctypes.data, len(o), out.ctypes.data))
    return out


class _DenoiseParams(C.Structure):   # dtof_denoise_params
    _fields_ = [("levels", C.c_int32), ("sigma_normal", C.c_double), ("sigma_position", C.c_double), ("sigma_luminance", C.c_double)]


class _TemporalParams(C.Structure):   # dtof_temporal_params
    _fields_ = [("alpha_min", C.c_double), ("max_length", C.c_double), ("tau_normal", C.c_double)]


class _TemporalBuffers(C.Structure):   # dtof_temporal_buffers
    _fields_ = [(name, C.c_void_p) for name in ("colour", "variance", "normal", "ids", "flow", "h_colour", "h_variance", "h_normal", "h_ids", "h_length",
                                                "o_colour", "o_variance", "o_length", "o_colour_f32")]


class Denoiser:
    """The counterpart of the reference's mi.OptixDenoiser(input_size, albedo, normals, temporal) (src/render/python/optixdenoiser_v.cpp), written in HIP
    (dtof_denoise): an edge-avoiding a-trous wavelet filter whose luminance term is normalised by the per-pixel variance, over up to four images that share ONE set
    of weights (include/dtof.h has the definition).  `input_size`: (width, height).  `normals`, `position`, `variance`: which guides every call will bring.
    `sigma_position=None`: 1 % of the largest extent of the finite positions of a call, computed with numpy and kept in `last_sigma_position`.  There is no albedo
    guide (the aov film refuses that channel) and no alpha plane.

        denoised = mi.Denoiser((w, h))(noisy)
        denoised, variance = mi.Denoiser((w, h), normals=True, position=True, variance=True)(noisy, normals=n, position=p, variance=v)

    `temporal=True` puts the temporal stage (dtof_denoise_temporal; include/dtof.h has the definition) in front of the spatial levels: every call then takes `flow`
    (H, W, 2), the pixel motion from the previous frame to this one, `ids` (H, W) if declared with `ids=True` (e.g. the aov film's shape_index plane) and `history`,
    None for a first frame or the dict the previous call returned.  The previous frame's accumulated images are reprojected through the flow, history whose id differs
    or whose normal is further than `tau_normal` away is rejected, and mean and variance are blended with weight max(1 / length, alpha_min), the length clamped to
    `max_length`; the spatial levels then filter the accumulated images, guided by the variance of the accumulated estimate.  The call returns the spatial result, its
    variance if one was brought, and the new history: the temporal result ("colour"), its "variance" and "length", and the current "normals" / "ids".  There is no
    world-space position test of the history and no 3 x 3 variance prefilter.

        den = mi.Denoiser((w, h), normals=True, variance=True, temporal=True, ids=True)
        history = None
        for frame in frames:
            denoised, variance, history = den(frame.noisy, normals=frame.n, variance=frame.v, flow=frame.flow, ids=frame.ids, history=history)"""

    def __init__(self, input_size, normals=False, position=False, variance=False, levels=5, sigma_normal=0.1, sigma_position=None, sigma_luminance=4.0,
                 temporal=False, ids=False, alpha_min=0.2, max_length=32, tau_normal=0.25):
        try:
            w, h = (int(v) for v in input_size)
        except (TypeError, ValueError):
            raise DtofError("Denoiser: input_size must be (width, height)")
        if w < 1 or h < 1:
            raise DtofError("Denoiser: input_size must be at least 1 x 1")
        if not 1 <= int(levels) <= 6:
            raise DtofError("Denoiser: levels must be between 1 and 6")
        self.input_size = (w, h)
        self.normals, self.position, self.variance = bool(normals), bool(position), bool(variance)
        self.levels = int(levels)
        self.sigma_normal, self.sigma_position, self.sigma_luminance = float(sigma_normal), None if sigma_position is None else float(sigma_position), float(sigma_luminance)
        self.last_sigma_position = None
        self.temporal, self.ids = bool(temporal), bool(ids)
        if self.ids and not self.temporal:
            raise DtofError("Denoiser: ids belong to the temporal stage (temporal=True)")
        self.alpha_min, self.max_length, self.tau_normal = float(alpha_min), float(max_length), float(tau_normal)
        if self.temporal and not (0 < self.alpha_min <= 1 and 1 <= self.max_length < float("inf") and 0 < self.tau_normal < float("inf")):
            raise DtofError("Denoiser: alpha_min must be in (0, 1], max_length finite and >= 1, tau_normal finite and > 0")

    def _guide(self, name, declared, value, shape, dtype):
        if declared != (value is not None):
            raise DtofError("Denoiser: the denoiser was created with %s=%s, so the call must %s it" % (name, declared, "bring" if declared else "not bring"))
        if value is None:
            return None
        a = np.ascontiguousarray(value, dtype=dtype)
        if a.shape != shape:
            raise DtofError("Denoiser: %s must have the shape %s, not %s" % (name, shape, a.shape))
        return a

    def _history(self, history, k, has_variance, has_normals):
        """the `history` argument of a temporal call -> its arrays in the order of dtof_temporal_buffers (None where the current frame brings no such buffer)"""
        w, h = self.input_size
        if history is None:
            return None, None, None, None, None
        if not isinstance(history, dict):
            raise DtofError("Denoiser: history must be None or the history a previous call returned")
        want = {"colour": ((k, h, w, 3), np.float64, True), "variance": ((k, h, w), np.float64, has_variance), "normals": ((h, w, 3), np.float32, has_normals),
                "ids": ((h, w), np.float32, self.ids), "length": ((h, w), np.float32, True)}
        out = []
        for name, (shape, dtype, needed) in want.items():
            if not needed:
                out.append(None)
                continue
            if history.get(name) is None:
                raise DtofError('Denoiser: the history holds no "%s"; it must come from a call with the same guides' % name)
            a = np.ascontiguousarray(history[name], dtype=dtype)
            if a.shape != shape:
                raise DtofError('Denoiser: the history\'s "%s" must have the shape %s, not %s' % (name, shape, a.shape))
            out.append(a)
        return tuple(out)

    def _accumulate(self, col, var, nrm, flow, ids, history):
        """the temporal stage over host arrays (dtof_denoise_temporal) -> (accumulated colour rounded to float32, its variance, the new history)"""
        k, h, w = col.shape[:3]
        f = self._guide("flow", True, flow, (h, w, 2), np.float32)
        idp = self._guide("ids", self.ids, ids, (h, w), np.float32)
        h_col, h_var, h_nrm, h_ids, h_len = self._history(history, k, var is not None, nrm is not None)
        o_col, o_len, o_f32 = np.zeros((k, h, w, 3), np.float64), np.zeros((h, w), np.float32), np.zeros((k, h, w, 3), np.float32)
        o_var = None if var is None else np.zeros((k, h, w), np.float64)
        arrays = (col, var, nrm, idp, f, h_col, h_var, h_nrm, h_ids, h_len, o_col, o_var, o_len, o_f32)
        buf = _TemporalBuffers(*(None if a is None else a.ctypes.data for a in arrays))
        prm = _TemporalParams(self.alpha_min, self.max_length, self.tau_normal)
        _check(_lib().dtof_denoise_temporal(C.byref(buf), k, w, h, C.byref(prm)))
        return o_f32, o_var, {"colour": o_col, "variance": o_var, "length": o_len, "normals": nrm, "ids": idp}

    def __call__(self, noisy, normals=None, position=None, variance=None, flow=None, ids=None, history=None):
        """noisy (H, W, 3) or (K, H, W, 3), K <= 4; normals, position (H, W, 3); variance (H, W) or (K, H, W): the variance of every image's luminance estimate.
        Returns the filtered images as float64 in the shape of `noisy`, and with a variance the tuple (images, filtered variance).  With temporal=True: flow (H, W, 2),
        ids (H, W) if declared, history None or the last element of the previous call's result, which gains the new history as its last element; the history's arrays
        keep the (K, ...) form whatever the shape of `noisy`."""
        w, h = self.input_size
        if not self.temporal and (flow is not None or ids is not None or history is not None):
            raise DtofError("Denoiser: flow, ids and history belong to a denoiser created with temporal=True")
        col = np.ascontiguousarray(noisy, dtype=np.float32)
        single = col.ndim == 3
        if single:
            col = col[None]
        if col.ndim != 4 or col.shape[1:] != (h, w, 3) or not 1 <= col.shape[0] <= MAX_VARIANTS:
            raise DtofError("Denoiser: noisy must be (%d, %d, 3) or (K, %d, %d, 3) with 1 <= K <= 4, not %s" % (h, w, h, w, np.shape(noisy)))
        k = col.shape[0]
        nrm = self._guide("normals", self.normals, normals, (h, w, 3), np.float32)
        pos = self._guide("position", self.position, position, (h, w, 3), np.float32)
        if variance is not None and single and np.ndim(variance) == 2:
            variance = np.asarray(variance)[None]
        var = self._guide("variance", self.variance, variance, (k, h, w), np.float64)
        sigma_x = self.sigma_position
        if pos is not None and sigma_x is None:
            finite = pos[np.isfinite(pos).all(axis=2)].astype(np.float64)
            extent = float((finite.max(axis=0) - finite.min(axis=0)).max()) if len(finite) else 0.0
            sigma_x = 0.01 * extent if extent > 0 else 1.0      # one point: every position difference is 0 whatever the sigma
            self.last_sigma_position = sigma_x
        new_history = None
        if self.temporal:      # the spatial levels below then filter the accumulated images, guided by the accumulated variance
            col, var, new_history = self._accumulate(col, var, nrm, flow, ids, history)
        prm = _DenoiseParams(self.levels, self.sigma_normal, 1.0 if sigma_x is None else sigma_x, self.sigma_luminance)
        out = np.zeros((k, h, w, 3), np.float64)
        out_var = None if var is None else np.zeros((k, h, w), np.float64)
        _check(_lib().dtof_denoise(col.ctypes.data, k, w, h, None if var is None else var.ctypes.data, None if nrm is None else nrm.ctypes.data,
                                   None if pos is None else pos.ctypes.data, C.byref(prm), out.ctypes.data, None if out_var is None else out_var.ctypes.data))
        if single:
            out, out_var = out[0], None if out_var is None else out_var[0]
        if self.temporal:
            return (out, new_history) if out_var is None else (out, out_var, new_history)
        return out if out_var is None else (out, out_var)


class Scene:
    """A loaded scene.xml (Scene + Sensor + Film + the integrator/sampler declared in it)."""

    def __init__(self, handle):
        self._h = handle
        self.last_stats = None
        self._film_layout = (0, 0)

    def __del__(self):
        try:
            if self._h:
                _lib().dtof_scene_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def info(self):
        i = _Info()
        _check(_lib().dtof_scene_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    @property
    def size(self):
        i = self.info()
        return i["crop_width"], i["crop_height"]

    def export(self, kind):
        n = C.c_size_t(0)
        _check(_lib().dtof_scene_export(self._h, kind, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(_lib().dtof_scene_export(self._h, kind, out.ctypes.data, out.size, C.byref(n)))
        return out

    def world_to_pixel(self):
        """S (3, 4) float64, world to FILM pixel (dtof_scene_world_to_pixel): pix(P) = (S[0] . (P, 1), S[1] . (P, 1)) / (S[2] . (P, 1)) in the coordinates of a
        lane's sample_pos.  Two of them make the flow of static geometry under a moving camera: harness.camera_flow."""
        out = np.zeros((3, 4), np.float64)
        _check(_lib().dtof_scene_world_to_pixel(self._h, out.ctypes.data))
        return out

    @property
    def plan_facts_launches(self):
        """first-bounce launches since the scene was loaded that ran a kernel compiled with the frame plan's constants (lane dumps included)"""
        return int(_lib().dtof_scene_plan_facts_launches(self._h))

    @property
    def last_plan_kernel(self):
        """the FACTS template argument of the first-bounce kernel compiled with the frame plan's constants that the last frame launched, 0 if it launched none:
        what dtof_scene_last_plan_facts reports, every bit of it"""
        return int(_lib().dtof_scene_last_plan_facts(self._h))

    @property
    def last_plan_mask(self):
        """the plan's constants in last_plan_kernel: the one-bit facts and, from bit 18 up, the shape fields of the flat table (dtof_kernels.h: kFactFlatShape).
        kFactPairSamples (bit 26) is not among them -- it follows from the facts below it and three inline iterations, and says how the kernel splits work between
        the lanes of a pair, not what the plan fixed: last_plan_pair_samples"""
        return self.last_plan_kernel & ~_PAIR_SAMPLES

    @property
    def last_plan_pair_samples(self):
        """did the kernel the last frame launched share the BSDF samples of a correlated pair between its two lanes (dtof_kernels.h: kFactPairSamples)?"""
        return bool(self.last_plan_kernel & _PAIR_SAMPLES)

    @property
    def last_plan_facts(self):
        """the one-bit facts of last_plan_mask (bits 0 .. 17): what callers compare with the masks of facts; the shape fields are values and come as last_plan_shape"""
        return self.last_plan_mask & ~_FLAT_SHAPE_FIELDS

    @property
    def last_plan_shape(self):
        """(objects of the flat table, index of its one wall) compiled into the kernel the last frame launched, None if that kernel has no shape"""
        m = self.last_plan_mask
        return ((m >> 19) & 0xf, (m >> 23) & 0x7) if m & (1 << 18) else None

    @property
    def last_splat(self):
        """which kernel splatted the last batch of the last frame into the float32 film, and its shape (dtof_scene_last_splat): a dict with "kernel" ("generic",
        "tent3", "x8", "pixel", "fused") and "n" (the footprint is n x n pixels), plus "seg" (tent3), "seg8" (x8) or "parts" and "chunk" (pixel); None if the frame
        splatted nothing into a float32 film, or the library (an older build timed through DTOF_LIB) has no such entry"""
        L = _lib()
        if not hasattr(L, "dtof_scene_last_splat"):
            return None
        w = int(L.dtof_scene_last_splat(self._h))
        kernel = (None, "generic", "tent3", "x8", "pixel", "fused")[w & 7]
        if kernel is None:
            return None
        out = {"kernel": kernel, "n": (w >> 3) & 15}
        if kernel == "tent3":
            out["seg"] = 1 << ((w >> 7) & 31)
        elif kernel == "x8":
            out["seg8"] = 1 << ((w >> 7) & 31)
        elif kernel == "pixel":
            out["parts"], out["chunk"] = 1 << ((w >> 7) & 31), w >> 12
        return out

    def set_integrator(self, props):
        _check(_lib().dtof_scene_set_integrator(self._h, *_plugin_args(props)))

    def set_sampler(self, props):
        _check(_lib().dtof_scene_set_sampler(self._h, *_plugin_args(props)))

    def render(self, seed=0, spp=0, offsets=None, sensor=0, variants=None, film="float32"):
        """Developed image (H, W, 3) float32 -- (H, W, 4) for an rgba film; with `offsets` (list of hetero_offset values) -> (K, H, W, 3 | 4).
        `variants`: list of (hetero_frequency, hetero_offset) pairs -> (K, H, W, 3 | 4), image k that of an integrator carrying pair k; every four of them
        share one traversal (dtof_render_variants), last_stats then sums the traversals.
        film="float64": the same images from a film accumulated and developed in double (dtof_render_variants_f64); offsets are then variants at the integrator's
        own frequency, every four of them one traversal."""
        if offsets is not None and variants is not None:
            raise DtofError("pass either offsets or variants, not both")
        if _film64(film):
            if sensor != 0:
                raise DtofError("Scene::render(): sensor index %d is out of bounds!" % sensor)
            if offsets is not None:
                f = self.info()["hetero_frequency"]
                variants = [(f, float(o)) for o in np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1)]
            images, _ = self._render_f64(seed, spp, variants, False)
            return images[0] if variants is None else images
        w, h = self.size
        st = _Stats()
        ch = 4 if self.info()["has_alpha"] else 3
        if variants is not None:
            var = _variant_array(variants)
            out = np.zeros((len(var), h, w, ch), np.float32)
            total = None
            for g in range(0, len(var), MAX_VARIANTS):
                group, part = np.ascontiguousarray(var[g:g + MAX_VARIANTS]), out[g:g + MAX_VARIANTS]
                _check(_lib().dtof_render_variants(self._h, seed, spp, group.ctypes.data, len(group), part.ctypes.data, C.byref(st)))
                d = st.as_dict()
                total = d if total is None else {k: total[k] + d[k] for k in d}
            self.last_stats = total
            return out
        if offsets is None:
            out = np.zeros((h, w, ch), np.float32)
            _check(_lib().dtof_render(self._h, sensor, seed, spp, out.ctypes.data, C.byref(st)))
        else:
            off = np.ascontiguousarray(offsets, dtype=np.float32)
            out = np.zeros((len(off), h, w, ch), np.float32)
            _check(_lib().dtof_render_offsets(self._h, seed, spp, off.ctypes.data, len(off), out.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        return out

    def _render_f64(self, seed, spp, variants, want_films):
        """(images (K, H, W, 3 | 4), films (planes, H, W, 4) float64 or None) through dtof_render_variants_f64, four variants per traversal; None: the integrator's own pair"""
        w, h = self.size
        alpha = 1 if self.info()["has_alpha"] else 0
        var = None if variants is None else _variant_array(variants)
        k = 1 if var is None else len(var)
        if want_films and k > MAX_VARIANTS:
            raise DtofError("at most 4 modulation variants can be batched per traversal")
        images = np.zeros((k, h, w, 3 + alpha), np.float32)
        films = np.zeros((k + alpha, h, w, 4), np.float64) if want_films else None
        st, total = _Stats(), None
        for g in range(0, k, MAX_VARIANTS):
            group = None if var is None else np.ascontiguousarray(var[g:g + MAX_VARIANTS])
            part = images[g:g + MAX_VARIANTS]
            _check(_lib().dtof_render_variants_f64(self._h, seed, spp, None if group is None else group.ctypes.data, 0 if group is None else len(group),
                                                   part.ctypes.data, films.ctypes.data if want_films else None, C.byref(st)))
            d = st.as_dict()
            total = d if total is None else {key: total[key] + d[key] for key in d}
        self.last_stats = total
        return images, films

    def render_film64(self, seed=0, spp=0, variants=None):
        """One traversal into the float64 film (dtof_render_variants_f64) -> (images (K, H, W, 3 | 4) float32, films (K, H, W, 4) float64 -- one more plane, the alpha
        film, behind the K colour planes of an rgba scene).  The images are the films developed in double: (float) (RGB / (W == 0 ? 1 : W)).  `variants`: up to four
        (hetero_frequency, hetero_offset) pairs; None: the integrator's own pair (K = 1)."""
        return self._render_f64(seed, spp, variants, True)

    def render_moments(self, seed=0, spp=0, n_passes=1, variants=None, raw=False):
        """The moment film of `n_passes` traversals with seeds seed, seed + 1, ... (dtof_render_moments): per pixel the filtered first and second moments of the
        samples' XYZ -- what the reference's `moment` integrator writes as AOVs -- of every variant of the traversal, and the cross moments of their Y.  Returns a dict
        of float64 arrays:
            "weight" (H, W)           sum of the filter weights
            "mean"   (K, H, W, 3)     weighted mean of X, Y, Z
            "m2"     (K, H, W, 3)     weighted mean of X^2, Y^2, Z^2
            "cross"  (K, K, H, W)     weighted mean of Y_j Y_k: symmetric, its diagonal is m2[..., 1]
        raw=True: the undivided sums under the same keys.  `variants`: up to four (hetero_frequency, hetero_offset) pairs; None: the integrator's own pair (K = 1).
        The alpha channel of an rgba film is not part of the moments.  last_stats sums the passes.  harness.moment_statistics turns the dict into variances."""
        var = None if variants is None else _variant_array(variants)
        if var is not None and not 1 <= len(var) <= MAX_VARIANTS:
            raise DtofError("between 1 and 4 modulation variants make a moment film")
        k = 1 if var is None else len(var)
        w, h = self.size
        planes = np.zeros((MOMENT_PLANES(k), h, w), np.float64)
        st = _Stats()
        _check(_lib().dtof_render_moments(self._h, int(seed), int(spp), int(n_passes), None if var is None else var.ctypes.data, 0 if var is None else k,
                                          0 if raw else 1, planes.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        per = planes[1:1 + 6 * k].reshape(k, 6, h, w)
        cross = np.zeros((k, k, h, w), np.float64)
        for a in range(k):
            cross[a, a] = per[a, 4]
        slot = 1 + 6 * k
        for a, b in _MOMENT_PAIRS:
            if b < k:
                cross[a, b] = cross[b, a] = planes[slot]
                slot += 1
        return {"weight": planes[0].copy(), "mean": np.ascontiguousarray(np.moveaxis(per[:, 0:3], 1, -1)),
                "m2": np.ascontiguousarray(np.moveaxis(per[:, 3:6], 1, -1)), "cross": cross}

    def render_denoised(self, seed=0, spp=0, n_passes=1, variants=None, **denoiser_kw):
        """The images of render(variants=...) and their jointly denoised versions (Denoiser), guided by what the moment film and the aov film provide.  THREE
        renders with the same seeds seed, seed + 1, ...: render() for the images (the float32 mean of the passes), render_moments for the variance of every
        variant's luminance estimate -- (m2_Y - mean_Y^2) / (samples per pixel x passes), harness.moment_statistics -- and render_aovs("p:position,n:sh_normal") for
        the guides; then ONE Denoiser call over all variants, which therefore share their weights.  That these are three traversals of the scene is accepted for
        now: fusing them on the device is a later step.  `variants`: up to four (hetero_frequency, hetero_offset) pairs; None: the integrator's own pair.
        `denoiser_kw`: levels and the sigmas of Denoiser.  Returns a dict: "image" (K, H, W, 3 | 4) float32 -- (H, W, 3 | 4) without variants --, "denoised"
        float64 (the first three channels: an alpha plane is not denoised), "variance" and "denoised_variance" (K, H, W) -- (H, W) -- float64, and "denoiser"."""
        from .harness import moment_statistics
        if variants is not None and not 1 <= len(variants) <= MAX_VARIANTS:
            raise DtofError("between 1 and 4 modulation variants can be denoised jointly")
        n_passes = int(n_passes)
        if n_passes < 1:
            raise DtofError("n_passes must be at least 1")
        image = self.render(seed=seed, spp=spp, variants=variants)
        for i in range(1, n_passes):
            image = image + self.render(seed=seed + i, spp=spp, variants=variants)
        if n_passes > 1:
            image = image / np.float32(n_passes)
        stats = self.last_stats
        m = self.render_moments(seed=seed, spp=spp, n_passes=n_passes, variants=variants)
        per_pixel = self.last_stats["n_paths"] / float(self.size[0] * self.size[1])        # samples per pixel x passes, as rendered
        variance = moment_statistics(m, per_pixel)["variance"][..., 1] / per_pixel
        guides = self.render_aovs("p:position,n:sh_normal", seed=seed, spp=spp, n_passes=n_passes)
        self.last_stats = stats
        den = Denoiser(self.size, normals=True, position=True, variance=True, **denoiser_kw)
        noisy = image[..., :3]
        if variants is None:
            variance = variance[0]
        denoised, denoised_variance = den(noisy, normals=guides["n"], position=guides["p"], variance=variance)
        return {"image": image, "denoised": denoised, "variance": variance, "denoised_variance": denoised_variance, "denoiser": den}

    @property
    def aovs(self):
        """the `aovs` string of a scene whose integrator is <integrator type="aov"> (dtof_scene_get_aovs), None for every other scene"""
        buf = C.create_string_buffer(1 << 16)
        _check(_lib().dtof_scene_get_aovs(self._h, buf, len(buf)))
        return buf.value.decode() or None

    def render_aovs(self, aovs=None, seed=0, spp=0, n_passes=1, raw=False):
        """The geometry channels of the reference's `aov` integrator along the scene integrator's own camera rays (dtof_render_aovs), accumulated in double over
        `n_passes` passes with seeds seed, seed + 1, ...  `aovs`: the reference's spec, "name:type,name:type" with the types of AOV_TYPES; None: the spec of the scene
        file's <integrator type="aov">.  Returns a dict of float64 arrays: "weight" (H, W), the sum of the filter weights; per name (H, W) for a one-channel type and
        (H, W, n) for the others, the weighted means (raw=True: the undivided sums); and "channels", the list of channel names in film order.  Every value is 0 where
        the camera ray leaves the scene.  last_stats sums the passes."""
        spec = self.aovs if aovs is None else aovs
        if spec is None:
            raise DtofError("render_aovs: the scene's integrator is no \"aov\" integrator, so the `aovs` spec must be given")
        types, names = _aov_parse(spec)
        w, h = self.size
        planes = np.zeros((1 + len(names), h, w), np.float64)
        st = _Stats()
        _check(_lib().dtof_render_aovs(self._h, int(seed), int(spp), int(n_passes), types.ctypes.data, len(types), 0 if raw else 1, planes.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        out = {"weight": planes[0].copy(), "channels": names}
        c = 1
        for t in types:      # the channels of one token follow each other: name.X, name.Y, name.Z
            n, name = _AOV_CHANNELS[t], names[c - 1].rsplit(".", 1)[0]
            if name in out:
                raise DtofError("render_aovs: the name \"%s\" occurs twice in the spec or is a key of the result; dtof_render_aovs returns such a film as planes" % name)
            out[name] = planes[c].copy() if n == 1 else np.ascontiguousarray(np.moveaxis(planes[c:c + n], 0, -1))
            c += n
        return out

    def sample_aov_lanes(self, aovs, seed, spp, lane_begin, n):
        """sample_lanes of an aov render (dtof_sample_aov_lanes): the dict of sample_lanes without `valid`, plus "values" (n, C) float32, the channels of every lane in
        the order of aov_channels(aovs), and "channels"."""
        types, names = _aov_parse(aovs)
        out, values = np.zeros((n, 12), np.float32), np.zeros((n, len(names)), np.float32)
        _check(_lib().dtof_sample_aov_lanes(self._h, seed, spp, types.ctypes.data, len(types), lane_begin, n, out.ctypes.data, values.ctypes.data))
        return {"sample_pos": out[:, 0:2], "time": out[:, 2], "ray_o": out[:, 3:6], "ray_d": out[:, 6:9], "rgb": out[:, 9:12], "values": values, "channels": names}

    def render_flow(self, seed=0, spp=0, n_passes=1, raw=False, weight=False):
        """The flow film (dtof_render_flow; include/dtof.h has the definition): the screen-space motion, in pixels over ONE shutter interval, of what the scene
        integrator's own camera rays hit, from the keyframes of the hit objects' <animation>; accumulated in double over `n_passes` passes with seeds seed,
        seed + 1, ... like render_aovs.  Returns (H, W, 2) float64, the weighted mean (raw=True: the undivided sums); weight=True: the tuple (flow, weight (H, W)).
        +0 where the rays leave the scene or meet static objects; NaN where a hit is not in front of the camera at both ends of the shutter.  It is what
        Denoiser(temporal=True) takes as `flow` when the frame interval is the exposure; scale it otherwise."""
        w, h = self.size
        planes = np.zeros((3, h, w), np.float64)
        st = _Stats()
        _check(_lib().dtof_render_flow(self._h, int(seed), int(spp), int(n_passes), 0 if raw else 1, planes.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        flow = np.ascontiguousarray(np.moveaxis(planes[1:3], 0, -1))
        return (flow, planes[0].copy()) if weight else flow

    def sample_flow_lanes(self, seed, spp, lane_begin, n):
        """sample_lanes of a flow render (dtof_sample_flow_lanes): the dict of sample_lanes without `valid`, plus "flow" (n, 2) float32"""
        out, flow = np.zeros((n, 12), np.float32), np.zeros((n, 2), np.float32)
        _check(_lib().dtof_sample_flow_lanes(self._h, seed, spp, lane_begin, n, out.ctypes.data, flow.ctypes.data))
        return {"sample_pos": out[:, 0:2], "time": out[:, 2], "ray_o": out[:, 3:6], "ray_d": out[:, 6:9], "rgb": out[:, 9:12], "flow": flow}

    def set_film_layout(self, planes, plane_stride_floats=0):
        """Declare the caller's device film for render_rows / render_stripes (dtof_scene_set_film_layout): `planes` RGBW planes, `plane_stride_floats` apart (0 = dense
        H * W * 4).  An rgba scene needs n_offsets + 1 planes -- the alpha film lies behind the colour films -- and is refused until they are declared.  With more
        than one plane, a stride too small for the rows a call writes (its rows plus the filter's halo) is refused by that call."""
        _check(_lib().dtof_scene_set_film_layout(self._h, int(planes), int(plane_stride_floats)))
        self._film_layout = (int(planes), int(plane_stride_floats))

    @property
    def film_layout(self):
        """(planes, plane_stride_floats) as last declared with set_film_layout; (0, 0) = nothing declared.  A helper that declares a layout of its own
        (distributed.render_sharded / render_striped) puts this one back."""
        return getattr(self, "_film_layout", (0, 0))

    def film_planes(self, n_offsets=1):
        """RGBW planes the device-film calls write for `n_offsets` batched offsets: one more for the alpha film of an rgba scene"""
        return max(int(n_offsets), 1) + (1 if self.info()["has_alpha"] else 0)

    def render_rows(self, d_film_ptr, seed, spp, row_begin, row_end, offsets=None, variants=None):
        """Accumulate the undeveloped RGBW film of rows [row_begin,row_end) into a DEVICE buffer (int pointer) of film_planes() planes (set_film_layout for rgba scenes).
        `variants`: up to four (hetero_frequency, hetero_offset) pairs instead of `offsets`, plane k = pair k (dtof_render_rows_variants)."""
        st = _Stats()
        keep, ptr, n, is_var = _batch_args(offsets, variants)
        fn = _lib().dtof_render_rows_variants if is_var else _lib().dtof_render_rows
        _check(fn(self._h, seed, spp, row_begin, row_end, ptr, n, d_film_ptr, C.byref(st)))
        self.last_stats = st.as_dict()
        return self.last_stats

    def render_rows_f64(self, d_film_ptr, seed, spp, row_begin, row_end, variants=None, planes=None, plane_stride_doubles=0):
        """render_rows into a float64 DEVICE film (dtof_render_rows_variants_f64): `planes` RGBW planes of doubles (default: film_planes() of the call), `plane_stride_doubles`
        apart (0 = dense H * W * 4).  The layout belongs to the call: set_film_layout is neither read nor changed."""
        st = _Stats()
        keep, ptr, n, _ = _batch_args(None, variants)
        planes = self.film_planes(n) if planes is None else int(planes)
        _check(_lib().dtof_render_rows_variants_f64(self._h, seed, spp, row_begin, row_end, ptr, n, d_film_ptr, planes, int(plane_stride_doubles), C.byref(st)))
        self.last_stats = st.as_dict()
        return self.last_stats

    def develop_f64_async(self, d_film_ptr, d_rgb_ptr, n_pixels, d_alpha_film_ptr=None):
        """enqueue the develop of one float64 film plane (dtof_develop_f64_async); with the alpha plane of an rgba film: rgba (dtof_develop_rgba_f64_async)"""
        if d_alpha_film_ptr is None:
            _check(_lib().dtof_develop_f64_async(self._h, d_film_ptr, d_rgb_ptr, n_pixels))
        else:
            _check(_lib().dtof_develop_rgba_f64_async(self._h, d_film_ptr, d_alpha_film_ptr, d_rgb_ptr, n_pixels))

    def render_rows_async(self, d_film_ptr, seed, spp, row_begin, row_end, offsets=None, variants=None):
        """enqueue one frame on the scene's stream without waiting for it (dtof_render_rows_async / _variants_async); collect() waits and returns the timings"""
        keep, ptr, n, is_var = _batch_args(offsets, variants)
        fn = _lib().dtof_render_rows_variants_async if is_var else _lib().dtof_render_rows_async
        _check(fn(self._h, seed, spp, row_begin, row_end, ptr, n, d_film_ptr))

    def clear_async(self, d_ptr, nbytes):
        _check(_lib().dtof_clear_async(self._h, d_ptr, nbytes))

    def set_stream(self, stream_ptr):
        """enqueue on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream); 0 / None: back to the scene's own (dtof_scene_set_stream)"""
        _check(_lib().dtof_scene_set_stream(self._h, C.c_void_p(stream_ptr or None)))

    def render_stripes_async(self, d_film_ptr, seed, spp, first_row, stripe_rows, stripe_period, offsets=None, variants=None):
        keep, ptr, n, is_var = _batch_args(offsets, variants)
        fn = _lib().dtof_render_stripes_variants_async if is_var else _lib().dtof_render_stripes_async
        _check(fn(self._h, seed, spp, first_row, stripe_rows, stripe_period, ptr, n, d_film_ptr))

    def develop_async(self, d_film_ptr, d_rgb_ptr, n_pixels):
        _check(_lib().dtof_develop_async(self._h, d_film_ptr, d_rgb_ptr, n_pixels))

    def develop_accumulate_async(self, d_film_ptr, planes, d_rgb_sum_ptr, n_pixels, first, plane_stride_floats=0):
        """enqueue rgb / W of `planes` RGBW film planes into (first) or onto the dense float32 sum [planes][n_pixels][3] of a multi-pass render (dtof_develop_accumulate_async)"""
        _check(_lib().dtof_develop_accumulate_async(self._h, d_film_ptr, int(planes), int(plane_stride_floats), d_rgb_sum_ptr, int(n_pixels), int(bool(first))))

    def velocity_map_async(self, d_rgb_sum_ptr, homodyne_planes, heterodyne_planes, n_passes, n_pixels, d_velocity_ptr, exposure_time=0.0015, w_g=30,
                           d_tof_ptr=None, d_velocity_pairs_ptr=None):
        """enqueue the velocity map of the sum of `n_passes` passes (dtof_velocity_map_async): pair k is planes (homodyne_planes[k], heterodyne_planes[k]) of the 2 * n_pairs
        planes of the sum; d_velocity [n_pixels] float64, optionally d_velocity_pairs [n_pairs][n_pixels] float64 and d_tof [2 * n_pairs][n_pixels] float32"""
        hom, het = np.ascontiguousarray(homodyne_planes, dtype=np.int32).reshape(-1), np.ascontiguousarray(heterodyne_planes, dtype=np.int32).reshape(-1)
        if len(hom) != len(het):
            raise DtofError("as many homodyne as heterodyne planes make the pairs")
        _check(_lib().dtof_velocity_map_async(self._h, d_rgb_sum_ptr, len(hom), hom.ctypes.data, het.ctypes.data, int(n_passes), float(exposure_time), float(w_g),
                                              int(n_pixels), d_tof_ptr, d_velocity_pairs_ptr, d_velocity_ptr))

    def render_velocity_map(self, n_passes, spp, offsets=(0.0, 0.25), exposure_time=0.0015, w_g=30, pairs=False, film="float32"):
        """The radial-velocity map of `n_passes` passes (seeds 0 .. n_passes - 1) of `spp` samples, reconstructed on the device (dtof_render_velocity_map): every two
        offsets share one traversal per pass, their films never leave the GPU.  Returns (velocity (H, W) float64, {"homodyne": [...], "heterodyne": [...]} float32 ToF
        images in the order of `offsets`) and, with pairs=True, the maps of every offset alone (len(offsets), H, W) float64 -- the values numpy computes from the same
        films with harness.calc_velocity_from_homo_heteros / _hetero.  last_stats sums the traversals.  film="float64": every pass is splatted and developed in double
        (dtof_render_velocity_map_f64) -- the films numpy has to be given are then those of render(..., film="float64")."""
        entry = _lib().dtof_render_velocity_map_f64 if _film64(film) else _lib().dtof_render_velocity_map
        off = np.ascontiguousarray([float(o) for o in offsets], dtype=np.float32)
        n = len(off)
        w, h = self.size
        st = _Stats()
        v, tof = np.zeros((h, w), np.float64), np.zeros((2 * n, h, w), np.float32)
        per_pair = np.zeros((n, h, w), np.float64) if pairs else None
        _check(entry(self._h, int(n_passes), int(spp), off.ctypes.data, n, float(exposure_time), float(w_g), v.ctypes.data,
                     per_pair.ctypes.data if pairs else None, tof.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        homo, hetero = [], []
        for g in range(0, n, 2):   # the planes of a group: its homodyne films, then its heterodyne films (velocity_map_variants)
            k = min(2, n - g)
            homo += [tof[2 * g + j] for j in range(k)]
            hetero += [tof[2 * g + k + j] for j in range(k)]
        films = {"homodyne": homo, "heterodyne": hetero}
        return (v, films, per_pair) if pairs else (v, films)

    def collect(self, max_frames=4096):
        """wait for the frames enqueued by render_rows_async -> (summed stats dict, per-frame GPU milliseconds)"""
        st, ms, n = _Stats(), np.zeros(max_frames, np.float64), C.c_uint32(0)
        _check(_lib().dtof_async_collect(self._h, C.byref(st), ms.ctypes.data, max_frames, C.byref(n)))
        return st.as_dict(), ms[:min(n.value, max_frames)].copy()

    def render_stripes(self, d_film_ptr, seed, spp, first_row, stripe_rows, stripe_period, offsets=None, variants=None):
        """Accumulate the rows of the stripes [first_row + k * stripe_period, ... + stripe_rows) (interleaved shard of one rank)."""
        st = _Stats()
        keep, ptr, n, is_var = _batch_args(offsets, variants)
        fn = _lib().dtof_render_stripes_variants if is_var else _lib().dtof_render_stripes
        _check(fn(self._h, seed, spp, first_row, stripe_rows, stripe_period, ptr, n, d_film_ptr, C.byref(st)))
        self.last_stats = st.as_dict()
        return self.last_stats

    def sample_lanes(self, seed, spp, lane_begin, n):
        out = np.zeros((n, 12), np.float32)
        valid = np.zeros(n, np.uint32)
        _check(_lib().dtof_sample_lanes_valid(self._h, seed, spp, lane_begin, n, out.ctypes.data, valid.ctypes.data))
        return {"sample_pos": out[:, 0:2], "time": out[:, 2], "ray_o": out[:, 3:6], "ray_d": out[:, 6:9], "rgb": out[:, 9:12], "valid": valid}

    def sample_lanes_variants(self, seed, spp, lane_begin, n, variants=None):
        """sample_lanes through the batched kernels (dtof_sample_lanes_variants): the lanes are evaluated once for up to four (hetero_frequency, hetero_offset)
        pairs; `rgb` is (K, n, 3), plane k the lanes' results with pair k, everything else is shared by the variants.  None: the integrator's own pair (K = 1)."""
        var = None if variants is None else _variant_array(variants)
        k = 1 if var is None or len(var) == 0 else len(var)
        out, valid, rgb = np.zeros((n, 12), np.float32), np.zeros(n, np.uint32), np.zeros((k, n, 3), np.float32)
        _check(_lib().dtof_sample_lanes_variants(self._h, seed, spp, None if var is None else var.ctypes.data, 0 if var is None else len(var),
                                                 lane_begin, n, out.ctypes.data, valid.ctypes.data, rgb.ctypes.data))
        return {"sample_pos": out[:, 0:2], "time": out[:, 2], "ray_o": out[:, 3:6], "ray_d": out[:, 6:9], "rgb": rgb, "valid": valid}

    def _cell_variants(self, variants):
        var = None if variants is None else _variant_array(variants)
        if var is not None and not 1 <= len(var) <= MAX_VARIANTS:
            raise DtofError("between 1 and 4 modulation variants make a moment film")
        return var, 1 if var is None else len(var)

    def sample_lanes_pixels(self, seed, spp, pixels, variants=None):
        """sample_lanes_variants of every lane of the listed pixels (dtof_sample_lanes_pixels): `pixels` strictly ascending flat indices y * width + x; record
        i * spp + j is global lane pixels[i] * spp + j of the dense render with this seed.  Same dict; `rgb` is (K, n, 3)."""
        var, k = self._cell_variants(variants)
        pix = _pixel_list(pixels)
        n = len(pix) * (int(spp) if spp else self.info()["sample_count"])
        out, valid, rgb = np.zeros((max(n, 1), 12), np.float32), np.zeros(max(n, 1), np.uint32), np.zeros((k, max(n, 1), 3), np.float32)
        if n == 0:
            rgb = np.zeros((k, 0, 3), np.float32)
        _check(_lib().dtof_sample_lanes_pixels(self._h, int(seed), int(spp), pix.ctypes.data if len(pix) else None, len(pix), None if var is None else var.ctypes.data,
                                               0 if var is None else k, out.ctypes.data, valid.ctypes.data, rgb.ctypes.data))
        out, valid = out[:n], valid[:n]
        return {"sample_pos": out[:, 0:2], "time": out[:, 2], "ray_o": out[:, 3:6], "ray_d": out[:, 6:9], "rgb": rgb, "valid": valid}

    def render_pixels(self, pixels, seed=0, spp=0, variants=None, raw=False, films=False, moments=True):
        """ONE traversal of the listed pixels only (dtof_render_pixels) -- region-of-interest rendering: the lanes of a listed pixel are those of the dense render with
        this seed, so the full list gives the dense films.  Returns the dict of render_moments (raw=True: the undivided sums); with films=True also "film64"
        (K, H, W, 4) float64 raw R, G, B, W sums (one more plane, the alpha film, for an rgba scene); moments=False: the float64 film alone.  Pixels outside every
        listed footprint are 0."""
        var, k = self._cell_variants(variants)
        pix = _pixel_list(pixels)
        w, h = self.size
        alpha = 1 if self.info()["has_alpha"] else 0
        planes = np.zeros((MOMENT_PLANES(k), h, w), np.float64) if moments else None
        film = np.zeros((k + alpha, h, w, 4), np.float64) if films else None
        st = _Stats()
        _check(_lib().dtof_render_pixels(self._h, int(seed), int(spp), pix.ctypes.data if len(pix) else None, len(pix), None if var is None else var.ctypes.data,
                                         0 if var is None else k, 0 if raw else 1, None if planes is None else planes.ctypes.data,
                                         None if film is None else film.ctypes.data, C.byref(st)))
        self.last_stats = st.as_dict()
        out = _moment_dict(planes, k) if moments else {}
        if films:
            out["film64"] = film
        return out

    def render_adaptive(self, seed=0, spp=0, base_passes=1, max_passes=4, variants=None, mode="image", tol=0.05, floor=1e-3, pairs=None, exposure_time=0.0015, w_g=30,
                        raw=False, films=False, lists=False):
        """Adaptive sampling (dtof_render_adaptive; include/dtof.h has the definition): `base_passes` dense passes with seeds seed, seed + 1, ..., then up to
        max_passes - base_passes passes that render only the pixels whose estimated error is still above `tol` -- mode "image": the relative standard error of Y,
        the largest over the variants; mode "velocity": the standard error (m/s) of the velocity map of the (homodyne, heterodyne) variant index `pairs`.  All passes
        accumulate into one moment film and one float64 film.  Returns a dict: the keys of render_moments (raw=True: undivided sums), "images" (K, H, W, 3 | 4)
        float32 developed from the float64 film, "count" (H, W) uint32 samples rendered in every pixel, "metric" (H, W) float64 of the final state,
        "pass_pixels" (pixels every pass that ran rendered); films=True: "film64"; lists=True: "lists", the pixel list of every sparse pass.
        Selecting by an estimated variance biases the estimator slightly: pixels that look converged by chance stop early; base_passes and spp bound that.  With a
        filter wider than the box, count is the nominal sample count (harness.moment_statistics)."""
        var, k = self._cell_variants(variants)
        prm = _adaptive_params(mode, tol, floor, pairs, exposure_time, w_g)
        base_passes, max_passes = int(base_passes), int(max_passes)
        if base_passes < 1 or max_passes < base_passes:
            raise DtofError("render_adaptive: base_passes must be at least 1 and max_passes at least base_passes")
        w, h = self.size
        alpha = 1 if self.info()["has_alpha"] else 0
        planes = np.zeros((MOMENT_PLANES(k), h, w), np.float64)
        images = np.zeros((k, h, w, 3 + alpha), np.float32)
        film = np.zeros((k + alpha, h, w, 4), np.float64) if films else None
        count, metric = np.zeros((h, w), np.uint32), np.zeros((h, w), np.float64)
        pass_pixels, n_passes = np.zeros(max_passes, np.uint32), C.c_uint32(0)
        cap = (max_passes - base_passes) * w * h if lists else 0
        flat = np.zeros(max(cap, 1), np.uint32)
        st = _Stats()
        _check(_lib().dtof_render_adaptive(self._h, int(seed), int(spp), base_passes, max_passes, None if var is None else var.ctypes.data, 0 if var is None else k,
                                           C.byref(prm), 0 if raw else 1, planes.ctypes.data, images.ctypes.data, None if film is None else film.ctypes.data,
                                           count.ctypes.data, metric.ctypes.data, pass_pixels.ctypes.data, C.byref(n_passes), flat.ctypes.data if lists else None, cap,
                                           C.byref(st)))
        self.last_stats = st.as_dict()
        out = _moment_dict(planes, k)
        out.update(images=images, count=count, metric=metric, pass_pixels=pass_pixels[:n_passes.value].copy())
        if films:
            out["film64"] = film
        if lists:
            ends = np.cumsum(pass_pixels[base_passes:n_passes.value].astype(np.int64))
            out["lists"] = [flat[e - m:e].copy() for e, m in zip(ends, pass_pixels[base_passes:n_passes.value])]
        return out

    def bsdf_eval(self, shape_index, queries, spec=-1, geometry=None):
        """BSDF::eval_pdf_sample of shape `shape_index` over an (n, 11) array of (wi, wo, sample1, sample2, uv) -> (n, 14): value[3], pdf, wo[3], pdf, eta, delta,
        weight[3], null.  `geometry`: (n, 18) or (18,) dp_du, dp_dv, n, sh_s, sh_t, sh_n (default: the flat frame); queries may also be (n, 29) with the geometry
        appended.  `spec`: the instantiation of the shade kernels' BSDF function (0, 1, 2; -1 = the one a render of this scene runs)."""
        q = np.ascontiguousarray(queries, np.float32)
        q = q.reshape(-1, 29 if geometry is None and q.ndim == 2 and q.shape[1] == 29 else 11)
        if q.shape[1] == 11:
            g = FLAT_GEOMETRY if geometry is None else np.asarray(geometry, np.float32).reshape(-1, 18)
            q = np.ascontiguousarray(np.concatenate([q, np.broadcast_to(g, (len(q), 18))], axis=1))
        out = np.zeros((len(q), 14), np.float32)
        _check(_lib().dtof_bsdf_eval_ex(self._h, shape_index, spec, len(q), q.ctypes.data, out.ctypes.data))
        return out

    def emitter_eval(self, mode, queries, level=-1, shape_index=-1):
        """The emitter side of a path vertex over arrays, through the shade kernels' own device functions (dtof_emitter_eval).  mode 0: (n, 5) reference point and the
        draws e1, e2 -> (n, 14) sampled point[3], direction[3], distance, density, delta, weight[3], usable, picked emitter; mode 1: (n, 11) previous vertex, hit point,
        shading normal, uv on shape `shape_index` -> (n, 5) distance, direction[3], density; mode 2: (n, 3) directions -> (n, 4) density and value of the environment.
        `level`: the (AREA, MESH, SPEC) instantiation (0 .. 6; -1 = the one a render of this scene runs).  Floats that are not finite and draws outside [0, 1) are refused."""
        n_in, n_out = {0: (5, 14), 1: (11, 5), 2: (3, 4)}[mode]
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, n_in)
        out = np.zeros((len(q), n_out), np.float32)
        _check(_lib().dtof_emitter_eval(self._h, mode, level, shape_index, len(q), q.ctypes.data, out.ctypes.data))
        return out

    def camera_rays(self, samples):
        """Sensor::sample_ray over an (n, 4) array of (position sample x, y in [0, 1]^2 of the crop window, aperture sample x, y) -> (origins, directions, maxt)"""
        s = np.ascontiguousarray(samples, np.float32).reshape(-1, 4)
        out = np.zeros((len(s), 7), np.float32)
        _check(_lib().dtof_camera_rays(self._h, len(s), s.ctypes.data, out.ctypes.data))
        return out[:, 0:3], out[:, 3:6], out[:, 6]

    def eval_modulation(self, mode, t, length=None):
        t = np.ascontiguousarray(t, np.float32)
        ln = np.ascontiguousarray(length, np.float32) if length is not None else None
        out = np.zeros_like(t)
        _check(_lib().dtof_eval_modulation(self._h, mode, t.ctypes.data, ln.ctypes.data if ln is not None else None,
                                           out.ctypes.data, t.size))
        return out

    @staticmethod
    def _rays(o, d, time, maxt):
        o, d = np.atleast_2d(np.asarray(o, np.float32)), np.atleast_2d(np.asarray(d, np.float32))
        n = max(len(o), len(d))
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, time
        rays[:, 7] = np.finfo(np.float32).max if maxt is None else maxt
        return rays

    def ray_intersect(self, o, d, time=0.0, maxt=None):
        """Scene::ray_intersect over arrays of rays -> dict(t, p, n, sh_n, sh_s, sh_t, wi, ids, uv, prim_uv, prim_index, valid) (dtof_ray_intersect_uv)"""
        rays = self._rays(o, d, time, maxt)
        out, ids, uv = np.zeros((len(rays), 19), np.float32), np.zeros((len(rays), 3), np.int32), np.zeros((len(rays), 4), np.float32)
        _check(_lib().dtof_ray_intersect_uv(self._h, len(rays), rays.ctypes.data, out.ctypes.data, ids.ctypes.data, uv.ctypes.data))
        return {"t": out[:, 0], "p": out[:, 1:4], "n": out[:, 4:7], "sh_n": out[:, 7:10], "sh_s": out[:, 10:13], "sh_t": out[:, 13:16],
                "wi": out[:, 16:19], "ids": ids, "uv": uv[:, 0:2], "prim_uv": uv[:, 2:4], "prim_index": ids[:, 2], "valid": ids[:, 0] >= 0}

    def ray_test(self, o, d, time=0.0, maxt=None):
        """Scene::ray_test over arrays of rays -> bool array (dtof_ray_test)"""
        rays = self._rays(o, d, time, maxt)
        occ = np.zeros(len(rays), np.int32)
        _check(_lib().dtof_ray_test(self._h, len(rays), rays.ctypes.data, occ.ctypes.data))
        return occ != 0

    FLAT_FORMS = {"generic": 0, "one_wall": 1, "shape": 2}

    def flat_query(self, rays8, form=0, any=False):
        """The ray query of a flat scene's fused kernels over an (n, 8) array of rays o, d, time, maxt (dtof_flat_query).  form: 0 / "generic", 1 / "one_wall",
        2 / "shape" -- the instantiation of trace_flat that runs.  Closest hit -> dict(t, u, v, obj) (inf, 0, 0, -1 on a miss); any=True -> int32 array of 1 / 0.
        A scene without a flat table, a form whose facts the scene does not meet and more than 2^24 rays raise DtofError; non-finite components are taken as they are."""
        rays = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        form = self.FLAT_FORMS.get(form, form)
        out, ids = np.zeros((len(rays), 3), np.float32), np.zeros(len(rays), np.int32)
        _check(_lib().dtof_flat_query(self._h, int(form), 1 if any else 0, len(rays), rays.ctypes.data, None if any else out.ctypes.data, ids.ctypes.data))
        return ids if any else {"t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "obj": ids}

    def flat_query_pairs(self, rays8, any=False):
        """flat_query in the pair form of the "shape" walk (dtof_flat_query_pairs), the one a frame's kernel runs where the two lanes of a correlated pair hold the same
        ray: rays 2k and 2k + 1 are equal in o, d and maxt, bit for bit, and have times of their own.  Same results as flat_query.  An odd count, a pair that differs
        and a table other than five rectangles with the wall at index 2 raise DtofError."""
        rays = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        out, ids = np.zeros((len(rays), 3), np.float32), np.zeros(len(rays), np.int32)
        _check(_lib().dtof_flat_query_pairs(self._h, 1 if any else 0, len(rays), rays.ctypes.data, None if any else out.ctypes.data, ids.ctypes.data))
        return ids if any else {"t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "obj": ids}

    def pair_setup_lanes(self, seed, spp, lane_begin, n, form=1):
        """Lane generation of the headline frame's kernel over lanes [lane_begin, lane_begin + n) (dtof_pair_setup_lanes), walked in 512-lane segments of 64-lane chunks
        as the first-bounce launch walks them.  form 0: every lane generates itself; form 1: what the two lanes of a correlated pair share is evaluated once per pair,
        for the pairs of two chunks at a time.  -> (n, 16) uint32: sample_pos[2], time, ray_o[3], ray_d[3], maxt as float bits, the path stream's state (low, high
        word), its selector, three zeros.  A scene or sample count the kernels are not compiled for, a lane_begin or n that is no multiple of 64 and n above 2^24
        raise DtofError before anything is launched."""
        out = np.zeros((int(n), 16), np.uint32)
        _check(_lib().dtof_pair_setup_lanes(self._h, int(form), seed, spp, lane_begin, n, out.ctypes.data))
        return out

    TREE_FORMS = {"float": 0, "half_overflow": 1, "half_overflow_tlas_lds": 2, "defer_pair": 3, "half_every_shape": 4}

    def tree_query(self, rays8, form=0, any=False):
        """The TLAS / BLAS ray query over an (n, 8) array of rays o, d, time, maxt in the form a frame's ray kernels run it (dtof_tree_query).  form: 0 / "float",
        1 / "half_overflow", 2 / "half_overflow_tlas_lds", 3 / "defer_pair", 4 / "half_every_shape".  Closest hit -> dict(t, u, v, ids (n, 3): object, shape in its
        group, primitive) (inf, 0, 0, -1 on a miss); any=True -> int32 array of 1 / 0.  A form the scene does not meet and more than 2^24 rays raise DtofError;
        non-finite components are taken as they are."""
        rays = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        form = self.TREE_FORMS.get(form, form)
        out, ids = np.zeros((len(rays), 3), np.float32), np.zeros(len(rays) if any else (len(rays), 3), np.int32)
        _check(_lib().dtof_tree_query(self._h, int(form), 1 if any else 0, len(rays), rays.ctypes.data, None if any else out.ctypes.data, ids.ctypes.data))
        return ids if any else {"t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "ids": ids}

    def cancel(self):
        _lib().dtof_cancel(self._h)


# DTOF_COMP_* of include/dtof.h
COMPONENTS = {"microfacet_eval": (0, 1), "microfacet_pdf": (1, 1), "microfacet_g1": (2, 1), "microfacet_sample": (3, 4), "fresnel": (4, 4),
              "fresnel_conductor": (5, 1), "rfilter": (6, 1), "warp_cosine_hemisphere": (7, 3), "warp_disk_concentric": (8, 2),
              "warp_uniform_triangle": (9, 2), "warp_uniform_sphere": (10, 3), "coordinate_system": (11, 6), "tea_float32": (12, 1), "math": (13, 1)}


def eval_component(name, inputs, params=()):
    """dtof_eval_component: one of the device functions the kernels are built from, over the rows of `inputs` (n x k float32)"""
    comp, n_out = COMPONENTS[name]
    x = np.ascontiguousarray(np.atleast_2d(np.asarray(inputs, np.float32)))
    p = np.ascontiguousarray(np.asarray(params, np.float32).reshape(-1))
    out = np.zeros((len(x), n_out), np.float32)
    _check(_lib().dtof_eval_component(comp, p.ctypes.data if p.size else None, p.size, x.ctypes.data, x.shape[1], out.ctypes.data, n_out, len(x)))
    return out


class Integrator:
    """What mi.load_dict({'type': 'dopplertofpath', ...}) returns: a plugin description that is bound to a
    scene at render time (the reference's integrator objects are scene-independent too)."""

    def __init__(self, props):
        self.props = dict(props)
        self._h = C.c_void_p()
        _check(_lib().dtof_integrator_create(*(_plugin_args(self.props) + (C.byref(self._h),))))   # constructor-time validation

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and _LIB is not None:
            _LIB.dtof_integrator_destroy(self._h)
            self._h = C.c_void_p()

    def render(self, scene, seed=0, spp=0, sensor=0, offsets=None, variants=None, film="float32"):
        """film="float64": the float64 film of Scene.render; like the batched forms it makes this integrator the scene's"""
        if offsets is not None and variants is not None:
            raise DtofError("pass either offsets or variants, not both")
        if offsets is not None or variants is not None or _film64(film):
            scene.set_integrator(self.props)
            return scene.render(seed=seed, spp=spp, sensor=sensor, offsets=offsets, variants=variants, film=film)
        w, h = scene.size
        st, out = _Stats(), np.zeros((h, w, 4 if scene.info()["has_alpha"] else 3), np.float32)
        _check(_lib().dtof_integrator_render(self._h, None, scene._h, sensor, seed, spp, out.ctypes.data, C.byref(st)))
        scene.last_stats = st.as_dict()
        return out


def load_file(path, **params):
    h = C.c_void_p()
    names, values, n = _kv(params)
    _check(_lib().dtof_scene_load_file(os.fspath(path).encode(), names, values, n, C.byref(h)))
    return Scene(h)


def load_string(xml, **params):
    h = C.c_void_p()
    names, values, n = _kv(params)
    _check(_lib().dtof_scene_load_string(xml.encode(), names, values, n, C.byref(h)))
    return Scene(h)


def load_dict(d):
    t = d.get("type")
    if t in ("dopplertofpath", "path", "velocity"):
        return Integrator(d)
    raise DtofError('load_dict: unsupported plugin type "%s" (supported: dopplertofpath, path, velocity)' % t)


def render(scene, spp=0, seed=0, integrator=None, sensor=0):
    """mi.render(scene, spp=..., seed=..., integrator=...) (src/python/python/util.py)"""
    if integrator is not None:
        return integrator.render(scene, seed=seed, spp=spp, sensor=sensor)
    return scene.render(seed=seed, spp=spp, sensor=sensor)


def render_multi_pass(scene, integrator, total_spp, single_pass_spp=1024, show_progress=False, film="float32"):
    """doppler_tutorials/src/program_runner.py:11-31: mean of renders with seeds 0..n-1, each of
    min(single_pass_spp, total_spp) samples per pixel.  film="float64": every pass through the float64 film."""
    single = min(single_pass_spp, total_spp)
    n_pass = max(total_spp // single, 1)
    film_kw = dict(film=film) if _film64(film) else {}
    acc = None
    for i in range(n_pass):
        img = integrator.render(scene, seed=i, spp=single, **film_kw).astype(np.float32)
        acc = img if acc is None else acc + img
    return acc / np.float32(n_pass)


def to_tof_image(img, exposure_time=0.0015):
    """doppler_tutorials/src/utils/image_utils.py:20-31: luminance * exposure time"""
    img = np.asarray(img)
    return (0.2126 * img[..., 0] + 0.7152 * img[..., 1] + 0.0722 * img[..., 2]) * exposure_time


class Sampler:
    """Array-of-lanes `correlated` sampler living on the GPU (include/mitsuba/render/sampler.h:99-168)."""

    def __init__(self, sample_count=4, seed=0, time_correlate_number=2, path_correlate_number=None):
        self._h = C.c_void_p()
        pcn = time_correlate_number if path_correlate_number is None else path_correlate_number
        _check(_lib().dtof_sampler_create(sample_count, seed, time_correlate_number, pcn, C.byref(self._h)))

    def __del__(self):
        try:
            if self._h:
                _lib().dtof_sampler_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def wavefront_size(self):
        return _lib().dtof_sampler_wavefront_size(self._h)

    def sample_count(self):
        return _lib().dtof_sampler_sample_count(self._h)

    def set_samples_per_wavefront(self, spw):
        _check(_lib().dtof_sampler_set_samples_per_wavefront(self._h, spw))

    def set_sample_count(self, spp):
        _check(_lib().dtof_sampler_set_sample_count(self._h, spp))

    def seeded(self):
        return bool(_lib().dtof_sampler_seeded(self._h))

    def _from_handle(self, fn):
        other = Sampler.__new__(Sampler)
        other._h = C.c_void_p()
        _check(fn(self._h, C.byref(other._h)))
        return other

    def fork(self):
        """same configuration, unseeded (src/samplers/correlated.cpp:25-32)"""
        return self._from_handle(_lib().dtof_sampler_fork)

    def clone(self):
        """same configuration and the same per-lane state (src/samplers/correlated.cpp:34-36)"""
        return self._from_handle(_lib().dtof_sampler_clone)

    def seed(self, seed, wavefront_size=0xffffffff):
        _check(_lib().dtof_sampler_seed(self._h, seed, wavefront_size))

    def advance(self):
        _check(_lib().dtof_sampler_advance(self._h))

    def _out(self, k=1):
        n = self.wavefront_size()
        return np.zeros((n, k) if k > 1 else n, np.float32)

    def next_1d(self):
        o = self._out()
        _check(_lib().dtof_sampler_next_1d(self._h, o.ctypes.data))
        return o

    def next_2d(self):
        o = self._out(2)
        _check(_lib().dtof_sampler_next_2d(self._h, o.ctypes.data))
        return o

    def _corr(self, correlate):
        if isinstance(correlate, (bool, int, np.bool_)):
            return None, int(bool(correlate)), None
        a = np.ascontiguousarray(correlate, dtype=np.uint8)
        return a.ctypes.data, 0, a

    def next_1d_correlate(self, correlate=False):
        o = self._out()
        p, allf, keep = self._corr(correlate)
        _check(_lib().dtof_sampler_next_1d_correlate(self._h, p, allf, o.ctypes.data))
        return o

    def next_2d_correlate(self, correlate=False):
        o = self._out(2)
        p, allf, keep = self._corr(correlate)
        _check(_lib().dtof_sampler_next_2d_correlate(self._h, p, allf, o.ctypes.data))
        return o

    def next_1d_time(self, strategy=ETimeSampling.UNIFORM, antithetic_shift=0.0, use_stratified_sampling_for_each_interval=False):
        o = self._out()
        _check(_lib().dtof_sampler_next_1d_time(self._h, int(strategy), float(antithetic_shift),
                                                int(bool(use_stratified_sampling_for_each_interval)), o.ctypes.data))
        return o

    def state(self):
        n = self.wavefront_size()
        o = np.zeros((n, 7), np.uint32)
        _check(_lib().dtof_sampler_get_state(self._h, o.ctypes.data))
        return o


# ------------------------------------------------------------------------------------------------ variant selection
# `import mitsuba as mi; mi.set_variant('cuda_rgb')` opens every tutorial script (program_runner.py:1-2).  This library has
# exactly one back end: RGB colour, float32 arithmetic, HIP kernels -- the counterpart of the reference's *_rgb variants.
_VARIANT = "hip_rgb"


def variants():
    return ["hip_rgb"]


def variant():
    return _VARIANT


def set_variant(*names):
    """Accepts the first usable of `names`; every scalar_/llvm_/cuda_ *_rgb variant of the reference maps onto hip_rgb
    (src/python/python/__init__.py: mi.set_variant).  Spectral, polarised, mono and double-precision variants do not exist here."""
    for n in names:
        if n == "hip_rgb" or (n.split("_", 1)[0] in ("scalar", "llvm", "cuda") and n.endswith("_rgb") and "_ad_" not in "_" + n.split("_", 1)[1] + "_"):
            return
    raise ImportError("Requested an unsupported variant \"%s\". The following variants are available: hip_rgb (the *_rgb variants of "
                      "the reference map onto it)." % ", ".join(names))
