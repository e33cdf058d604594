"""The C ABI of include/dtof.h as ctypes sees it: the library, the mirrored structures and ONE table of signatures.  The table is written by hand, in the header's
order, and tests/test_binding_abi_cpu.py holds every entry and every structure field against the header."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class DtofError(RuntimeError):
    pass


class _Info(C.Structure):   # dtof_scene_info
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


class _Stats(C.Structure):   # dtof_render_stats
    _fields_ = [("n_paths", C.c_uint64), ("n_bounces", C.c_uint64), ("n_shadow_rays", C.c_uint64),
                ("ms_total", C.c_double), ("ms_generate", C.c_double), ("ms_trace", C.c_double),
                ("ms_shade", C.c_double), ("ms_shadow", C.c_double), ("ms_splat", C.c_double),
                ("n_launches_trace", C.c_uint32), ("n_launches_shade", C.c_uint32), ("n_launches_shadow", C.c_uint32),
                ("n_batches", C.c_uint32), ("n_launches_first", C.c_uint32), ("ms_first", C.c_double),
                ("n_inline_iterations", C.c_uint32), ("n_bounces_inline", C.c_uint64), ("n_fused_splat_launches", C.c_uint32),
                ("n_plan_facts_launches", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class _Modulation(C.Structure):   # dtof_modulation
    _fields_ = [("hetero_frequency", C.c_float), ("hetero_offset", C.c_float)]


MAX_VARIANTS = 4   # modulation variants (films) one traversal evaluates (kMaxOffsets)


class _DenoiseParams(C.Structure):   # dtof_denoise_params
    _fields_ = [("levels", C.c_int32), ("sigma_normal", C.c_double), ("sigma_position", C.c_double), ("sigma_luminance", C.c_double)]


class _TemporalParams(C.Structure):   # dtof_temporal_params
    _fields_ = [("alpha_min", C.c_double), ("max_length", C.c_double), ("tau_normal", C.c_double)]


class _TemporalBuffers(C.Structure):   # dtof_temporal_buffers
    _fields_ = [(name, C.c_void_p) for name in ("colour", "variance", "normal", "ids", "flow", "h_colour", "h_variance", "h_normal", "h_ids", "h_length",
                                                "o_colour", "o_variance", "o_length", "o_colour_f32")]


class _DenoisedOutputs(C.Structure):   # dtof_denoised_outputs
    _fields_ = [(name, C.c_void_p) for name in ("denoised", "denoised_map", "sum", "moments", "aovs", "colour", "variance", "normal", "position",
                                                "denoised_variance", "noisy_map", "sigma_position")]


class _AdaptiveParams(C.Structure):   # dtof_adaptive_params
    _fields_ = [("mode", C.c_int32), ("n_pairs", C.c_int32), ("homodyne", C.c_int32 * 2), ("heterodyne", C.c_int32 * 2),
                ("tol", C.c_double), ("floor", C.c_double), ("exposure_time", C.c_double), ("w_g_mhz", C.c_double)]


# ------------------------------------------------------------------------------------------------ the signatures, name -> (restype, argtypes), in the header's order
_int, _i32, _u32, _i64, _u64, _sz, _f32, _f64 = C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_size_t, C.c_float, C.c_double
_vp, _str, _cpp, _out, _st = C.c_void_p, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(_Stats)
_rows = [_vp, _u32, _u32, _i32, _i32, _vp, _int, _vp]               # scene, seed, spp, row_begin, row_end, offsets | variants, their count, the device film
_stripes = [_vp, _u32, _u32, _i32, _i32, _i32, _vp, _int, _vp]      # scene, seed, spp, first_row, stripe_rows, stripe_period, ...
_velocity = [_vp, _u32, _u32, _vp, _int, _f64, _f64, _vp, _vp, _vp, _st]

SIGNATURES = {
    "dtof_version": (_str, []),
    "dtof_last_error": (_str, []),
    # scene loading
    "dtof_scene_load_file": (_int, [_str, _cpp, _cpp, _int, _out]),
    "dtof_scene_load_string": (_int, [_str, _cpp, _cpp, _int, _out]),
    "dtof_scene_destroy": (None, [_vp]),
    "dtof_scene_set_integrator": (_int, [_vp, _str, _cpp, _str, _cpp, _int]),
    "dtof_scene_set_sampler": (_int, [_vp, _str, _cpp, _str, _cpp, _int]),
    "dtof_integrator_create": (_int, [_str, _cpp, _str, _cpp, _int, _out]),
    "dtof_integrator_destroy": (None, [_vp]),
    "dtof_sampler_plugin_create": (_int, [_str, _cpp, _str, _cpp, _int, _out]),
    "dtof_sampler_plugin_destroy": (None, [_vp]),
    "dtof_scene_get_info": (_int, [_vp, C.POINTER(_Info)]),
    "dtof_scene_export": (_int, [_vp, _int, _vp, _sz, C.POINTER(_sz)]),
    "dtof_scene_world_to_pixel": (_int, [_vp, _vp]),
    "dtof_camera_rays": (_int, [_vp, _u32, _vp, _vp]),
    "dtof_bsdf_eval": (_int, [_vp, _u32, _u32, _vp, _vp]),
    "dtof_bsdf_eval_ex": (_int, [_vp, _u32, _int, _u32, _vp, _vp]),
    "dtof_emitter_eval": (_int, [_vp, _int, _int, _i32, _u32, _vp, _vp]),
    # rendering
    "dtof_render": (_int, [_vp, _u32, _u32, _u32, _vp, _st]),
    "dtof_integrator_render": (_int, [_vp, _vp, _vp, _u32, _u32, _u32, _vp, _st]),
    "dtof_render_rows": (_int, _rows + [_st]),
    "dtof_render_rows_async": (_int, _rows),
    "dtof_clear_async": (_int, [_vp, _vp, _sz]),
    "dtof_develop_async": (_int, [_vp, _vp, _vp, _i64]),
    "dtof_async_collect": (_int, [_vp, _vp, _vp, _u32, _vp]),
    "dtof_render_stripes": (_int, _stripes + [_st]),
    "dtof_scene_set_stream": (_int, [_vp, _vp]),
    "dtof_render_stripes_async": (_int, _stripes),
    "dtof_scene_set_film_layout": (_int, [_vp, _i32, _u64]),
    "dtof_develop": (_int, [_vp, _vp, _i64]),
    "dtof_develop_on_stream": (_int, [_vp, _vp, _i64, _vp]),
    "dtof_develop_rgba": (_int, [_vp, _vp, _vp, _i64]),
    "dtof_render_offsets": (_int, [_vp, _u32, _u32, _vp, _int, _vp, _st]),
    # modulation variants
    "dtof_render_variants": (_int, [_vp, _u32, _u32, _vp, _int, _vp, _st]),
    "dtof_render_rows_variants": (_int, _rows + [_st]),
    "dtof_render_rows_variants_async": (_int, _rows),
    "dtof_render_stripes_variants": (_int, _stripes + [_st]),
    "dtof_render_stripes_variants_async": (_int, _stripes),
    # radial-velocity map
    "dtof_develop_accumulate_async": (_int, [_vp, _vp, _i32, _u64, _vp, _i64, _int]),
    "dtof_velocity_map_async": (_int, [_vp, _vp, _int, _vp, _vp, _u32, _f64, _f64, _i64, _vp, _vp, _vp]),
    "dtof_velocity_map_variants": (_int, [_vp, _int, _vp]),
    "dtof_render_velocity_map": (_int, _velocity),
    # float64 film
    "dtof_render_variants_f64": (_int, [_vp, _u32, _u32, _vp, _int, _vp, _vp, _st]),
    "dtof_render_rows_variants_f64": (_int, _rows + [_i32, _u64, _st]),
    "dtof_develop_f64_async": (_int, [_vp, _vp, _vp, _i64]),
    "dtof_develop_rgba_f64_async": (_int, [_vp, _vp, _vp, _vp, _i64]),
    "dtof_render_velocity_map_f64": (_int, _velocity),
    # modulation frequency per variant
    "dtof_render_variants_freq": (_int, [_vp, _u32, _u32, _vp, _vp, _int, _vp, _st]),
    "dtof_render_variants_freq_f64": (_int, [_vp, _u32, _u32, _vp, _vp, _int, _vp, _vp, _st]),
    "dtof_sample_lanes_variants_freq": (_int, [_vp, _u32, _u32, _vp, _vp, _int, _u64, _u64, _vp, _vp, _vp]),
    # depth map
    "dtof_depth_map_variants": (_int, [_vp, _int, _vp, _vp]),
    "dtof_depth_map_async": (_int, [_vp, _vp, _int, _vp, _vp, _vp, _u32, _f64, _f64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "dtof_render_depth_map": (_int, [_vp, _u32, _u32, _vp, _int, _f64, _f64, _int, _vp, _vp, _vp, _vp, _vp, _vp, _st]),
    # moment film
    "dtof_moment_planes": (_int, [_int]),
    "dtof_render_moments": (_int, [_vp, _u32, _u32, _u32, _vp, _int, _int, _vp, _st]),
    # geometry channels of the `aov` integrator
    "dtof_aov_parse": (_int, [_str, _vp, _int, C.POINTER(_int), _vp, _sz, C.POINTER(_int)]),
    "dtof_scene_get_aovs": (_int, [_vp, _vp, _sz]),
    "dtof_render_aovs": (_int, [_vp, _u32, _u32, _u32, _vp, _int, _int, _vp, _st]),
    "dtof_sample_aov_lanes": (_int, [_vp, _u32, _u32, _vp, _int, _u64, _u64, _vp, _vp]),
    # the flow film
    "dtof_render_flow": (_int, [_vp, _u32, _u32, _u32, _int, _vp, _st]),
    "dtof_sample_flow_lanes": (_int, [_vp, _u32, _u32, _u64, _u64, _vp, _vp]),
    # denoiser
    "dtof_denoise_async": (_int, [_vp, _vp, _int, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dtof_denoise": (_int, [_vp, _int, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    # denoiser, temporal stage
    "dtof_denoise_temporal_async": (_int, [_vp, _vp, _int, _i32, _i32, _vp]),
    "dtof_denoise_temporal": (_int, [_vp, _int, _i32, _i32, _vp]),
    # denoised renders on the device
    "dtof_denoise_inputs_async": (_int, [_vp, _int, _vp, _vp, _vp, _int, _i64, _u32, _f64, _f64, _vp, _vp, _vp, _vp, _vp]),
    "dtof_render_denoised": (_int, [_vp, _u32, _u32, _u32, _vp, _int, _vp, _int, _vp, _st]),
    "dtof_render_velocity_map_denoised": (_int, [_vp, _u32, _u32, _u32, _vp, _f64, _f64, _vp, _int, _vp, _st]),
    # adaptive sampling
    "dtof_adaptive_select": (_int, [_vp, _i64, _int, _vp, _u32, _vp, _vp, _vp, _vp]),
    "dtof_render_pixels": (_int, [_vp, _u32, _u32, _vp, _u32, _vp, _int, _int, _vp, _vp, _st]),
    "dtof_sample_lanes_pixels": (_int, [_vp, _u32, _u32, _vp, _u32, _vp, _int, _vp, _vp, _vp]),
    "dtof_render_adaptive": (_int, [_vp, _u32, _u32, _u32, _u32, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _st]),
    "dtof_cancel": (None, [_vp]),
    "dtof_scene_plan_facts_launches": (_u64, [_vp]),
    "dtof_scene_last_plan_facts": (_u32, [_vp]),
    "dtof_scene_last_splat": (_u32, [_vp]),
    "dtof_sample_lanes": (_int, [_vp, _u32, _u32, _u64, _u64, _vp]),
    "dtof_sample_lanes_valid": (_int, [_vp, _u32, _u32, _u64, _u64, _vp, _vp]),
    "dtof_sample_lanes_variants": (_int, [_vp, _u32, _u32, _vp, _int, _u64, _u64, _vp, _vp, _vp]),
    # sampler surface
    "dtof_sampler_create": (_int, [_u32, _u32, _i32, _i32, _out]),
    "dtof_sampler_destroy": (None, [_vp]),
    "dtof_sampler_seed": (_int, [_vp, _u32, _u32]),
    "dtof_sampler_set_samples_per_wavefront": (_int, [_vp, _u32]),
    "dtof_sampler_advance": (_int, [_vp]),
    "dtof_sampler_next_1d": (_int, [_vp, _vp]),
    "dtof_sampler_next_2d": (_int, [_vp, _vp]),
    "dtof_sampler_next_1d_correlate": (_int, [_vp, _vp, _int, _vp]),
    "dtof_sampler_next_2d_correlate": (_int, [_vp, _vp, _int, _vp]),
    "dtof_sampler_next_1d_time": (_int, [_vp, _int, _f32, _int, _vp]),
    "dtof_sampler_get_state": (_int, [_vp, _vp]),
    "dtof_sampler_fork": (_int, [_vp, _out]),
    "dtof_sampler_clone": (_int, [_vp, _out]),
    "dtof_sampler_set_sample_count": (_int, [_vp, _u32]),
    "dtof_sampler_seeded": (_int, [_vp]),
    "dtof_sampler_wavefront_size": (_u32, [_vp]),
    "dtof_sampler_sample_count": (_u32, [_vp]),
    # modulation functions
    "dtof_eval_modulation": (_int, [_vp, _int, _vp, _vp, _vp, _u32]),
    # ray queries
    "dtof_ray_intersect": (_int, [_vp, _u32, _vp, _vp, _vp]),
    "dtof_ray_intersect_uv": (_int, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "dtof_ray_test": (_int, [_vp, _u32, _vp, _vp]),
    "dtof_flat_query": (_int, [_vp, _int, _int, _u32, _vp, _vp, _vp]),
    "dtof_flat_query_pairs": (_int, [_vp, _int, _u32, _vp, _vp, _vp]),
    "dtof_flat_query_zrow": (_int, [_vp, _int, _u32, _vp, _vp, _vp, _vp]),
    "dtof_pair_setup_lanes": (_int, [_vp, _int, _u32, _u32, _u64, _u64, _vp]),
    "dtof_tree_query": (_int, [_vp, _int, _int, _u32, _vp, _vp, _vp]),
    "dtof_fused_query": (_int, [_vp, _int, _int, _int, _u32, _vp, _vp, _vp]),
    "dtof_surface_eval": (_int, [_vp, _int, _int, _u32, _vp, _vp, _vp]),
    # component evaluation
    "dtof_eval_component": (_int, [_int, _vp, _int, _vp, _int, _vp, _int, _u32]),
}


def declare(lib, signatures=SIGNATURES):
    """set restype and argtypes of every entry that `lib` has; one it lacks (an older build timed through DTOF_LIB) is skipped and raises AttributeError where it is called"""
    for name, (restype, argtypes) in signatures.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
    return lib


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
    _LIB = declare(C.CDLL(path))
    return _LIB


def _check(rc):
    if rc != 0:
        raise DtofError(_lib().dtof_last_error().decode("utf-8", "replace"))


def _ptr(a):
    """the pointer argument of an optional array"""
    return None if a is None else a.ctypes.data


def _release(owner, entry):
    """__del__ of the owner of a handle `_h`: destroy it once; never raises and never loads the library (a half-constructed owner, interpreter exit)"""
    try:
        if owner._h and _LIB is not None:
            getattr(_LIB, entry)(owner._h)
            owner._h = None
    except Exception:
        pass
