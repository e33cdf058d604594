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
from ._abi import (MAX_VARIANTS, DtofError, _AdaptiveParams, _check, _DenoiseParams, _Info, _lib, _Modulation, _Stats, _TemporalBuffers, _TemporalParams,   # noqa: F401
                   lib_path)
from ._denoiser import Denoiser
from ._plugins import (ETimeSampling, Integrator, Sampler, load_dict, load_file, load_string, render, render_multi_pass, set_variant, to_tof_image,   # noqa: F401
                       variant, variants)
from ._scene import (ADAPTIVE_MODES, AOV_TYPES, COMPONENTS, DEPTH_OUTPUTS, FILMS, FLAT_GEOMETRY, MAX_DEPTH_FREQUENCIES, MAX_VELOCITY_OFFSETS, MOMENT_PLANES, Scene, _adaptive_params, _aov_parse,   # noqa: F401
                     _film64, _moment_dict, _plugin_args, _variant_array, _variant_freq, adaptive_select, aov_channels, default_max_path_length, depth_map_variants, eval_component,
                     velocity_map_variants)

__all__ = ["load_file", "load_string", "load_dict", "Scene", "Integrator", "Sampler", "DtofError", "render",
           "render_multi_pass", "to_tof_image", "lib_path", "ETimeSampling", "velocity_map_variants", "MOMENT_PLANES", "aov_channels", "AOV_TYPES", "Denoiser", "adaptive_select",
           "ADAPTIVE_MODES", "depth_map_variants"]
