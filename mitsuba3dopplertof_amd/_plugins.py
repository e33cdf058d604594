"""The plugin objects and module-level calls of the Mitsuba interface: load_file / load_string / load_dict, Integrator, Sampler, render, and the variant shim."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import DtofError, _check, _release
from ._scene import Scene, _either, _film64, _plugin_args


class ETimeSampling:   # include/mitsuba/render/sampler.h:27-34
    UNIFORM, STRATIFIED, ANTITHETIC, ANTITHETIC_MIRROR, PERIODIC, REGULAR = 0, 1, 2, 3, 4, 5


def _kv(params):
    names = [str(k).encode() for k in params]
    values = [str(v).encode() for v in params.values()]
    n = len(names)
    return (C.c_char_p * max(n, 1))(*names), (C.c_char_p * max(n, 1))(*values), n


class Integrator:
    """What mi.load_dict({'type': 'dopplertofpath', ...}) returns: a plugin description that is bound to a
    scene at render time (the reference's integrator objects are scene-independent too)."""

    def __init__(self, props):
        self.props = dict(props)
        self._h = C.c_void_p()
        _check(_abi._lib().dtof_integrator_create(*(_plugin_args(self.props) + (C.byref(self._h),))))   # constructor-time validation

    def __del__(self):
        _release(self, "dtof_integrator_destroy")

    def render(self, scene, seed=0, spp=0, sensor=0, offsets=None, variants=None, film="float32"):
        """film="float64": the float64 film of Scene.render; like the batched forms it makes this integrator the scene's"""
        _either(offsets, variants)
        if offsets is not None or variants is not None or _film64(film):
            scene.set_integrator(self.props)
            return scene.render(seed=seed, spp=spp, sensor=sensor, offsets=offsets, variants=variants, film=film)
        w, h = scene.size
        out = np.zeros((h, w, 4 if scene.info()["has_alpha"] else 3), np.float32)
        scene._timed(_abi._lib().dtof_integrator_render, self._h, None, scene._h, sensor, seed, spp, out.ctypes.data)
        return out


def _load(name, text, params):
    h = C.c_void_p()
    names, values, n = _kv(params)
    _check(getattr(_abi._lib(), name)(text.encode(), names, values, n, C.byref(h)))
    return Scene(h)


def load_file(path, **params):
    return _load("dtof_scene_load_file", os.fspath(path), params)


def load_string(xml, **params):
    return _load("dtof_scene_load_string", xml, params)


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
        _check(_abi._lib().dtof_sampler_create(sample_count, seed, time_correlate_number, pcn, C.byref(self._h)))

    def __del__(self):
        _release(self, "dtof_sampler_destroy")

    def wavefront_size(self):
        return _abi._lib().dtof_sampler_wavefront_size(self._h)

    def sample_count(self):
        return _abi._lib().dtof_sampler_sample_count(self._h)

    def set_samples_per_wavefront(self, spw):
        _check(_abi._lib().dtof_sampler_set_samples_per_wavefront(self._h, spw))

    def set_sample_count(self, spp):
        _check(_abi._lib().dtof_sampler_set_sample_count(self._h, spp))

    def seeded(self):
        return bool(_abi._lib().dtof_sampler_seeded(self._h))

    def _from_handle(self, fn):
        other = Sampler.__new__(Sampler)
        other._h = C.c_void_p()
        _check(fn(self._h, C.byref(other._h)))
        return other

    def fork(self):
        """same configuration, unseeded (src/samplers/correlated.cpp:25-32)"""
        return self._from_handle(_abi._lib().dtof_sampler_fork)

    def clone(self):
        """same configuration and the same per-lane state (src/samplers/correlated.cpp:34-36)"""
        return self._from_handle(_abi._lib().dtof_sampler_clone)

    def seed(self, seed, wavefront_size=0xffffffff):
        _check(_abi._lib().dtof_sampler_seed(self._h, seed, wavefront_size))

    def advance(self):
        _check(_abi._lib().dtof_sampler_advance(self._h))

    def _draw(self, name, k, *args, dtype=np.float32):
        """one record of every lane through the entry `name` -> (n,) array, (n, k) for k > 1"""
        n = self.wavefront_size()
        o = np.zeros((n, k) if k > 1 else n, dtype)
        _check(getattr(_abi._lib(), name)(self._h, *args, o.ctypes.data))
        return o

    def next_1d(self):
        return self._draw("dtof_sampler_next_1d", 1)

    def next_2d(self):
        return self._draw("dtof_sampler_next_2d", 2)

    def _corr(self, correlate):
        if isinstance(correlate, (bool, int, np.bool_)):
            return None, int(bool(correlate)), None
        a = np.ascontiguousarray(correlate, dtype=np.uint8)
        return a.ctypes.data, 0, a

    def next_1d_correlate(self, correlate=False):
        p, allf, keep = self._corr(correlate)
        return self._draw("dtof_sampler_next_1d_correlate", 1, p, allf)

    def next_2d_correlate(self, correlate=False):
        p, allf, keep = self._corr(correlate)
        return self._draw("dtof_sampler_next_2d_correlate", 2, p, allf)

    def next_1d_time(self, strategy=ETimeSampling.UNIFORM, antithetic_shift=0.0, use_stratified_sampling_for_each_interval=False):
        return self._draw("dtof_sampler_next_1d_time", 1, int(strategy), float(antithetic_shift), int(bool(use_stratified_sampling_for_each_interval)))

    def state(self):
        return self._draw("dtof_sampler_get_state", 7, dtype=np.uint32)


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
