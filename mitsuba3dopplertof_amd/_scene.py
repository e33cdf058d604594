"""Scene: a loaded scene and every call over it -- renders, films, lane dumps, ray queries -- and the module-level functions over the same entries."""
import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import MAX_VARIANTS, DtofError, _AdaptiveParams, _check, _DenoisedOutputs, _DenoiseParams, _Info, _ptr, _release, _Stats
from ._denoiser import Denoiser


# dtof_kernels.h: kFlatShapeFields -- the presence bit, the object count (bits 19 .. 22) and the wall's index (bits 23 .. 25)
_FLAT_SHAPE_FIELDS = 1 << 18 | 0xf << 19 | 0x7 << 23
# dtof_kernels.h: kFactPairSamples -- above the shape fields: not a fact of the plan's own but work the kernel lets the two lanes of a pair share
_PAIR_SAMPLES = 1 << 26


FLAT_GEOMETRY = np.array([[1, 0, 0,  0, 1, 0,  0, 0, 1,  1, 0, 0,  0, 1, 0,  0, 0, 1]], np.float32)   # dp_du, dp_dv, n, sh_s, sh_t, sh_n of dtof_bsdf_eval


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


def _variant_array(variants):
    """[(hetero_frequency, hetero_offset), ...] -> (n, 2) float32 array laid out like dtof_modulation[n]"""
    v = np.ascontiguousarray(variants, dtype=np.float32)
    if v.ndim != 2 or v.shape[1] != 2:
        raise DtofError("variants must be a sequence of (hetero_frequency, hetero_offset) pairs")
    return v


def _variant_freq(variants):
    """pairs, or (hetero_frequency, hetero_offset, w_g_mhz) triples -> ((n, 2) float32 array like dtof_modulation[n], (n,) float32 frequencies or None for pairs).
    All pairs or all triples: a mixture is refused."""
    try:
        widths = {len(v) for v in variants}
    except TypeError:
        widths = set()
    if widths == {3}:
        v = np.ascontiguousarray(variants, dtype=np.float32)
        return np.ascontiguousarray(v[:, :2]), np.ascontiguousarray(v[:, 2])
    if 3 in widths:
        raise DtofError("variants are all (hetero_frequency, hetero_offset) pairs or all (hetero_frequency, hetero_offset, w_g_mhz) triples, not a mixture")
    return _variant_array(variants), None


def _either(offsets, variants):
    if offsets is not None and variants is not None:
        raise DtofError("pass either offsets or variants, not both")


def _variant_args(variants, offsets=None, cell=False):
    """The (array to keep alive, pointer, count) of a call's `variants` or `offsets` argument, and whether it is the variants form; neither: (None, None, 0, False),
    the integrator's own pair.  cell=True: the variants of ONE traversal's moment film, 1 .. 4 of them."""
    if variants is not None:
        _either(offsets, variants)
        v = _variant_array(variants)
        if cell and not 1 <= len(v) <= MAX_VARIANTS:
            raise DtofError("between 1 and 4 modulation variants make a moment film")
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
    return int(_abi._lib().dtof_moment_planes(int(n_variants)))


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
    _check(_abi._lib().dtof_adaptive_select(pl.ctypes.data, n, k, C.byref(prm), int(spp), cnt.ctypes.data, out.ctypes.data, C.byref(out_n), metric.ctypes.data))
    return out[:out_n.value].copy(), metric[:n], cnt


def _pixel_list(pixels):
    """the `pixels` argument of a call -> (uint32 array to keep alive, pointer -- None for an empty list --, count)"""
    p = np.ascontiguousarray(pixels, dtype=np.int64).reshape(-1)
    if len(p) and (p.min() < 0 or p.max() > 0xffffffff):
        raise DtofError("pixel list: indices must be flat indices y * width + x of the crop window")
    p = p.astype(np.uint32)
    return p, p.ctypes.data if len(p) else None, len(p)


AOV_TYPES = ("depth", "position", "uv", "geo_normal", "sh_normal", "dp_du", "dp_dv", "prim_index", "shape_index")   # the DTOF_AOV_* constants, in their order


_AOV_CHANNELS = (1, 3, 2, 3, 3, 3, 3, 1, 1)   # channels per type


def _aov_parse(spec):
    """dtof_aov_parse -> (types int32 array, channel names)"""
    text = str(spec).encode()
    nt, nc = C.c_int(0), C.c_int(0)
    _check(_abi._lib().dtof_aov_parse(text, None, 0, C.byref(nt), None, 0, C.byref(nc)))
    types = np.zeros(max(nt.value, 1), np.int32)
    buf = C.create_string_buffer(len(text) * 3 + 16 * max(nc.value, 1))      # a channel name is its token's name and a two-character suffix
    _check(_abi._lib().dtof_aov_parse(text, types.ctypes.data, nt.value, C.byref(nt), buf, len(buf), C.byref(nc)))
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
    _check(_abi._lib().dtof_velocity_map_variants(o.ctypes.data, len(o), out.ctypes.data))
    return out


MAX_DEPTH_FREQUENCIES = 4   # modulation frequencies one depth map combines (kMaxDepthFrequencies)
DEPTH_OUTPUTS = ("depth", "residual", "wraps", "amplitude", "phase", "tof")


def depth_map_variants(frequencies):
    """The (hetero_frequency, hetero_offset, w_g_mhz) films of a depth map in the order they are rendered (dtof_depth_map_variants): frequency j contributes (0, 0, f_j)
    and (0, 0.25, f_j), two frequencies share one traversal -> (2 * len(frequencies), 3) float32"""
    f = np.ascontiguousarray(frequencies, dtype=np.float32).reshape(-1)
    var, freq = np.zeros((2 * len(f), 2), np.float32), np.zeros(2 * len(f), np.float32)
    _check(_abi._lib().dtof_depth_map_variants(f.ctypes.data, len(f), var.ctypes.data, freq.ctypes.data))
    return np.concatenate([var, freq[:, None]], axis=1)


def default_max_path_length(frequencies):
    """300 / gcd of the frequencies (metres of path): the unambiguous range of whole-MHz frequencies; anything else has to say its own"""
    f = [float(np.float32(x)) for x in frequencies]
    if not f or any(x != int(x) or x <= 0 for x in f):
        raise DtofError("max_path_length is required unless every frequency is a whole number of MHz")
    return 300.0 / math.gcd(*[int(x) for x in f])


def _lane_dict(out, **more):
    """the dict of the lane dumps from their (n, 12) records; `more`: the call's further arrays (an `rgb` of its own replaces the records')"""
    return {"sample_pos": out[:, 0:2], "time": out[:, 2], "ray_o": out[:, 3:6], "ray_d": out[:, 6:9], "rgb": out[:, 9:12], **more}


def _stats(entry, *args):
    """call an entry whose last argument is the dtof_render_stats it fills -> the stats as a dict"""
    st = _Stats()
    _check(entry(*args, C.byref(st)))
    return st.as_dict()


class Scene:
    """A loaded scene.xml (Scene + Sensor + Film + the integrator/sampler declared in it)."""

    def __init__(self, handle):
        self._h = handle
        self.last_stats = None
        self._film_layout = (0, 0)

    def __del__(self):
        _release(self, "dtof_scene_destroy")

    def _timed(self, entry, *args):
        """call an entry whose last argument is the dtof_render_stats it fills -> last_stats"""
        self.last_stats = _stats(entry, *args)
        return self.last_stats

    def _grouped(self, name, seed, spp, var, images, *films, freq=None):
        """dtof_render_variants / _f64 over the variants `var` (None: the integrator's own pair), MAX_VARIANTS of them per traversal, into `images`, one per variant;
        last_stats sums the traversals.  `freq`: the variants' own w_g (MHz), which takes the call through dtof_render_variants_freq / _freq_f64"""
        total = None
        for g in range(0, len(images), MAX_VARIANTS):
            group = None if var is None else var[g:g + MAX_VARIANTS]
            n = 0 if group is None else len(group)
            tail = (images[g:g + MAX_VARIANTS].ctypes.data,) + films
            if freq is None:
                d = _stats(getattr(_abi._lib(), name), self._h, seed, spp, _ptr(group), n, *tail)
            else:
                d = _stats(getattr(_abi._lib(), name.replace("variants", "variants_freq")), self._h, seed, spp, _ptr(group), freq[g:g + MAX_VARIANTS].ctypes.data, n, *tail)
            total = d if total is None else {key: total[key] + d[key] for key in d}
        self.last_stats = total

    def info(self):
        i = _Info()
        _check(_abi._lib().dtof_scene_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    @property
    def size(self):
        i = self.info()
        return i["crop_width"], i["crop_height"]

    def export(self, kind):
        n = C.c_size_t(0)
        _check(_abi._lib().dtof_scene_export(self._h, kind, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        _check(_abi._lib().dtof_scene_export(self._h, kind, out.ctypes.data, out.size, C.byref(n)))
        return out

    def world_to_pixel(self):
        """S (3, 4) float64, world to FILM pixel (dtof_scene_world_to_pixel): pix(P) = (S[0] . (P, 1), S[1] . (P, 1)) / (S[2] . (P, 1)) in the coordinates of a
        lane's sample_pos.  Two of them make the flow of static geometry under a moving camera: harness.camera_flow."""
        out = np.zeros((3, 4), np.float64)
        _check(_abi._lib().dtof_scene_world_to_pixel(self._h, out.ctypes.data))
        return out

    @property
    def plan_facts_launches(self):
        """first-bounce launches since the scene was loaded that ran a kernel compiled with the frame plan's constants (lane dumps included)"""
        return int(_abi._lib().dtof_scene_plan_facts_launches(self._h))

    @property
    def last_plan_kernel(self):
        """the FACTS template argument of the first-bounce kernel compiled with the frame plan's constants that the last frame launched, 0 if it launched none:
        what dtof_scene_last_plan_facts reports, every bit of it"""
        return int(_abi._lib().dtof_scene_last_plan_facts(self._h))

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
        L = _abi._lib()
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
        _check(_abi._lib().dtof_scene_set_integrator(self._h, *_plugin_args(props)))

    def set_sampler(self, props):
        _check(_abi._lib().dtof_scene_set_sampler(self._h, *_plugin_args(props)))

    def render(self, seed=0, spp=0, offsets=None, sensor=0, variants=None, film="float32"):
        """Developed image (H, W, 3) float32 -- (H, W, 4) for an rgba film; with `offsets` (list of hetero_offset values) -> (K, H, W, 3 | 4).
        `variants`: list of (hetero_frequency, hetero_offset) pairs -> (K, H, W, 3 | 4), image k that of an integrator carrying pair k; every four of them
        share one traversal (dtof_render_variants), last_stats then sums the traversals.  (hetero_frequency, hetero_offset, w_g_mhz) triples give every film its own
        illumination frequency as well (dtof_render_variants_freq); all pairs or all triples.
        film="float64": the same images from a film accumulated and developed in double (dtof_render_variants_f64); offsets are then variants at the integrator's
        own frequency, every four of them one traversal."""
        _either(offsets, variants)
        if _film64(film):
            if sensor != 0:
                raise DtofError("Scene::render(): sensor index %d is out of bounds!" % sensor)
            if offsets is not None:
                f = self.info()["hetero_frequency"]
                variants = [(f, float(o)) for o in np.ascontiguousarray(offsets, dtype=np.float32).reshape(-1)]
            images, _ = self._render_f64(seed, spp, variants, False)
            return images[0] if variants is None else images
        w, h = self.size
        ch = 4 if self.info()["has_alpha"] else 3
        if variants is not None:
            var, freq = _variant_freq(variants)
            out = np.zeros((len(var), h, w, ch), np.float32)
            self._grouped("dtof_render_variants", seed, spp, var, out, freq=freq)
        elif offsets is None:
            out = np.zeros((h, w, ch), np.float32)
            self._timed(_abi._lib().dtof_render, self._h, sensor, seed, spp, out.ctypes.data)
        else:
            off = np.ascontiguousarray(offsets, dtype=np.float32)
            out = np.zeros((len(off), h, w, ch), np.float32)
            self._timed(_abi._lib().dtof_render_offsets, self._h, seed, spp, off.ctypes.data, len(off), out.ctypes.data)
        return out

    def _render_f64(self, seed, spp, variants, want_films):
        """(images (K, H, W, 3 | 4), films (planes, H, W, 4) float64 or None) through dtof_render_variants_f64, four variants per traversal; None: the integrator's own pair"""
        w, h = self.size
        alpha = 1 if self.info()["has_alpha"] else 0
        var, freq = (None, None) if variants is None else _variant_freq(variants)
        k = 1 if var is None else len(var)
        if want_films and k > MAX_VARIANTS:
            raise DtofError("at most 4 modulation variants can be batched per traversal")
        images = np.zeros((k, h, w, 3 + alpha), np.float32)
        films = np.zeros((k + alpha, h, w, 4), np.float64) if want_films else None
        self._grouped("dtof_render_variants_f64", seed, spp, var, images, _ptr(films), freq=freq)
        return images, films

    def render_film64(self, seed=0, spp=0, variants=None):
        """One traversal into the float64 film (dtof_render_variants_f64) -> (images (K, H, W, 3 | 4) float32, films (K, H, W, 4) float64 -- one more plane, the alpha
        film, behind the K colour planes of an rgba scene).  The images are the films developed in double: (float) (RGB / (W == 0 ? 1 : W)).  `variants`: up to four
        (hetero_frequency, hetero_offset) pairs or (hetero_frequency, hetero_offset, w_g_mhz) triples; None: the integrator's own pair (K = 1)."""
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
        var, var_ptr, n_var, _ = _variant_args(variants, cell=True)
        k = max(n_var, 1)
        w, h = self.size
        planes = np.zeros((MOMENT_PLANES(k), h, w), np.float64)
        self._timed(_abi._lib().dtof_render_moments, self._h, int(seed), int(spp), int(n_passes), var_ptr, n_var, 0 if raw else 1, planes.ctypes.data)
        return _moment_dict(planes, k)

    def render_denoised(self, seed=0, spp=0, n_passes=1, variants=None, **denoiser_kw):
        """The images of render(variants=...) and their jointly denoised versions (Denoiser), guided by what the moment film and the aov film provide.  THREE
        renders with the same seeds seed, seed + 1, ...: render() for the images (the float32 mean of the passes), render_moments for the variance of every
        variant's luminance estimate -- (m2_Y - mean_Y^2) / (samples per pixel x passes), harness.moment_statistics -- and render_aovs("p:position,n:sh_normal") for
        the guides; then ONE Denoiser call over all variants, which therefore share their weights.  These are three traversals of the scene with numpy between the films and
        the denoiser, the host route; render_denoised_device is the device route: one traversal per pass, everything up to the result on the GPU.  `variants`: up to four (hetero_frequency, hetero_offset) pairs; None: the integrator's own pair.
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

    def _denoised_call(self, entry, head, k, tof, details, denoiser_kw):
        """dtof_render_denoised / dtof_render_velocity_map_denoised: `head` is the entry's arguments between the scene and `params` -> the dict of every array the
        call was asked for (details: the intermediate films as well) and "sigma_position" """
        kw = dict(levels=5, sigma_normal=0.1, sigma_position=None, sigma_luminance=4.0)
        unknown = set(denoiser_kw) - set(kw)
        if unknown:
            raise DtofError("unknown denoiser arguments %s; known: %s" % (sorted(unknown), ", ".join(kw)))
        kw.update(denoiser_kw)
        auto = kw["sigma_position"] is None
        prm = _DenoiseParams(int(kw["levels"]), float(kw["sigma_normal"]), 1.0 if auto else float(kw["sigma_position"]), float(kw["sigma_luminance"]))
        w, h = self.size
        arrays = {"denoised": np.zeros((k, h, w, 3), np.float64), "denoised_variance": np.zeros((k, h, w), np.float64),
                  "sum": np.zeros((k, h, w, 3), np.float32), "variance": np.zeros((k, h, w), np.float64), "sigma_position": np.zeros(1, np.float64)}
        if tof:
            arrays.update(denoised_map=np.zeros((h, w), np.float64), noisy_map=np.zeros((h, w), np.float64))
        if details or tof:
            arrays.update(colour=np.zeros((k, h, w, 3), np.float32))
        if details:
            arrays.update(moments=np.zeros((MOMENT_PLANES(k), h, w), np.float64), aovs=np.zeros((7, h, w), np.float64),
                          normal=np.zeros((h, w, 3), np.float32), position=np.zeros((h, w, 3), np.float32))
        out = _DenoisedOutputs(**{name: a.ctypes.data for name, a in arrays.items()})
        self._timed(entry, self._h, *head, C.byref(prm), 1 if auto else 0, C.byref(out))
        arrays["sigma_position"] = float(arrays["sigma_position"][0])
        return arrays

    def render_denoised_device(self, seed=0, spp=0, n_passes=1, variants=None, details=False, **denoiser_kw):
        """render_denoised from ONE traversal per pass, on the device until the result (dtof_render_denoised): every pass renders the float64 film, the moment film
        and the aov film of "p:position,n:sh_normal" from the same lanes; the pass mean, the variance, the guides, the automatic sigma_position, the denoiser and
        nothing else run behind them on the GPU, and only the results cross to the host.  Same arguments; `denoiser_kw`: levels, sigma_normal, sigma_position (None:
        1 % of the extent of the finite positions), sigma_luminance.  Returns the keys of render_denoised without "denoiser" and with "sigma_position", the one the
        denoiser ran with.  The images are those of the FLOAT64 film -- render(film="float64") of every pass, summed in float32 and divided by the passes -- where
        render_denoised reads the float32 film; "image" has three channels (an alpha plane is neither returned nor denoised).  details=True adds "sum" (K, H, W, 3)
        float32, "moments" and "aovs" (the raw planes of render_moments(raw=True) / render_aovs(raw=True), (P, H, W) and (7, H, W) float64) and the denoiser's arguments
        "colour", "normal", "position".  last_stats sums the passes: one traversal each."""
        if variants is not None and not 1 <= len(variants) <= MAX_VARIANTS:
            raise DtofError("between 1 and 4 modulation variants can be denoised jointly")
        if int(n_passes) < 1:
            raise DtofError("n_passes must be at least 1")
        var, var_ptr, n_var, _ = _variant_args(variants)
        r = self._denoised_call(_abi._lib().dtof_render_denoised, (int(seed), int(spp), int(n_passes), var_ptr, n_var), max(n_var, 1), False, details, denoiser_kw)
        image = r["sum"] / np.float32(n_passes)
        out = {"image": image, "denoised": r["denoised"], "variance": r["variance"], "denoised_variance": r["denoised_variance"], "sigma_position": r["sigma_position"]}
        if variants is None:
            out.update({name: out[name][0] for name in ("image", "denoised", "variance", "denoised_variance")})
        if details:
            out.update({name: r[name] for name in ("sum", "moments", "aovs", "colour", "normal", "position")})
        return out

    def render_velocity_map_denoised(self, n_passes, spp, offsets=(0.0, 0.25), exposure_time=0.0015, w_g=30, seed=0, details=False, **denoiser_kw):
        """harness.velocity_map_denoised from ONE traversal per pass, on the device until the result (dtof_render_velocity_map_denoised): the four films (0, o0),
        (0, o1), (1, o0), (1, o1) of the two `offsets`, the moment film and the aov film from the same lanes; the ToF planes, their variances, the guides, the denoiser
        and both maps on the GPU.  Passes of `spp` samples with seeds seed, seed + 1, ...  Returns (noisy map (H, W), denoised map (H, W)) float64 -- bit for bit
        calc_velocity_from_homo_heteros of the ToF planes and of the denoised planes left in `denoise_details`: "homodyne", "heterodyne" (float32 ToF images),
        "denoised_homodyne", "denoised_heterodyne", "variance", "denoised_variance", "sigma_position", and with details=True "sum", "moments", "aovs", "colour",
        "normal", "position" as render_denoised_device returns them.  The films are the FLOAT64 film's, as in render_velocity_map(film="float64")."""
        off = np.ascontiguousarray([float(o) for o in offsets], dtype=np.float32)
        if len(off) != 2:
            raise DtofError("a denoised velocity map takes two offsets: the four films of one traversal")
        if int(n_passes) < 1:
            raise DtofError("n_passes must be at least 1")
        r = self._denoised_call(_abi._lib().dtof_render_velocity_map_denoised, (int(seed), int(spp), int(n_passes), off.ctypes.data, float(exposure_time), float(w_g)),
                                4, True, details, denoiser_kw)
        tof, den = r["colour"][..., 0], r["denoised"][..., 0]
        self.denoise_details = {"homodyne": list(tof[:2]), "heterodyne": list(tof[2:]), "denoised_homodyne": list(den[:2]), "denoised_heterodyne": list(den[2:]),
                                "variance": r["variance"], "denoised_variance": r["denoised_variance"], "sigma_position": r["sigma_position"]}
        if details:
            self.denoise_details.update({name: r[name] for name in ("sum", "moments", "aovs", "colour", "normal", "position")}, denoised=r["denoised"])
        return r["noisy_map"], r["denoised_map"]

    @property
    def aovs(self):
        """the `aovs` string of a scene whose integrator is <integrator type="aov"> (dtof_scene_get_aovs), None for every other scene"""
        buf = C.create_string_buffer(1 << 16)
        _check(_abi._lib().dtof_scene_get_aovs(self._h, buf, len(buf)))
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
        self._timed(_abi._lib().dtof_render_aovs, self._h, int(seed), int(spp), int(n_passes), types.ctypes.data, len(types), 0 if raw else 1, planes.ctypes.data)
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
        _check(_abi._lib().dtof_sample_aov_lanes(self._h, seed, spp, types.ctypes.data, len(types), lane_begin, n, out.ctypes.data, values.ctypes.data))
        return _lane_dict(out, values=values, channels=names)

    def render_flow(self, seed=0, spp=0, n_passes=1, raw=False, weight=False):
        """The flow film (dtof_render_flow; include/dtof.h has the definition): the screen-space motion, in pixels over ONE shutter interval, of what the scene
        integrator's own camera rays hit, from the keyframes of the hit objects' <animation>; accumulated in double over `n_passes` passes with seeds seed,
        seed + 1, ... like render_aovs.  Returns (H, W, 2) float64, the weighted mean (raw=True: the undivided sums); weight=True: the tuple (flow, weight (H, W)).
        +0 where the rays leave the scene or meet static objects; NaN where a hit is not in front of the camera at both ends of the shutter.  It is what
        Denoiser(temporal=True) takes as `flow` when the frame interval is the exposure; scale it otherwise."""
        w, h = self.size
        planes = np.zeros((3, h, w), np.float64)
        self._timed(_abi._lib().dtof_render_flow, self._h, int(seed), int(spp), int(n_passes), 0 if raw else 1, planes.ctypes.data)
        flow = np.ascontiguousarray(np.moveaxis(planes[1:3], 0, -1))
        return (flow, planes[0].copy()) if weight else flow

    def sample_flow_lanes(self, seed, spp, lane_begin, n):
        """sample_lanes of a flow render (dtof_sample_flow_lanes): the dict of sample_lanes without `valid`, plus "flow" (n, 2) float32"""
        out, flow = np.zeros((n, 12), np.float32), np.zeros((n, 2), np.float32)
        _check(_abi._lib().dtof_sample_flow_lanes(self._h, seed, spp, lane_begin, n, out.ctypes.data, flow.ctypes.data))
        return _lane_dict(out, flow=flow)

    def set_film_layout(self, planes, plane_stride_floats=0):
        """Declare the caller's device film for render_rows / render_stripes (dtof_scene_set_film_layout): `planes` RGBW planes, `plane_stride_floats` apart (0 = dense
        H * W * 4).  An rgba scene needs n_offsets + 1 planes -- the alpha film lies behind the colour films -- and is refused until they are declared.  With more
        than one plane, a stride too small for the rows a call writes (its rows plus the filter's halo) is refused by that call."""
        _check(_abi._lib().dtof_scene_set_film_layout(self._h, int(planes), int(plane_stride_floats)))
        self._film_layout = (int(planes), int(plane_stride_floats))

    @property
    def film_layout(self):
        """(planes, plane_stride_floats) as last declared with set_film_layout; (0, 0) = nothing declared.  A helper that declares a layout of its own
        (distributed.render_sharded / render_striped) puts this one back."""
        return self._film_layout

    def film_planes(self, n_offsets=1):
        """RGBW planes the device-film calls write for `n_offsets` batched offsets: one more for the alpha film of an rgba scene"""
        return max(int(n_offsets), 1) + (1 if self.info()["has_alpha"] else 0)

    def render_rows(self, d_film_ptr, seed, spp, row_begin, row_end, offsets=None, variants=None):
        """Accumulate the undeveloped RGBW film of rows [row_begin,row_end) into a DEVICE buffer (int pointer) of film_planes() planes (set_film_layout for rgba scenes).
        `variants`: up to four (hetero_frequency, hetero_offset) pairs instead of `offsets`, plane k = pair k (dtof_render_rows_variants)."""
        keep, ptr, n, is_var = _variant_args(variants, offsets)
        return self._timed(_abi._lib().dtof_render_rows_variants if is_var else _abi._lib().dtof_render_rows, self._h, seed, spp, row_begin, row_end, ptr, n, d_film_ptr)

    def render_rows_f64(self, d_film_ptr, seed, spp, row_begin, row_end, variants=None, planes=None, plane_stride_doubles=0):
        """render_rows into a float64 DEVICE film (dtof_render_rows_variants_f64): `planes` RGBW planes of doubles (default: film_planes() of the call), `plane_stride_doubles`
        apart (0 = dense H * W * 4).  The layout belongs to the call: set_film_layout is neither read nor changed."""
        keep, ptr, n, _ = _variant_args(variants)
        planes = self.film_planes(n) if planes is None else int(planes)
        return self._timed(_abi._lib().dtof_render_rows_variants_f64, self._h, seed, spp, row_begin, row_end, ptr, n, d_film_ptr, planes, int(plane_stride_doubles))

    def develop_f64_async(self, d_film_ptr, d_rgb_ptr, n_pixels, d_alpha_film_ptr=None):
        """enqueue the develop of one float64 film plane (dtof_develop_f64_async); with the alpha plane of an rgba film: rgba (dtof_develop_rgba_f64_async)"""
        if d_alpha_film_ptr is None:
            _check(_abi._lib().dtof_develop_f64_async(self._h, d_film_ptr, d_rgb_ptr, n_pixels))
        else:
            _check(_abi._lib().dtof_develop_rgba_f64_async(self._h, d_film_ptr, d_alpha_film_ptr, d_rgb_ptr, n_pixels))

    def render_rows_async(self, d_film_ptr, seed, spp, row_begin, row_end, offsets=None, variants=None):
        """enqueue one frame on the scene's stream without waiting for it (dtof_render_rows_async / _variants_async); collect() waits and returns the timings"""
        keep, ptr, n, is_var = _variant_args(variants, offsets)
        fn = _abi._lib().dtof_render_rows_variants_async if is_var else _abi._lib().dtof_render_rows_async
        _check(fn(self._h, seed, spp, row_begin, row_end, ptr, n, d_film_ptr))

    def clear_async(self, d_ptr, nbytes):
        _check(_abi._lib().dtof_clear_async(self._h, d_ptr, nbytes))

    def set_stream(self, stream_ptr):
        """enqueue on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream); 0 / None: back to the scene's own (dtof_scene_set_stream)"""
        _check(_abi._lib().dtof_scene_set_stream(self._h, C.c_void_p(stream_ptr or None)))

    def render_stripes_async(self, d_film_ptr, seed, spp, first_row, stripe_rows, stripe_period, offsets=None, variants=None):
        keep, ptr, n, is_var = _variant_args(variants, offsets)
        fn = _abi._lib().dtof_render_stripes_variants_async if is_var else _abi._lib().dtof_render_stripes_async
        _check(fn(self._h, seed, spp, first_row, stripe_rows, stripe_period, ptr, n, d_film_ptr))

    def develop_async(self, d_film_ptr, d_rgb_ptr, n_pixels):
        _check(_abi._lib().dtof_develop_async(self._h, d_film_ptr, d_rgb_ptr, n_pixels))

    def develop_accumulate_async(self, d_film_ptr, planes, d_rgb_sum_ptr, n_pixels, first, plane_stride_floats=0):
        """enqueue rgb / W of `planes` RGBW film planes into (first) or onto the dense float32 sum [planes][n_pixels][3] of a multi-pass render (dtof_develop_accumulate_async)"""
        _check(_abi._lib().dtof_develop_accumulate_async(self._h, d_film_ptr, int(planes), int(plane_stride_floats), d_rgb_sum_ptr, int(n_pixels), int(bool(first))))

    def velocity_map_async(self, d_rgb_sum_ptr, homodyne_planes, heterodyne_planes, n_passes, n_pixels, d_velocity_ptr, exposure_time=0.0015, w_g=30,
                           d_tof_ptr=None, d_velocity_pairs_ptr=None):
        """enqueue the velocity map of the sum of `n_passes` passes (dtof_velocity_map_async): pair k is planes (homodyne_planes[k], heterodyne_planes[k]) of the 2 * n_pairs
        planes of the sum; d_velocity [n_pixels] float64, optionally d_velocity_pairs [n_pairs][n_pixels] float64 and d_tof [2 * n_pairs][n_pixels] float32"""
        hom, het = np.ascontiguousarray(homodyne_planes, dtype=np.int32).reshape(-1), np.ascontiguousarray(heterodyne_planes, dtype=np.int32).reshape(-1)
        if len(hom) != len(het):
            raise DtofError("as many homodyne as heterodyne planes make the pairs")
        _check(_abi._lib().dtof_velocity_map_async(self._h, d_rgb_sum_ptr, len(hom), hom.ctypes.data, het.ctypes.data, int(n_passes), float(exposure_time), float(w_g),
                                              int(n_pixels), d_tof_ptr, d_velocity_pairs_ptr, d_velocity_ptr))

    def render_velocity_map(self, n_passes, spp, offsets=(0.0, 0.25), exposure_time=0.0015, w_g=30, pairs=False, film="float32"):
        """The radial-velocity map of `n_passes` passes (seeds 0 .. n_passes - 1) of `spp` samples, reconstructed on the device (dtof_render_velocity_map): every two
        offsets share one traversal per pass, their films never leave the GPU.  Returns (velocity (H, W) float64, {"homodyne": [...], "heterodyne": [...]} float32 ToF
        images in the order of `offsets`) and, with pairs=True, the maps of every offset alone (len(offsets), H, W) float64 -- the values numpy computes from the same
        films with harness.calc_velocity_from_homo_heteros / _hetero.  last_stats sums the traversals.  film="float64": every pass is splatted and developed in double
        (dtof_render_velocity_map_f64) -- the films numpy has to be given are then those of render(..., film="float64")."""
        entry = _abi._lib().dtof_render_velocity_map_f64 if _film64(film) else _abi._lib().dtof_render_velocity_map
        off = np.ascontiguousarray([float(o) for o in offsets], dtype=np.float32)
        n = len(off)
        w, h = self.size
        v, tof = np.zeros((h, w), np.float64), np.zeros((2 * n, h, w), np.float32)
        per_pair = np.zeros((n, h, w), np.float64) if pairs else None
        self._timed(entry, self._h, int(n_passes), int(spp), off.ctypes.data, n, float(exposure_time), float(w_g), v.ctypes.data, _ptr(per_pair), tof.ctypes.data)
        homo, hetero = [], []
        for g in range(0, n, 2):   # the planes of a group: its homodyne films, then its heterodyne films (velocity_map_variants)
            k = min(2, n - g)
            homo += [tof[2 * g + j] for j in range(k)]
            hetero += [tof[2 * g + k + j] for j in range(k)]
        films = {"homodyne": homo, "heterodyne": hetero}
        return (v, films, per_pair) if pairs else (v, films)

    def depth_map_async(self, d_rgb_sum_ptr, i_planes, q_planes, frequencies, n_passes, n_pixels, d_depth_ptr, exposure_time=0.0015, max_path_length=None,
                        d_residual_ptr=None, d_wraps_ptr=None, d_amplitude_ptr=None, d_phase_ptr=None):
        """enqueue the depth map of the sum of `n_passes` passes (dtof_depth_map_async): frequency j (MHz) has its I film in plane i_planes[j] and its Q film in plane
        q_planes[j] of the 2 * F planes of the sum; d_depth [n_pixels] float64, optionally d_residual [n_pixels] float64, d_wraps [F][n_pixels] int32,
        d_amplitude [F][n_pixels] float64 and d_phase [F][n_pixels] float32"""
        ip, qp = np.ascontiguousarray(i_planes, dtype=np.int32).reshape(-1), np.ascontiguousarray(q_planes, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(frequencies, dtype=np.float64).reshape(-1)
        if not len(ip) == len(qp) == len(f):
            raise DtofError("as many I planes and Q planes as frequencies")
        if max_path_length is None:
            max_path_length = default_max_path_length(f)
        _check(_abi._lib().dtof_depth_map_async(self._h, d_rgb_sum_ptr, len(f), ip.ctypes.data, qp.ctypes.data, f.ctypes.data, int(n_passes), float(exposure_time),
                                           float(max_path_length), int(n_pixels), d_depth_ptr, d_residual_ptr, d_wraps_ptr, d_amplitude_ptr, d_phase_ptr))

    def render_depth_map(self, n_passes, spp, frequencies=(30.0, 40.0), exposure_time=0.0015, max_path_length=None, film="float32", outputs=DEPTH_OUTPUTS):
        """The depth map of `n_passes` passes (seeds 0 .. n_passes - 1) of `spp` samples at the modulation `frequencies` (MHz), reconstructed on the device
        (dtof_render_depth_map): the I / Q films of two frequencies share one traversal per pass and never leave the GPU.  Returns a dict of the requested `outputs`:
        "depth" (H, W) float64 metres (half the unwrapped path length; always there), "residual" (H, W) float64, "wraps" (F, H, W) int32, "amplitude" (F, H, W) float64,
        "phase" (F, H, W) float32, "tof" (2 F, H, W) float32 in the order of depth_map_variants -- the values harness.calc_depth_from_homodynes computes from the same
        films.  max_path_length=None: 300 / gcd of whole-MHz frequencies.  film="float64": every pass is splatted and developed in double."""
        unknown = set(outputs) - set(DEPTH_OUTPUTS)
        if unknown:
            raise DtofError("unknown depth-map outputs %s; known: %s" % (sorted(unknown), ", ".join(DEPTH_OUTPUTS)))
        f = np.ascontiguousarray([float(x) for x in frequencies], dtype=np.float32)
        if max_path_length is None:
            max_path_length = default_max_path_length(f)
        n = len(f)
        w, h = self.size
        shapes = {"depth": ((h, w), np.float64), "residual": ((h, w), np.float64), "wraps": ((n, h, w), np.int32), "amplitude": ((n, h, w), np.float64),
                  "phase": ((n, h, w), np.float32), "tof": ((2 * n, h, w), np.float32)}
        out = {k: np.zeros(*shapes[k]) for k in DEPTH_OUTPUTS if k == "depth" or k in outputs}
        self._timed(_abi._lib().dtof_render_depth_map, self._h, int(n_passes), int(spp), f.ctypes.data, n, float(exposure_time), float(max_path_length),
                    int(_film64(film)), out["depth"].ctypes.data, *[_ptr(out.get(k)) for k in DEPTH_OUTPUTS[1:]])
        return out

    def collect(self, max_frames=4096):
        """wait for the frames enqueued by render_rows_async -> (summed stats dict, per-frame GPU milliseconds)"""
        st, ms, n = _Stats(), np.zeros(max_frames, np.float64), C.c_uint32(0)
        _check(_abi._lib().dtof_async_collect(self._h, C.byref(st), ms.ctypes.data, max_frames, C.byref(n)))
        return st.as_dict(), ms[:min(n.value, max_frames)].copy()

    def render_stripes(self, d_film_ptr, seed, spp, first_row, stripe_rows, stripe_period, offsets=None, variants=None):
        """Accumulate the rows of the stripes [first_row + k * stripe_period, ... + stripe_rows) (interleaved shard of one rank)."""
        keep, ptr, n, is_var = _variant_args(variants, offsets)
        return self._timed(_abi._lib().dtof_render_stripes_variants if is_var else _abi._lib().dtof_render_stripes, self._h, seed, spp, first_row, stripe_rows, stripe_period, ptr, n, d_film_ptr)

    def sample_lanes(self, seed, spp, lane_begin, n):
        out = np.zeros((n, 12), np.float32)
        valid = np.zeros(n, np.uint32)
        _check(_abi._lib().dtof_sample_lanes_valid(self._h, seed, spp, lane_begin, n, out.ctypes.data, valid.ctypes.data))
        return _lane_dict(out, valid=valid)

    def sample_lanes_variants(self, seed, spp, lane_begin, n, variants=None):
        """sample_lanes through the batched kernels (dtof_sample_lanes_variants): the lanes are evaluated once for up to four (hetero_frequency, hetero_offset)
        pairs; `rgb` is (K, n, 3), plane k the lanes' results with pair k, everything else is shared by the variants.  None: the integrator's own pair (K = 1).
        (hetero_frequency, hetero_offset, w_g_mhz) triples: film k at its own illumination frequency (dtof_sample_lanes_variants_freq)."""
        var, freq = (None, None) if variants is None else _variant_freq(variants)
        k = 0 if var is None else len(var)
        out, valid, rgb = np.zeros((n, 12), np.float32), np.zeros(n, np.uint32), np.zeros((max(k, 1), n, 3), np.float32)
        if freq is None:
            _check(_abi._lib().dtof_sample_lanes_variants(self._h, seed, spp, _ptr(var), k, lane_begin, n, out.ctypes.data, valid.ctypes.data, rgb.ctypes.data))
        else:
            _check(_abi._lib().dtof_sample_lanes_variants_freq(self._h, seed, spp, _ptr(var), freq.ctypes.data, k, lane_begin, n, out.ctypes.data, valid.ctypes.data,
                                                            rgb.ctypes.data))
        return _lane_dict(out, rgb=rgb, valid=valid)

    def sample_lanes_pixels(self, seed, spp, pixels, variants=None):
        """sample_lanes_variants of every lane of the listed pixels (dtof_sample_lanes_pixels): `pixels` strictly ascending flat indices y * width + x; record
        i * spp + j is global lane pixels[i] * spp + j of the dense render with this seed.  Same dict; `rgb` is (K, n, 3)."""
        var, var_ptr, n_var, _ = _variant_args(variants, cell=True)
        pix, pix_ptr, n_pix = _pixel_list(pixels)
        n, k = n_pix * (int(spp) if spp else self.info()["sample_count"]), max(n_var, 1)
        out, valid, rgb = np.zeros((max(n, 1), 12), np.float32), np.zeros(max(n, 1), np.uint32), np.zeros((k, max(n, 1), 3), np.float32)
        if n == 0:
            rgb = np.zeros((k, 0, 3), np.float32)
        _check(_abi._lib().dtof_sample_lanes_pixels(self._h, int(seed), int(spp), pix_ptr, n_pix, var_ptr, n_var, out.ctypes.data, valid.ctypes.data, rgb.ctypes.data))
        return _lane_dict(out[:n], rgb=rgb, valid=valid[:n])

    def render_pixels(self, pixels, seed=0, spp=0, variants=None, raw=False, films=False, moments=True):
        """ONE traversal of the listed pixels only (dtof_render_pixels) -- region-of-interest rendering: the lanes of a listed pixel are those of the dense render with
        this seed, so the full list gives the dense films.  Returns the dict of render_moments (raw=True: the undivided sums); with films=True also "film64"
        (K, H, W, 4) float64 raw R, G, B, W sums (one more plane, the alpha film, for an rgba scene); moments=False: the float64 film alone.  Pixels outside every
        listed footprint are 0."""
        var, var_ptr, n_var, _ = _variant_args(variants, cell=True)
        pix, pix_ptr, n_pix = _pixel_list(pixels)
        k = max(n_var, 1)
        w, h = self.size
        alpha = 1 if self.info()["has_alpha"] else 0
        planes = np.zeros((MOMENT_PLANES(k), h, w), np.float64) if moments else None
        film = np.zeros((k + alpha, h, w, 4), np.float64) if films else None
        self._timed(_abi._lib().dtof_render_pixels, self._h, int(seed), int(spp), pix_ptr, n_pix, var_ptr, n_var, 0 if raw else 1, _ptr(planes), _ptr(film))
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
        var, var_ptr, n_var, _ = _variant_args(variants, cell=True)
        k = max(n_var, 1)
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
        self._timed(_abi._lib().dtof_render_adaptive, self._h, int(seed), int(spp), base_passes, max_passes, var_ptr, n_var, C.byref(prm), 0 if raw else 1,
                    planes.ctypes.data, images.ctypes.data, _ptr(film), count.ctypes.data, metric.ctypes.data, pass_pixels.ctypes.data, C.byref(n_passes),
                    flat.ctypes.data if lists else None, cap)
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
        _check(_abi._lib().dtof_bsdf_eval_ex(self._h, shape_index, spec, len(q), q.ctypes.data, out.ctypes.data))
        return out

    def emitter_eval(self, mode, queries, level=-1, shape_index=-1):
        """The emitter side of a path vertex over arrays, through the shade kernels' own device functions (dtof_emitter_eval).  mode 0: (n, 5) reference point and the
        draws e1, e2 -> (n, 14) sampled point[3], direction[3], distance, density, delta, weight[3], usable, picked emitter; mode 1: (n, 11) previous vertex, hit point,
        shading normal, uv on shape `shape_index` -> (n, 5) distance, direction[3], density; mode 2: (n, 3) directions -> (n, 4) density and value of the environment.
        `level`: the (AREA, MESH, SPEC) instantiation (0 .. 6; -1 = the one a render of this scene runs).  Floats that are not finite and draws outside [0, 1) are refused."""
        n_in, n_out = {0: (5, 14), 1: (11, 5), 2: (3, 4)}[mode]
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, n_in)
        out = np.zeros((len(q), n_out), np.float32)
        _check(_abi._lib().dtof_emitter_eval(self._h, mode, level, shape_index, len(q), q.ctypes.data, out.ctypes.data))
        return out

    def camera_rays(self, samples):
        """Sensor::sample_ray over an (n, 4) array of (position sample x, y in [0, 1]^2 of the crop window, aperture sample x, y) -> (origins, directions, maxt)"""
        s = np.ascontiguousarray(samples, np.float32).reshape(-1, 4)
        out = np.zeros((len(s), 7), np.float32)
        _check(_abi._lib().dtof_camera_rays(self._h, len(s), s.ctypes.data, out.ctypes.data))
        return out[:, 0:3], out[:, 3:6], out[:, 6]

    def eval_modulation(self, mode, t, length=None):
        t = np.ascontiguousarray(t, np.float32)
        ln = np.ascontiguousarray(length, np.float32) if length is not None else None
        out = np.zeros_like(t)
        _check(_abi._lib().dtof_eval_modulation(self._h, mode, t.ctypes.data, ln.ctypes.data if ln is not None else None,
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
        _check(_abi._lib().dtof_ray_intersect_uv(self._h, len(rays), rays.ctypes.data, out.ctypes.data, ids.ctypes.data, uv.ctypes.data))
        return {"t": out[:, 0], "p": out[:, 1:4], "n": out[:, 4:7], "sh_n": out[:, 7:10], "sh_s": out[:, 10:13], "sh_t": out[:, 13:16],
                "wi": out[:, 16:19], "ids": ids, "uv": uv[:, 0:2], "prim_uv": uv[:, 2:4], "prim_index": ids[:, 2], "valid": ids[:, 0] >= 0}

    def ray_test(self, o, d, time=0.0, maxt=None):
        """Scene::ray_test over arrays of rays -> bool array (dtof_ray_test)"""
        rays = self._rays(o, d, time, maxt)
        occ = np.zeros(len(rays), np.int32)
        _check(_abi._lib().dtof_ray_test(self._h, len(rays), rays.ctypes.data, occ.ctypes.data))
        return occ != 0

    def _ray_query(self, name, rays8, any, key, forms=None, form=None):
        """the (n, 8) rays of a query entry, its call (`forms`: the entry takes a form, given by name or number) and its result: closest hit -> dict(t, u, v, `key`);
        any=True -> the int32 array of 1 / 0"""
        rays = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        lead = () if forms is None else (int(forms.get(form, form)),)
        out, ids = np.zeros((len(rays), 3), np.float32), np.zeros((len(rays), 3) if key == "ids" and not any else len(rays), np.int32)
        _check(getattr(_abi._lib(), name)(self._h, *lead, 1 if any else 0, len(rays), rays.ctypes.data, None if any else out.ctypes.data, ids.ctypes.data))
        return ids if any else {"t": out[:, 0], "u": out[:, 1], "v": out[:, 2], key: ids}

    FLAT_FORMS = {"generic": 0, "one_wall": 1, "shape": 2}

    def flat_query(self, rays8, form=0, any=False):
        """The ray query of a flat scene's fused kernels over an (n, 8) array of rays o, d, time, maxt (dtof_flat_query).  form: 0 / "generic", 1 / "one_wall",
        2 / "shape" -- the instantiation of trace_flat that runs.  Closest hit -> dict(t, u, v, obj) (inf, 0, 0, -1 on a miss); any=True -> int32 array of 1 / 0.
        A scene without a flat table, a form whose facts the scene does not meet and more than 2^24 rays raise DtofError; non-finite components are taken as they are."""
        return self._ray_query("dtof_flat_query", rays8, any, "obj", self.FLAT_FORMS, form)

    def flat_query_pairs(self, rays8, any=False):
        """flat_query in the pair form of the "shape" walk (dtof_flat_query_pairs), the one a frame's kernel runs where the two lanes of a correlated pair hold the same
        ray: rays 2k and 2k + 1 are equal in o, d and maxt, bit for bit, and have times of their own.  Same results as flat_query.  An odd count, a pair that differs
        and a table other than five rectangles with the wall at index 2 raise DtofError."""
        return self._ray_query("dtof_flat_query_pairs", rays8, any, "obj")

    def flat_query_zrow(self, rays8, any=False, zrows=False):
        """flat_query in the "shape" walk whose four plain rectangles take their z rows from the matrix cores (dtof_flat_query_zrow), the form a frame's kernel runs for a
        vertex's shadow and continuation rays.  Same results as flat_query.  zrows=True -> (result, (n, 8) float32): per ray the local z of the origin in rectangles
        0, 1, 3, 4, then that of the direction, as the MFMAs left them.  A table other than five rectangles with the wall at index 2 raises DtofError."""
        rays = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        out, ids, z = np.zeros((len(rays), 3), np.float32), np.zeros(len(rays), np.int32), np.zeros((len(rays), 8), np.float32)
        _check(_abi._lib().dtof_flat_query_zrow(self._h, 1 if any else 0, len(rays), rays.ctypes.data, None if any else out.ctypes.data, ids.ctypes.data, z.ctypes.data if zrows else None))
        r = ids if any else {"t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "obj": ids}
        return (r, z) if zrows else r

    def pair_setup_lanes(self, seed, spp, lane_begin, n, form=1):
        """Lane generation of the headline frame's kernel over lanes [lane_begin, lane_begin + n) (dtof_pair_setup_lanes), walked in 512-lane segments of 64-lane chunks
        as the first-bounce launch walks them.  form 0: every lane generates itself; form 1: what the two lanes of a correlated pair share is evaluated once per pair,
        for the pairs of two chunks at a time.  -> (n, 16) uint32: sample_pos[2], time, ray_o[3], ray_d[3], maxt as float bits, the path stream's state (low, high
        word), its selector, three zeros.  A scene or sample count the kernels are not compiled for, a lane_begin or n that is no multiple of 64 and n above 2^24
        raise DtofError before anything is launched."""
        out = np.zeros((int(n), 16), np.uint32)
        _check(_abi._lib().dtof_pair_setup_lanes(self._h, int(form), seed, spp, lane_begin, n, out.ctypes.data))
        return out

    TREE_FORMS = {"float": 0, "half_overflow": 1, "half_overflow_tlas_lds": 2, "defer_pair": 3, "half_every_shape": 4}

    def tree_query(self, rays8, form=0, any=False):
        """The TLAS / BLAS ray query over an (n, 8) array of rays o, d, time, maxt in the form a frame's ray kernels run it (dtof_tree_query).  form: 0 / "float",
        1 / "half_overflow", 2 / "half_overflow_tlas_lds", 3 / "defer_pair", 4 / "half_every_shape".  Closest hit -> dict(t, u, v, ids (n, 3): object, shape in its
        group, primitive) (inf, 0, 0, -1 on a miss); any=True -> int32 array of 1 / 0.  A form the scene does not meet and more than 2^24 rays raise DtofError;
        non-finite components are taken as they are."""
        return self._ray_query("dtof_tree_query", rays8, any, "ids", self.TREE_FORMS, form)

    FUSED_FORMS = {"classic": 0, "classic_rect": 1, "resident": 2, "resident_16": 3, "resident_half": 4, "resident_half_16": 5}

    def fused_query(self, rays8, form=0, waves=8, any=False):
        """The tree walk of the fused shade kernels over an (n, 8) array of rays o, d, time, maxt (dtof_fused_query), with the instance memo and the stack columns in
        those kernels' layout.  form: 0 / "classic", 1 / "classic_rect", 2 / "resident", 3 / "resident_16", 4 / "resident_half", 5 / "resident_half_16"; waves: 8, 12 or
        16 waves per block for the resident forms.  Results as tree_query.  A form the scene does not meet, another wave count and more than 2^24 rays raise DtofError."""
        rays = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        out, ids = np.zeros((len(rays), 3), np.float32), np.zeros(len(rays) if any else (len(rays), 3), np.int32)
        _check(_abi._lib().dtof_fused_query(self._h, int(self.FUSED_FORMS.get(form, form)), int(waves), 1 if any else 0, len(rays), rays.ctypes.data,
                                            None if any else out.ctypes.data, ids.ctypes.data))
        return ids if any else {"t": out[:, 0], "u": out[:, 1], "v": out[:, 2], "ids": ids}

    SURFACE_FORMS = {"mesh": 0, "rect": 1, "rect_memo_regs": 2, "rect_memo_lds": 3, "one_wall": 4, "mesh_memo_regs": 5}

    def surface_eval(self, in10, ids3, form=0, want_frame=True):
        """The surface-interaction fill over (n, 10) hits o, d, time, t, b1, b2 with (n, 3) ids object, shape in its group, primitive in the BLAS's order
        (dtof_surface_eval; triangle_order() maps faces).  form: 0 / "mesh", 1 / "rect", 2 / "rect_memo_regs", 3 / "rect_memo_lds", 4 / "one_wall",
        5 / "mesh_memo_regs" -- the instantiation of compute_surface that runs.  -> (n, 32) float32: p, n, sh_n, sh_s, sh_t, wi, uv, dp_du, dp_dv, offset_p(d),
        offset_p(-d).  A form the scene does not meet, an id out of range and more than 2^24 hits raise DtofError; non-finite floats are taken as they are."""
        q = np.ascontiguousarray(in10, np.float32).reshape(-1, 10)
        ids = np.ascontiguousarray(ids3, np.int32).reshape(-1, 3)
        if len(ids) != len(q):
            raise ValueError("surface_eval: %d hits and %d id rows" % (len(q), len(ids)))
        out = np.zeros((len(q), 32), np.float32)
        _check(_abi._lib().dtof_surface_eval(self._h, int(self.SURFACE_FORMS.get(form, form)), 1 if want_frame else 0, len(q), q.ctypes.data, ids.ctypes.data, out.ctypes.data))
        return out

    def triangle_order(self):
        """{(object, shape in its group): uint32 array, the face index of every triangle in the BLAS's order} for the mesh shapes (dtof_scene_export kind 27)"""
        w = self.export(27).view(np.uint32)
        out, at = {}, 0
        while at < len(w):
            obj, k, n = (int(x) for x in w[at:at + 3])
            out[(obj, k)] = w[at + 3:at + 3 + n].copy()
            at += 3 + n
        return out

    def cancel(self):
        _abi._lib().dtof_cancel(self._h)


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
    _check(_abi._lib().dtof_eval_component(comp, p.ctypes.data if p.size else None, p.size, x.ctypes.data, x.shape[1], out.ctypes.data, n_out, len(x)))
    return out
