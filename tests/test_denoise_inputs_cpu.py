"""The denoised renders on the device (dtof_denoise_inputs_async, dtof_render_denoised, dtof_render_velocity_map_denoised; Scene.render_denoised_device,
Scene.render_velocity_map_denoised) as far as they can be held without a GPU: the ABI table and the mirrored outputs structure against the header, every refusal
that needs no device (sentinel-filled outputs stay untouched), the command line, and tests/denoise_inputs_ref.py -- the numpy definition of the stage -- against the
expressions Scene.render_denoised and harness.velocity_map_denoised evaluate inline."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_inputs_ref as dref
import test_binding_abi_cpu as abi_checks
from conftest import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALL = os.path.join(SCENES, "cornell_wall.xml")
OK, INVALID = 0, 1
FAKE = 0x10000      # a non-null, aligned "device pointer": a refused call never dereferences or enqueues it
ENTRIES = {"dtof_denoise_inputs_async": 15, "dtof_render_denoised": 10, "dtof_render_velocity_map_denoised": 11}


# ---------------------------------------------------------------------------- the ABI
def test_the_table_declares_the_new_entries_with_the_headers_arities(mi):
    from mitsuba3dopplertof_amd import _abi
    protos = abi_checks.parse_prototypes(abi_checks.header_code())
    lib = C.CDLL(mi.lib_path())
    for name, arity in ENTRIES.items():
        assert name in _abi.SIGNATURES and name in protos and hasattr(lib, name), name
        restype, argtypes = _abi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == arity == len(protos[name][1]), name
        assert [abi_checks.ctypes_class(t) for t in argtypes] == protos[name][1], name
    assert protos["dtof_denoise_inputs_async"][1][6:10] == ["i64", "u32", "f64", "f64"]
    assert protos["dtof_render_velocity_map_denoised"][1][5:7] == ["f64", "f64"]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_the_outputs_structure_has_the_headers_layout(tmp_path):
    from mitsuba3dopplertof_amd import _abi
    code = abi_checks.header_code()
    body = re.search(r"typedef\s+struct\s+dtof_denoised_outputs\s*\{([^{}]*)\}\s*dtof_denoised_outputs\s*;", code).group(1)
    assert sum(len(stmt.split(",")) for stmt in body.split(";") if stmt.strip()) == len(_abi._DenoisedOutputs._fields_) == 12
    src = tmp_path / "outputs.c"
    src.write_text(abi_checks.struct_source(_abi._DenoisedOutputs, "dtof_denoised_outputs"))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "outputs.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------- refusals that need no device
class Outputs:
    """every output of dtof_denoised_outputs as a sentinel-filled host array"""
    SENT = 123.25

    def __init__(self, mi, k, h, w):
        from mitsuba3dopplertof_amd import _abi
        shapes = {"denoised": ((k, h, w, 3), np.float64), "denoised_map": ((h, w), np.float64), "sum": ((k, h, w, 3), np.float32),
                  "moments": ((mi.MOMENT_PLANES(k), h, w), np.float64), "aovs": ((7, h, w), np.float64), "colour": ((k, h, w, 3), np.float32),
                  "variance": ((k, h, w), np.float64), "normal": ((h, w, 3), np.float32), "position": ((h, w, 3), np.float32),
                  "denoised_variance": ((k, h, w), np.float64), "noisy_map": ((h, w), np.float64), "sigma_position": ((1,), np.float64)}
        self.arrays = {name: np.full(shape, self.SENT, dtype) for name, (shape, dtype) in shapes.items()}
        self.struct = _abi._DenoisedOutputs(**{name: a.ctypes.data for name, a in self.arrays.items()})

    def without(self, name):
        from mitsuba3dopplertof_amd import _abi
        return _abi._DenoisedOutputs(**{n: (None if n == name else a.ctypes.data) for n, a in self.arrays.items()})

    def untouched(self):
        return all((a == self.SENT).all() for a in self.arrays.values())


def test_refusals_that_need_no_device(mi):
    L = mi._lib()
    sc = mi.load_file(WALL, resx=8, resy=8)
    out = Outputs(mi, 4, 8, 8)
    st = mi._Stats()
    var5 = np.zeros((5, 2), np.float32)
    off = np.asarray([0.0, 0.25], np.float32)
    nan, inf = float("nan"), float("inf")
    P = mi._abi._DenoiseParams

    def image(scene=sc._h, n_passes=1, variants=var5.ctypes.data, n=4, params=P(5, 0.1, 1.0, 4.0), auto=0, outputs=out.struct):
        return L.dtof_render_denoised(scene, 3, 4, n_passes, variants, n, None if params is None else C.byref(params), auto, None if outputs is None else C.byref(outputs),
                                      C.byref(st))

    def vmap(scene=sc._h, n_passes=1, offsets=off.ctypes.data, T=0.0015, w_g=30.0, params=P(5, 0.1, 1.0, 4.0), auto=0, outputs=out.struct):
        return L.dtof_render_velocity_map_denoised(scene, 0, 4, n_passes, offsets, T, w_g, None if params is None else C.byref(params), auto,
                                                   None if outputs is None else C.byref(outputs), C.byref(st))

    cases = {"image null scene": (lambda: image(scene=None), b"null argument"), "image null params": (lambda: image(params=None), b"null argument"),
             "image null outputs": (lambda: image(outputs=None), b"null argument"),
             "image null denoised": (lambda: image(outputs=out.without("denoised")), b"null argument"),
             "image 0 passes": (lambda: image(n_passes=0), b"n_passes must be at least 1"),
             "image 5 variants": (lambda: image(n=5), b"between 0 and 4 modulation variants can be denoised jointly"),
             "image -1 variants": (lambda: image(n=-1), b"between 0 and 4 modulation variants can be denoised jointly"),
             "image variants without an array": (lambda: image(variants=None), b"null argument: n_variants > 0 without variants"),
             "map null scene": (lambda: vmap(scene=None), b"null argument"), "map null offsets": (lambda: vmap(offsets=None), b"null argument"),
             "map null params": (lambda: vmap(params=None), b"null argument"), "map null outputs": (lambda: vmap(outputs=None), b"null argument"),
             "map null denoised": (lambda: vmap(outputs=out.without("denoised")), b"null argument"),
             "map null denoised map": (lambda: vmap(outputs=out.without("denoised_map")), b"null argument"),
             "map 0 passes": (lambda: vmap(n_passes=0), b"n_passes must be at least 1")}
    for levels in (0, 7, -1):
        cases["image levels %d" % levels] = (lambda levels=levels: image(params=P(levels, 0.1, 1.0, 4.0)), b"dtof_denoise: levels must be between 1 and 6")
        cases["map levels %d" % levels] = (lambda levels=levels: vmap(params=P(levels, 0.1, 1.0, 4.0)), b"dtof_denoise: levels must be between 1 and 6")
    for bad in (0.0, -1.0, nan, inf):
        for call, who in ((image, "image"), (vmap, "map")):
            cases["%s sigma_normal %r" % (who, bad)] = (lambda bad=bad, call=call: call(params=P(5, bad, 1.0, 4.0)), b"dtof_denoise: sigma_normal must be finite and > 0")
            cases["%s sigma_position %r" % (who, bad)] = (lambda bad=bad, call=call: call(params=P(5, 0.1, bad, 4.0)), b"dtof_denoise: sigma_position must be finite and > 0")
            cases["%s sigma_luminance %r" % (who, bad)] = (lambda bad=bad, call=call: call(params=P(5, 0.1, 1.0, bad)), b"dtof_denoise: sigma_luminance must be finite and > 0")
        cases["map exposure_time %r" % bad] = (lambda bad=bad: vmap(T=bad), b"exposure_time must be finite and > 0")
        cases["map w_g_mhz %r" % bad] = (lambda bad=bad: vmap(w_g=bad), b"w_g_mhz must be finite and > 0")
    cases["image sigma_normal squared underflows"] = (lambda: image(params=P(5, 1e-200, 1.0, 4.0)), b"dtof_denoise: sigma_normal squared must be a finite double > 0")
    cases["map sigma_position squared overflows"] = (lambda: vmap(params=P(5, 0.1, 1e200, 4.0)), b"dtof_denoise: sigma_position squared must be a finite double > 0")
    for name, (call, message) in cases.items():
        assert call() == INVALID, (name, L.dtof_last_error())
        assert L.dtof_last_error() == message, (name, L.dtof_last_error())
    for plugin in ("path", "velocity"):      # variants under another integrator
        sc.set_integrator(dict(type=plugin))
        for call in (image, vmap):
            assert call() == INVALID, plugin
            assert L.dtof_last_error() == b"modulation offsets only apply to the dopplertofpath integrator", (plugin, L.dtof_last_error())
    assert out.untouched()      # no refused call wrote
    for wrapper, message in ((lambda: sc.render_denoised_device(variants=[(0, 0)] * 5), "between 1 and 4"), (lambda: sc.render_denoised_device(n_passes=0), "n_passes"),
                             (lambda: sc.render_denoised_device(radius=3), "unknown denoiser arguments"),
                             (lambda: sc.render_velocity_map_denoised(1, 4, offsets=(0.0, 0.25, 0.5)), "two offsets"),
                             (lambda: sc.render_velocity_map_denoised(0, 4), "n_passes")):
        with pytest.raises(mi.DtofError, match=message):
            wrapper()


def test_refusals_of_the_stage_entry(mi):
    L = mi._lib()
    sc = mi.load_file(WALL, resx=8, resy=8)
    nan, inf = float("nan"), float("inf")
    px = 64
    # distinct, far apart fake addresses: sum, moments, aovs | colour, variance, normal, position, extent
    base = dict(scene=sc._h, mode=dref.TOF, d_sum=FAKE, d_mom=2 * FAKE, d_aov=3 * FAKE, k=4, n=px, n_passes=1, n_samples=4.0, T=0.0015, d_col=4 * FAKE, d_var=5 * FAKE,
                d_nrm=6 * FAKE, d_pos=7 * FAKE, d_ext=8 * FAKE)

    def stage(**kw):
        a = dict(base, **kw)
        return L.dtof_denoise_inputs_async(a["scene"], a["mode"], a["d_sum"], a["d_mom"], a["d_aov"], a["k"], a["n"], a["n_passes"], a["n_samples"], a["T"], a["d_col"],
                                           a["d_var"], a["d_nrm"], a["d_pos"], a["d_ext"])

    cases = {"null scene": (dict(scene=None), b"null argument")}
    for name in ("d_sum", "d_mom", "d_aov", "d_col", "d_var", "d_nrm", "d_pos"):
        cases["null " + name] = ({name: None}, b"dtof_denoise_inputs: null argument")
    cases.update({"mode 2": (dict(mode=2), b"dtof_denoise_inputs: mode must be DTOF_DENOISE_INPUTS_IMAGE or DTOF_DENOISE_INPUTS_TOF"),
                  "mode -1": (dict(mode=-1), b"dtof_denoise_inputs: mode must be DTOF_DENOISE_INPUTS_IMAGE or DTOF_DENOISE_INPUTS_TOF"),
                  "0 planes": (dict(k=0), b"dtof_denoise_inputs: between 1 and 4 colour planes can be denoised jointly"),
                  "5 planes": (dict(k=5), b"dtof_denoise_inputs: between 1 and 4 colour planes can be denoised jointly"),
                  "0 passes": (dict(n_passes=0), b"dtof_denoise_inputs: n_passes must be at least 1"),
                  "negative pixels": (dict(n=-1), b"dtof_denoise_inputs: negative pixel count"),
                  "2^31 pixels": (dict(n=2 ** 31), b"dtof_denoise_inputs: too many pixels for one launch"),
                  "misaligned sum": (dict(d_sum=FAKE + 2), b"dtof_denoise_inputs: misaligned buffer"),
                  "misaligned moments": (dict(d_mom=2 * FAKE + 4), b"dtof_denoise_inputs: misaligned buffer"),
                  "misaligned aovs": (dict(d_aov=3 * FAKE + 4), b"dtof_denoise_inputs: misaligned buffer"),
                  "misaligned variance": (dict(d_var=5 * FAKE + 4), b"dtof_denoise_inputs: misaligned buffer"),
                  "misaligned position": (dict(d_pos=7 * FAKE + 1), b"dtof_denoise_inputs: misaligned buffer"),
                  "misaligned extent": (dict(d_ext=8 * FAKE + 2), b"dtof_denoise_inputs: misaligned buffer"),
                  "colour inside the sum": (dict(d_col=FAKE + 8), b"dtof_denoise_inputs: an output buffer overlaps an input buffer"),
                  "extent inside the aov cells": (dict(d_ext=3 * FAKE + 64), b"dtof_denoise_inputs: an output buffer overlaps an input buffer"),
                  "normal inside the position": (dict(d_nrm=7 * FAKE + 12), b"dtof_denoise_inputs: two output buffers overlap")})
    for bad in (0.0, -1.0, nan, inf):
        cases["n_samples %r" % bad] = (dict(n_samples=bad), b"dtof_denoise_inputs: n_samples must be finite and > 0")
        cases["exposure_time %r" % bad] = (dict(T=bad), b"dtof_denoise_inputs: exposure_time must be finite and > 0")
    cases["exposure_time squared underflows"] = (dict(T=1e-200), b"dtof_denoise_inputs: exposure_time squared must be a finite double > 0")
    for name, (kw, message) in cases.items():
        assert stage(**kw) == INVALID, (name, L.dtof_last_error())
        assert L.dtof_last_error() == message, (name, L.dtof_last_error())


# ---------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("argv,message", [
    (["--denoise-route", "device"], "belong to --denoise"),
    (["--denoise-route", "device", "--moments"], "belong to --denoise"),
    (["--denoise-route", "device", "--aovs", "d:depth"], "belong to --denoise"),
    (["--denoise-route", "device", "--stripes", "4"], "belong to --denoise"),
    (["--denoise-route", "device", "--film", "float64"], "belong to --denoise"),
    (["--denoise", "--denoise-route", "device", "--moments"], "--moments and --aovs write the films it is guided by"),
    (["--denoise", "--denoise-route", "device", "--aovs", "d:depth"], "--moments and --aovs write the films it is guided by"),
    (["--denoise", "--denoise-route", "device", "--stripes", "4"], "single-GPU"),
    (["--denoise", "--denoise-route", "device", "--film", "float64"], "do not combine it with --film float64"),
    (["--denoise", "--denoise-route", "gpu"], "invalid choice"),
])
def test_command_line_refusals_before_the_scene_is_loaded(argv, message, tmp_path):
    """the scene file does not exist: a refusal that came after loading it would report that instead"""
    from mitsuba3dopplertof_amd import __main__ as cli
    r = subprocess.run([os.sys.executable, "-m", "mitsuba3dopplertof_amd", str(tmp_path / "no_such_scene.xml")] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-1000:]
    args = cli.parser().parse_args([WALL, "--denoise", "--denoise-route", "device", "--velocity-map", "0,0.25"])
    assert args.denoise_route == "device" and cli.parser().parse_args([WALL, "--denoise"]).denoise_route == "host"


# ---------------------------------------------------------------------------- the stage's definition against the harness's own expressions
def random_films(rng, K, h, w, n_passes, special=True):
    """raw films of K variants with the pixels a render can leave: W == 0, a negative m2 - mean^2, NaN / Inf words"""
    n = h * w
    total = rng.normal(0.0, 1.0, (K, n, 3)).astype(np.float32) * np.float32(n_passes)
    P = 1 + 6 * K + K * (K - 1) // 2
    moments = rng.normal(0.0, 1.0, (P, n))
    moments[0] = rng.uniform(0.5, 40.0, n)
    for k in range(K):      # Y^2 sums mostly above the squared mean
        moments[1 + 6 * k + 4] = moments[1 + 6 * k + 1] ** 2 / moments[0] + rng.uniform(0.0, 3.0, n) * moments[0]
    aovs = rng.normal(0.0, 2.0, (7, n))
    aovs[0] = rng.uniform(0.5, 40.0, n)
    if special and n >= 8:
        moments[:, 1] = 0.0                                  # a pixel no sample reached
        aovs[:, 1] = 0.0
        moments[0, 2] = 0.0                                  # W == 0 under non-zero sums
        aovs[0, 3] = 0.0
        moments[1 + 4, 4] = 0.0                              # m2 = 0 < mean^2: a negative variance
        moments[1 + 1, 4] = 5.0
        moments[1 + 1, 5], moments[1 + 4, 6] = np.nan, np.inf
        aovs[2, 5], aovs[5, 6], aovs[0, 7] = np.nan, -np.inf, np.inf
        total[0, 5, 1], total[K - 1, 6, 2] = np.nan, np.inf
    return total, moments, aovs


def developed_dicts(mi, moments, aovs, K, h, w):
    """the dicts Scene.render_moments and Scene.render_aovs return for these raw planes: the develop of k_develop_moments in numpy, then the binding's own reshaping"""
    from mitsuba3dopplertof_amd import _scene
    with np.errstate(all="ignore"):
        dm = np.concatenate([moments[:1], moments[1:] / np.where(moments[0] == 0.0, 1.0, moments[0])]).reshape(-1, h, w)
        da = np.concatenate([aovs[:1], aovs[1:] / np.where(aovs[0] == 0.0, 1.0, aovs[0])]).reshape(7, h, w)
    m = _scene._moment_dict(dm, K)
    g = {"p": np.ascontiguousarray(np.moveaxis(da[1:4], 0, -1)), "n": np.ascontiguousarray(np.moveaxis(da[4:7], 0, -1))}
    return m, g


@pytest.mark.parametrize("K,h,w,n_passes", [(4, 5, 7, 3), (1, 3, 3, 1), (2, 4, 4, 2)])
def test_reference_is_what_the_host_routes_compute_inline(mi, K, h, w, n_passes):
    from mitsuba3dopplertof_amd import harness, to_tof_image
    rng = np.random.default_rng(100 * K + n_passes)
    total, moments, aovs = random_films(rng, K, h, w, n_passes)
    if n_passes == 1:
        total[0, 0, 0] = np.float32(-0.0)      # x / 1.0f keeps the sign of a zero
    n_samples, T = 4.0 * n_passes, 0.0015
    m, g = developed_dicts(mi, moments, aovs, K, h, w)
    acc = total.reshape(K, h, w, 3)
    with np.errstate(all="ignore"):
        # Scene.render_denoised: image / np.float32(n_passes) for more than one pass; the variance; the guides through Denoiser._guide
        image = acc / np.float32(n_passes) if n_passes > 1 else acc
        variance_image = harness.moment_statistics(m, n_samples)["variance"][..., 1] / n_samples
        # harness.velocity_map_denoised
        tof = [to_tof_image(im, T) for im in acc / np.float32(n_passes)]
        films = np.stack(tof).astype(np.float32)
        colour_tof = np.repeat(films[..., None], 3, axis=3)
        variance_tof = harness.moment_statistics(m, n_samples)["variance"][..., 1] / n_samples * (T * T)
    normal, position = np.ascontiguousarray(g["n"], dtype=np.float32), np.ascontiguousarray(g["p"], dtype=np.float32)
    for mode, colour, variance in ((dref.IMAGE, image, variance_image), (dref.TOF, colour_tof, variance_tof)):
        c, v, nrm, pos = dref.inputs(mode, total, moments, aovs, n_passes, n_samples, T)
        assert dref.same_bits(c.reshape(K, h, w, 3), np.ascontiguousarray(colour, np.float32), nan_equal=True), mode
        assert dref.same_bits(v.reshape(K, h, w), variance, nan_equal=True), mode
        assert dref.same_bits(nrm.reshape(h, w, 3), normal, nan_equal=True) and dref.same_bits(pos.reshape(h, w, 3), position, nan_equal=True), mode
        assert (v[0, 4] < 0) and np.isnan(v[0, 5]) and not np.isfinite(pos.reshape(-1, 3)[5:8]).all(), "the special pixels are there"
    if n_passes == 1:
        assert np.signbit(dref.inputs(dref.IMAGE, total, moments, aovs, 1, n_samples)[0][0, 0, 0])
    # the automatic sigma_position: Denoiser.__call__'s lines, on this position plane and on the degenerate ones
    den = mi.Denoiser((w, h), position=True)
    for plane in (position, np.full((h, w, 3), np.nan, np.float32), np.where(np.arange(h * w).reshape(h, w, 1) == 2, np.float32(1.5), np.float32(np.inf)).repeat(3, axis=2)):
        pos = plane
        finite = pos[np.isfinite(pos).all(axis=2)].astype(np.float64)
        extent = float((finite.max(axis=0) - finite.min(axis=0)).max()) if len(finite) else 0.0
        want = 0.01 * extent if extent > 0 else 1.0
        assert dref.sigma_position(plane) == want
        lo, hi, count = dref.extent_words(plane)
        assert count == len(finite) and (count == 0 or ((lo == finite.min(axis=0)).all() and (hi == finite.max(axis=0)).all()))
    assert dref.sigma_position(np.full((2, 2, 3), np.nan, np.float32)) == 1.0 and den.sigma_position is None


def test_sanitizer_run_of_the_argument_checks():
    """tools/sanitize_denoise_inputs_args.sh: the argument-check header under -fsanitize=address,undefined in a stand-alone program (no GPU, no Python in it)"""
    cxx = os.environ.get("CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx) and shutil.which(cxx) is None:
        pytest.skip("no clang++ for the sanitizer build")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize_denoise_inputs_args.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert re.search(r"ok accepted \d+ refused \d+ failures 0", r.stdout), r.stdout
