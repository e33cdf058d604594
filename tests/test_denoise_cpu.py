"""The denoiser (dtof_denoise_async, dtof_denoise, mi.Denoiser, Scene.render_denoised, --denoise) as far as it can be held without a GPU:
  - tests/denoise_ref.py, the definition the kernel is held to in test_denoise_gpu.py, checks itself: a constant image is a fixed point bit for bit, one level without
    guides is the separable B3 convolution renormalised over the taps inside the image, scaling colour by a power of two c and variance by c^2 scales the output by
    exactly c and c^2, invalid pixels pass through and poison no neighbour
  - the header declares and the library exports the entries; every refusal comes back as DTOF_ERR_INVALID without a device and leaves sentinel-filled outputs alone;
    what passes them fails with DTOF_ERR_HIP on a host without a device (there is no CPU fallback)
  - Denoiser's shape, dtype and argument handling, and the command line's refusals."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as R  # noqa: E402

WALL = os.path.join(SCENES, "cornell_wall.xml")
INVALID, HIP = 1, 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_inputs(rng, k, h, w):
    colour = (rng.standard_normal((k, h, w, 3)) * 10.0 ** rng.uniform(-6, 2, (k, h, w, 1))).astype(np.float32)
    variance = (colour.astype(np.float64) ** 2).mean(axis=3) * rng.uniform(0.01, 1.0, (k, h, w))
    normal = rng.standard_normal((h, w, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    position = rng.uniform(-1, 1, (h, w, 3)).astype(np.float32)
    return colour, variance, normal, position


# ---------------------------------------------------------------------------- the reference checks itself
def test_constant_image_is_a_fixed_point_bit_for_bit():
    k, h, w = 3, 11, 13
    colour = np.broadcast_to(np.array([[0.3, -1.7e-4, 512.0], [1e-6, 2.0, -3.0], [0.0, 0.0, 7.0]], np.float32)[:, None, None, :], (k, h, w, 3)).copy()
    variance = np.broadcast_to(np.array([0.25, 0.0, 1e-3])[:, None, None], (k, h, w)).copy()
    normal = np.broadcast_to(np.array([0.0, 0.6, 0.8], np.float32), (h, w, 3)).copy()
    position = np.broadcast_to(np.array([1.0, 2.0, 3.0], np.float32), (h, w, 3)).copy()
    out = R.denoise(colour, variance, normal, position, levels=6)
    # every weight is the dyadic b[i] b[j], so sum (w c) = c sum w exactly as long as the partial sums stay representable: they are multiples of c / 256
    assert (bits(out["colour"]) == bits(colour.astype(np.float64))).all()
    assert out["valid"].all()
    assert (out["variance"] <= variance).all() and (out["variance"][0] > 0).all()      # the variance of a weighted mean shrinks


def _b3_separable(img):
    """zero-padded separable convolution with B3 along both axes of (H, W, ...)"""
    b = np.array(R.B3)
    out = np.zeros_like(img)
    h, w = img.shape[:2]
    rows = np.zeros_like(img)
    for i in range(-2, 3):
        x0, x1 = max(0, -i), min(w, w - i)
        if x0 < x1:
            rows[:, x0:x1] += b[i + 2] * img[:, x0 + i:x1 + i]
    for j in range(-2, 3):
        y0, y1 = max(0, -j), min(h, h - j)
        if y0 < y1:
            out[y0:y1] += b[j + 2] * rows[y0 + j:y1 + j]
    return out


@pytest.mark.parametrize("h,w", [(1, 1), (2, 7), (9, 4), (12, 17)])
def test_one_level_without_guides_is_the_renormalised_b3_convolution(h, w):
    rng = np.random.default_rng(h * 100 + w)
    colour = rng.standard_normal((2, h, w, 3)).astype(np.float32)
    out = R.denoise(colour, levels=1)
    norm = _b3_separable(np.ones((h, w)))
    for k in range(2):
        expected = _b3_separable(colour[k].astype(np.float64)) / norm[..., None]
        assert np.allclose(out["colour"][k], expected, rtol=1e-13, atol=1e-15)
    assert out["variance"] is None and out["envelope_variance"] == []
    assert (norm >= 9.0 / 64.0).all()


@pytest.mark.parametrize("scale", [2.0 ** -30, 2.0 ** 7, 2.0 ** 40])
def test_power_of_two_scaling_is_exact(scale):
    """no epsilon anywhere: the luminance term divides a difference of luminances by the standard deviation, so scaling both changes no weight by one bit"""
    rng = np.random.default_rng(5)
    colour, variance, normal, position = make_inputs(rng, 4, 10, 12)
    colour = (colour * np.float32(2.0 ** 20)).astype(np.float32) * np.float32(2.0 ** -20)      # stay clear of float32 denormals after scaling down
    variance[1, 2:5] = 0.0
    variance[2, 3, 3] = -1.0
    colour[1, 3, 4] = colour[1, 3, 5]      # equal luminance under a zero variance
    a = R.denoise(colour, variance, normal, position, levels=3, sigma_position=0.7)
    b = R.denoise(colour * np.float32(scale), variance * scale * scale, normal, position, levels=3, sigma_position=0.7)
    assert (bits(b["colour"]) == bits(a["colour"] * scale)).all()
    assert (bits(b["variance"]) == bits(a["variance"] * scale * scale)).all()


def test_invalid_pixels_pass_through_and_poison_no_neighbour():
    rng = np.random.default_rng(9)
    colour, variance, normal, position = make_inputs(rng, 2, 9, 9)
    colour[0, 4, 4, 1] = np.nan
    variance[1, 2, 6] = np.inf
    normal[6, 2, 0] = -np.inf
    position[0, 0, 2] = np.nan
    bad = [(4, 4), (2, 6), (6, 2), (0, 0)]
    out = R.denoise(colour, variance, normal, position, levels=4)
    assert sorted(zip(*np.nonzero(~out["valid"]))) == sorted(bad)
    c64 = colour.astype(np.float64)
    for y, x in bad:
        assert (bits(out["colour"][:, y, x]) == bits(c64[:, y, x])).all() and (bits(out["variance"][:, y, x]) == bits(variance[:, y, x])).all()
    assert np.isfinite(out["colour"][:, out["valid"]]).all() and np.isfinite(out["variance"][:, out["valid"]]).all()
    # the result is that of the image with ANY finite value in the invalid pixels' other words: they take part in nothing
    colour2, variance2 = colour.copy(), variance.copy()
    for y, x in bad:
        colour2[:, y, x] = np.where(np.isfinite(colour[:, y, x]), 99.0, colour[:, y, x])
        variance2[:, y, x] = np.where(np.isfinite(variance[:, y, x]), 5.0, variance[:, y, x])
    for y, x in bad:      # ... and whichever word made them invalid
        colour2[0, y, x, 0] = np.nan
    out2 = R.denoise(colour2, variance2, normal, position, levels=4)
    v = out["valid"]
    assert (bits(out2["colour"][:, v]) == bits(out["colour"][:, v])).all() and (bits(out2["variance"][:, v]) == bits(out["variance"][:, v])).all()


def test_envelope_bounds_the_result():
    rng = np.random.default_rng(3)
    colour, variance, normal, position = make_inputs(rng, 2, 8, 8)
    out = R.denoise(colour, variance, normal, position, levels=2)
    assert len(out["envelope_colour"]) == 2 and len(out["envelope_variance"]) == 2
    assert (np.abs(out["colour"]) <= out["envelope_colour"][-1] * (1 + 1e-12)).all()
    assert (np.abs(out["variance"]) <= out["envelope_variance"][-1] * (1 + 1e-12)).all()


# ---------------------------------------------------------------------------- the C ABI without a device
def test_header_declares_and_library_exports_the_entries(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ("dtof_denoise_async", "dtof_denoise"):
        assert re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr), name
        assert hasattr(lib, name), name
    m = re.search(r"typedef struct \{([^}]*)\}\s*dtof_denoise_params;", hdr)
    assert m and re.search(r"int32_t\s+levels;", m.group(1)) and re.search(r"double\s+sigma_normal,\s*sigma_position,\s*sigma_luminance;", m.group(1))
    assert C.sizeof(mi._DenoiseParams) == 32


def _params(mi, levels=3, sn=0.1, sx=1.0, sl=4.0):
    return mi._DenoiseParams(levels, sn, sx, sl)


def test_refusals_need_no_device_and_write_nothing(mi):
    L = mi._lib()
    sc = mi.load_file(WALL, resx=8, resy=8)
    k, h, w = 2, 5, 6
    SENT = -7.5e111
    colour = np.ones((k, h, w, 3), np.float32)
    variance, normal, position = np.ones((k, h, w)), np.ones((h, w, 3), np.float32), np.ones((h, w, 3), np.float32)
    out, out_var = np.full((k, h, w, 3), SENT), np.full((k, h, w), SENT)
    nan, inf = float("nan"), float("inf")

    def ptr(a):
        return None if a is None else a.ctypes.data

    def call(entry, colour=colour, k=k, w=w, h=h, variance=variance, normal=normal, position=position, prm=_params(mi), out=out, out_var=out_var):
        args = (ptr(colour), k, w, h, ptr(variance), ptr(normal), ptr(position), None if prm is None else C.byref(prm), ptr(out), ptr(out_var))
        return L.dtof_denoise_async(sc._h, *args) if entry == "async" else L.dtof_denoise(*args)

    cases = {
        "0 planes": dict(k=0), "5 planes": dict(k=5), "0 levels": dict(prm=_params(mi, levels=0)), "7 levels": dict(prm=_params(mi, levels=7)),
        "width 0": dict(w=0), "height 0": dict(h=0), "negative width": dict(w=-3),
        "sigma_normal 0": dict(prm=_params(mi, sn=0.0)), "sigma_normal nan": dict(prm=_params(mi, sn=nan)), "sigma_normal inf": dict(prm=_params(mi, sn=inf)),
        "sigma_position -1": dict(prm=_params(mi, sx=-1.0)), "sigma_position nan": dict(prm=_params(mi, sx=nan)),
        "sigma_luminance 0": dict(prm=_params(mi, sl=0.0)), "sigma_luminance inf": dict(prm=_params(mi, sl=inf)),
        "null colour": dict(colour=None), "null output": dict(out=None), "null params": dict(prm=None),
        "out_variance without variance": dict(variance=None),
        "output is the variance": dict(out_var=variance),
    }
    for entry in ("async", "host"):
        for name, kw in cases.items():
            assert call(entry, **kw) == INVALID, (entry, name, L.dtof_last_error())
            assert len(L.dtof_last_error()) > 0, (entry, name)
        # an output inside an input, and one that only shares its last bytes with it
        big = np.ones(k * h * w * 3 + 8, np.float64)
        inside = big[:k * h * w * 3].reshape(k, h, w, 3)
        tail_colour = big[k * h * w * 3 - 1:].view(np.float32)[:6].reshape(1, 1, 2, 3)
        assert call(entry, colour=big.view(np.float32)[:k * h * w * 3].reshape(k, h, w, 3), out=inside) == INVALID, entry
        assert b"overlaps" in L.dtof_last_error()
        assert call(entry, colour=tail_colour, k=1, h=1, w=2, variance=None, normal=None, position=None, out=big[k * h * w * 3 - 6:k * h * w * 3], out_var=None) == INVALID, entry
        assert (big == 1.0).all()
        assert call(entry, normal=out.view(np.float32).reshape(-1)[:h * w * 3].reshape(h, w, 3)) == INVALID, entry
    assert L.dtof_denoise_async(None, ptr(colour), k, w, h, ptr(variance), ptr(normal), ptr(position), C.byref(_params(mi)), ptr(out), ptr(out_var)) == INVALID
    assert (out == SENT).all() and (out_var == SENT).all()      # no refused call wrote
    # a sigma is read only when its guide is present
    rc = call("host", normal=None, position=None, prm=_params(mi, sn=nan, sx=-1.0))
    assert rc in (0, HIP), L.dtof_last_error()


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
class P(C.Structure):
    _fields_ = [("levels", C.c_int32), ("sn", C.c_double), ("sx", C.c_double), ("sl", C.c_double)]
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_denoise_async.argtypes = [vp, vp, C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
L.dtof_denoise.argtypes = [vp, C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
n = 4 * 3
colour, guide = (C.c_float * (2 * n * 3))(*([1.0] * (2 * n * 3))), (C.c_float * (n * 3))(*([1.0] * (n * 3)))
var = (C.c_double * (2 * n))(*([1.0] * (2 * n)))
out, out_var = (C.c_double * (2 * n * 3))(*([7.0] * (2 * n * 3))), (C.c_double * (2 * n))(*([7.0] * (2 * n)))
p = P(2, 0.1, 1.0, 4.0)
print(L.dtof_denoise_async(h, colour, 2, 4, 3, var, guide, guide, C.byref(p), out, out_var), L.dtof_denoise(colour, 2, 4, 3, var, guide, guide, C.byref(p), out, out_var),
      L.dtof_denoise(colour, 1, 4, 3, None, None, None, C.byref(p), out, None), int(all(x == 7.0 for x in list(out) + list(out_var))))
"""


def test_entries_fail_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), WALL], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP), str(HIP), str(HIP), "1"], r.stdout


# ---------------------------------------------------------------------------- the Python class
def test_denoiser_checks_shapes_and_arguments(mi, monkeypatch):
    calls = []

    class FakeLib:
        """stands in for the library: records the call and fills the outputs, so that the shapes and dtypes can be held without a device"""
        def dtof_denoise(self, colour, k, w, h, variance, normal, position, prm, out, out_var):
            p = C.cast(prm, C.POINTER(mi._DenoiseParams)).contents
            calls.append(dict(k=k, w=w, h=h, variance=variance, normal=normal, position=position, levels=p.levels, sigmas=(p.sigma_normal, p.sigma_position, p.sigma_luminance)))
            C.memset(out, 0, k * w * h * 3 * 8)
            return 0

    monkeypatch.setattr(mi._abi, "_lib", lambda: FakeLib())
    w, h = 7, 5
    d = mi.Denoiser((w, h))
    out = d(np.ones((h, w, 3), np.float64))      # any float type is taken and converted
    assert out.shape == (h, w, 3) and out.dtype == np.float64
    assert calls[-1] == dict(k=1, w=w, h=h, variance=None, normal=None, position=None, levels=5, sigmas=(0.1, 1.0, 4.0))
    out = d(np.ones((3, h, w, 3), np.float32))
    assert out.shape == (3, h, w, 3) and calls[-1]["k"] == 3
    full = mi.Denoiser((w, h), normals=True, position=True, variance=True, levels=2, sigma_normal=0.5, sigma_luminance=2.0)
    pos = np.zeros((h, w, 3), np.float32)
    pos[..., 0] = np.linspace(-2.0, 6.0, w)
    pos[:, 0] = np.nan      # not part of the extent
    out, var = full(np.ones((2, h, w, 3), np.float32), normals=np.ones((h, w, 3)), position=pos, variance=np.ones((2, h, w), np.float32))
    assert out.shape == (2, h, w, 3) and var.shape == (2, h, w) and var.dtype == np.float64
    assert calls[-1]["levels"] == 2 and calls[-1]["sigmas"] == (0.5, 0.01 * (float(pos[0, -1, 0]) - float(pos[0, 1, 0])), 2.0) and full.last_sigma_position == calls[-1]["sigmas"][1]
    out, var = full(np.ones((h, w, 3), np.float32), normals=np.ones((h, w, 3)), position=np.zeros((h, w, 3)), variance=np.ones((h, w)))
    assert out.shape == (h, w, 3) and var.shape == (h, w) and full.last_sigma_position == 1.0      # one point: no extent
    assert mi.Denoiser((w, h), position=True, sigma_position=0.25)(np.ones((h, w, 3)), position=pos).shape == (h, w, 3) and calls[-1]["sigmas"][1] == 0.25
    n_calls = len(calls)
    for make, match in ((lambda: mi.Denoiser((w,)), "input_size"), (lambda: mi.Denoiser((0, 4)), "at least 1 x 1"), (lambda: mi.Denoiser((w, h), levels=0), "levels"),
                        (lambda: mi.Denoiser((w, h), levels=7), "levels"),
                        (lambda: d(np.ones((h, w, 4))), "noisy must be"), (lambda: d(np.ones((w, h, 3))), "noisy must be"), (lambda: d(np.ones((5, h, w, 3))), "noisy must be"),
                        (lambda: d(np.ones((h, w, 3)), normals=np.ones((h, w, 3))), "normals=False"), (lambda: full(np.ones((h, w, 3))), "normals=True"),
                        (lambda: full(np.ones((2, h, w, 3)), normals=np.ones((h, w, 3)), position=pos, variance=np.ones((h, w))), "variance must have the shape"),
                        (lambda: full(np.ones((h, w, 3)), normals=np.ones((h, w, 2)), position=pos, variance=np.ones((h, w))), "normals must have the shape")):
        with pytest.raises(mi.DtofError, match=match):
            make()
    assert len(calls) == n_calls      # a refused call never reaches the library
    assert "Denoiser" in mi.__all__


def test_render_denoised_refuses_what_it_cannot_do_before_it_renders(mi):
    sc = mi.load_file(WALL, resx=8, resy=8)
    with pytest.raises(mi.DtofError, match="between 1 and 4"):
        sc.render_denoised(variants=[(0, 0)] * 5)
    with pytest.raises(mi.DtofError, match="n_passes"):
        sc.render_denoised(n_passes=0)
    from mitsuba3dopplertof_amd import harness
    with pytest.raises(ValueError, match="two offsets"):
        harness.run_scene_velocity_map_denoised(sc, 16, offsets=(0.0, 0.25, 0.5))


# ---------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("argv,message", [
    (["--denoise", "--moments"], "--moments and --aovs write the films it is guided by"),
    (["--denoise", "--aovs", "d:depth"], "--moments and --aovs write the films it is guided by"),
    (["--denoise", "--offsets", "0,0.25"], "not --offsets"),
    (["--denoise", "--film", "float64"], "float32 images"),
    (["--denoise", "--stripes", "4"], "single-GPU"),
    (["--denoise", "--denoise-levels", "7"], "between 1 and 6"),
    (["--denoise", "--denoise-sigma", "0.1,1"], "three comma separated numbers"),
    (["--denoise", "--denoise-sigma", "0.1,0,4"], "finite and > 0"),
    (["--denoise", "--velocity-map", "0,0.25,0.5"], "two offsets"),
    (["--denoise-levels", "3"], "belong to --denoise"),
    (["--denoise-sigma", "0.1,1,4"], "belong to --denoise"),
])
def test_command_line_refusals(argv, message):
    r = subprocess.run([sys.executable, "-m", "mitsuba3dopplertof_amd", WALL] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-1000:]


def test_command_line_parses_the_denoise_flags():
    from mitsuba3dopplertof_amd import __main__ as M
    ap = M.parser()
    args = ap.parse_args([WALL, "--denoise", "--denoise-levels", "3", "--denoise-sigma", "0.2,0.5,3", "--velocity-map", "0,0.25", "-o", "x.npy"])
    assert M.check_denoise_args(ap, args) == dict(levels=3, sigma_normal=0.2, sigma_position=0.5, sigma_luminance=3.0)
    assert M._noisy_sibling("a/b/out.npy") == "a/b/out_noisy.npy"
    assert M.check_denoise_args(ap, ap.parse_args([WALL, "--denoise"])) == {}
