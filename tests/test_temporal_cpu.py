"""The denoiser's temporal stage (dtof_denoise_temporal_async, dtof_denoise_temporal, mi.Denoiser(temporal=True)) as far as it can be held without a GPU:
  - tests/temporal_ref.py, the definition the kernel is held to bit for bit in test_temporal_gpu.py, checks itself: under zero flow, equal guides and
    alpha_min = 2^-20, N frames of equal variance v give the running mean, the variance v / N and the length N; an integer flow gives the exactly shifted history;
    scaling by a power of two is exact; invalid pixels pass through with length 0 and hand on no history
  - the header declares and the library exports the entries; every refusal comes back as DTOF_ERR_INVALID without a device and leaves sentinel-filled outputs alone
    (through the library, and shape by shape through tests/temporal_args_check.cpp, a host program over csrc/dtof_temporal_args.h with its own main -- the program
    to build with -fsanitize=address,undefined if a sanitizer pass over the checks is wanted); what passes them fails with DTOF_ERR_HIP on a host without a device
  - Denoiser's argument handling in temporal mode."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_ref as T  # noqa: E402

WALL = os.path.join(SCENES, "cornell_wall.xml")
INVALID, HIP = 1, 2
BUFFERS = ("colour", "variance", "normal", "ids", "flow", "h_colour", "h_variance", "h_normal", "h_ids", "h_length", "o_colour", "o_variance", "o_length", "o_colour_f32")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def history_of(out, normal=None, ids=None):
    return {"colour": out["colour"], "variance": out["variance"], "length": out["length"], "normal": normal, "ids": ids}


# ---------------------------------------------------------------------------- the reference checks itself
def test_static_frames_give_the_running_mean():
    """alpha = 1 / n while 1 / n > alpha_min: mean_n = (1 - 1/n) mean_(n-1) + x_n / n and var_n = (1 - 1/n)^2 var_(n-1) + v / n^2 = v / n"""
    rng = np.random.default_rng(1)
    k, h, w, frames, v = 2, 6, 7, 12, 0.75
    normal = np.broadcast_to(np.array([0.0, 0.6, 0.8], np.float32), (h, w, 3)).copy()
    ids = np.full((h, w), 3, np.float32)
    flow = np.zeros((h, w, 2), np.float32)
    history, images = None, []
    for n in range(1, frames + 1):
        images.append(rng.standard_normal((k, h, w, 3)).astype(np.float32))
        out = T.temporal(images[-1], flow, np.full((k, h, w), v), normal, ids, history, alpha_min=2.0 ** -20, max_length=64.0)
        history = history_of(out, normal, ids)
        assert (out["length"] == n).all()
        assert (out["accepted"] == (1 if n > 1 else 0)).all()      # zero flow: the one tap of weight 1
        mean = np.mean(np.array(images, dtype=np.float64), axis=0)
        assert np.allclose(out["colour"], mean, rtol=0, atol=1e-14 * n)
        assert np.allclose(out["variance"], v / n, rtol=1e-14 * n, atol=0)
    # the clamp: at max_length the weight stays 1 / max_length
    out = T.temporal(images[0], flow, np.full((k, h, w), v), normal, ids, history, alpha_min=2.0 ** -20, max_length=4.0)
    assert (out["length"] == 4).all()
    assert (bits(out["colour"]) == bits(0.75 * history["colour"] + 0.25 * images[0].astype(np.float64))).all()
    # ... and alpha_min wins over 1 / n
    out = T.temporal(images[0], flow, np.full((k, h, w), v), normal, ids, history, alpha_min=0.5, max_length=64.0)
    assert (out["length"] == frames + 1).all()
    assert (bits(out["variance"]) == bits(0.25 * history["variance"] + 0.25 * v)).all()


@pytest.mark.parametrize("dx,dy", [(1, 0), (0, -2), (-3, 2), (7, 0), (0, 5)])
def test_an_integer_flow_gives_the_exactly_shifted_history(dx, dy):
    """flow (dx, dy): pixel (x, y) takes the history of (x - dx, y - dy) with the one weight 1; where that lies outside, the pixel starts anew"""
    rng = np.random.default_rng(7)
    k, h, w = 3, 5, 7
    colour = rng.standard_normal((k, h, w, 3)).astype(np.float32)
    variance = rng.uniform(0.1, 1.0, (k, h, w))
    hist = {"colour": rng.standard_normal((k, h, w, 3)), "variance": rng.uniform(0.1, 1.0, (k, h, w)), "length": rng.integers(1, 9, (h, w)).astype(np.float32)}
    flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = dx, dy
    out = T.temporal(colour, flow, variance, history=hist, alpha_min=2.0 ** -20, max_length=64.0)
    c64 = colour.astype(np.float64)
    for y in range(h):
        for x in range(w):
            sx, sy = x - dx, y - dy
            if 0 <= sx < w and 0 <= sy < h:
                n = float(hist["length"][sy, sx]) + 1.0
                alpha = 1.0 / n
                assert out["length"][y, x] == n and out["accepted"][y, x] == 1
                assert (bits(out["colour"][:, y, x]) == bits((1.0 - alpha) * hist["colour"][:, sy, sx] + alpha * c64[:, y, x])).all()
                assert (bits(out["variance"][:, y, x]) == bits(((1.0 - alpha) * (1.0 - alpha)) * hist["variance"][:, sy, sx] + (alpha * alpha) * variance[:, y, x])).all()
            else:
                assert out["length"][y, x] == 1 and out["accepted"][y, x] == 0
                assert (bits(out["colour"][:, y, x]) == bits(c64[:, y, x])).all() and (bits(out["variance"][:, y, x]) == bits(variance[:, y, x])).all()


def test_a_fractional_flow_is_the_bilinear_mean_and_rejected_taps_renormalise():
    h, w = 4, 4
    colour = np.zeros((1, h, w, 3), np.float32)
    hist = {"colour": np.arange(h * w * 3, dtype=np.float64).reshape(1, h, w, 3), "length": np.full((h, w), 3, np.float32), "ids": np.zeros((h, w), np.float32)}
    flow = np.zeros((h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = 0.25, 0.5
    ids = np.zeros((h, w), np.float32)
    out = T.temporal(colour, flow, ids=ids, history=hist, alpha_min=2.0 ** -20, max_length=64.0)
    hc = hist["colour"][0]
    want = 0.75 * (0.125 * hc[1, 0] + 0.375 * hc[1, 1] + 0.125 * hc[2, 0] + 0.375 * hc[2, 1])      # pixel (x 1, y 2): rx 0.75, ry 1.5; alpha 1 / 4
    assert np.allclose(out["colour"][0, 2, 1], want, rtol=1e-15) and out["accepted"][2, 1] == 4
    assert out["accepted"][0, 0] == 1 and out["accepted"][0, 1] == 2 and out["accepted"][1, 0] == 2      # taps outside the image are dropped
    hist["ids"][1, 0] = 9.0      # another surface: the tap is rejected and the other three renormalise
    out = T.temporal(colour, flow, ids=ids, history=hist, alpha_min=2.0 ** -20, max_length=64.0)
    want = 0.75 * ((0.375 * hc[1, 1] + 0.125 * hc[2, 0] + 0.375 * hc[2, 1]) / 0.875)
    assert np.allclose(out["colour"][0, 2, 1], want, rtol=1e-15) and out["accepted"][2, 1] == 3 and out["length"][2, 1] == 4


@pytest.mark.parametrize("scale", [2.0 ** -30, 2.0 ** 7, 2.0 ** 40])
def test_power_of_two_scaling_is_exact(scale):
    rng = np.random.default_rng(5)
    k, h, w = 4, 9, 11
    colour = rng.standard_normal((k, h, w, 3)).astype(np.float32)
    variance = rng.uniform(-0.1, 1.0, (k, h, w))
    normal = rng.standard_normal((h, w, 3)).astype(np.float32)
    ids = rng.integers(0, 2, (h, w)).astype(np.float32)
    hist = {"colour": rng.standard_normal((k, h, w, 3)), "variance": rng.uniform(0.0, 1.0, (k, h, w)), "length": rng.integers(0, 40, (h, w)).astype(np.float32),
            "normal": (normal + 0.1 * rng.standard_normal((h, w, 3))).astype(np.float32), "ids": rng.integers(0, 2, (h, w)).astype(np.float32)}
    flow = rng.uniform(-2, 2, (h, w, 2)).astype(np.float32)
    a = T.temporal(colour, flow, variance, normal, ids, hist)
    scaled = dict(hist, colour=hist["colour"] * scale, variance=hist["variance"] * scale * scale)
    b = T.temporal(colour * np.float32(scale), flow, variance * scale * scale, normal, ids, scaled)
    assert 0 < (a["accepted"] > 0).sum() < h * w
    assert (bits(b["colour"]) == bits(a["colour"] * scale)).all() and (bits(b["variance"]) == bits(a["variance"] * scale * scale)).all()
    assert np.array_equal(a["length"], b["length"])


def test_invalid_pixels_pass_through_and_hand_on_no_history():
    rng = np.random.default_rng(9)
    k, h, w = 2, 6, 6
    colour = rng.standard_normal((k, h, w, 3)).astype(np.float32)
    variance = rng.uniform(0.1, 1.0, (k, h, w))
    ids = np.zeros((h, w), np.float32)
    flow = np.zeros((h, w, 2), np.float32)
    colour[1, 2, 3, 0] = np.nan
    variance[0, 4, 1] = np.inf
    ids[0, 5] = -np.inf
    flow[3, 3] = (np.nan, 0.0)      # no usable motion: the pixel is valid but starts anew
    first = T.temporal(colour, flow, variance, ids=ids)
    assert sorted(zip(*np.nonzero(first["length"] == 0))) == [(0, 5), (2, 3), (4, 1)] and (first["length"] <= 1).all()
    assert (bits(first["colour"]) == bits(colour.astype(np.float64))).all() and (bits(first["variance"]) == bits(variance)).all()
    clean = rng.standard_normal((k, h, w, 3)).astype(np.float32)
    second = T.temporal(clean, flow, np.abs(variance.clip(0, 1)), ids=np.zeros((h, w), np.float32), history=history_of(first, ids=ids))
    # the three pixels whose history has length 0 (and non-finite words), and the one without a flow, start anew; every other pixel has two frames
    assert sorted(zip(*np.nonzero(second["length"] == 1))) == [(0, 5), (2, 3), (3, 3), (4, 1)] and (second["length"][second["length"] != 1] == 2).all()
    assert np.isfinite(second["colour"]).all() and np.isfinite(second["variance"]).all()


# ---------------------------------------------------------------------------- the C ABI without a device
def test_header_declares_and_library_exports_the_entries(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ("dtof_denoise_temporal_async", "dtof_denoise_temporal"):
        assert re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr), name
        assert hasattr(lib, name), name
    m = re.search(r"typedef struct \{([^}]*)\}\s*dtof_temporal_params;", hdr)
    assert m and [n for n in re.findall(r"double\s+(\w+);", m.group(1))] == [n for n, _ in mi._TemporalParams._fields_] == ["alpha_min", "max_length", "tau_normal"]
    m = re.search(r"typedef struct \{([^}]*)\}\s*dtof_temporal_buffers;", hdr)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    declared = [n for decl in re.findall(r"(?:const\s+)?(?:float|double)\s+([^;]*);", body) for n in re.findall(r"\*\s*(\w+)", decl)]
    assert declared == list(BUFFERS) == [n for n, _ in mi._TemporalBuffers._fields_]
    assert C.sizeof(mi._TemporalBuffers) == 14 * 8 and C.sizeof(mi._TemporalParams) == 24
    L = mi._lib()
    vp = C.c_void_p
    assert L.dtof_denoise_temporal_async.argtypes == [vp, vp, C.c_int, C.c_int32, C.c_int32, vp]
    assert L.dtof_denoise_temporal.argtypes == [vp, C.c_int, C.c_int32, C.c_int32, vp]
    # the kernel file is part of every build of the library
    mk = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNEL_SRCS :=.*\bdtof_temporal\b", mk, re.M)


def _arrays(k, h, w, sent):
    a = {"colour": np.ones((k, h, w, 3), np.float32), "variance": np.ones((k, h, w)), "normal": np.ones((h, w, 3), np.float32), "ids": np.ones((h, w), np.float32),
         "flow": np.zeros((h, w, 2), np.float32), "h_colour": np.ones((k, h, w, 3)), "h_variance": np.ones((k, h, w)), "h_normal": np.ones((h, w, 3), np.float32),
         "h_ids": np.ones((h, w), np.float32), "h_length": np.ones((h, w), np.float32), "o_colour": np.full((k, h, w, 3), sent), "o_variance": np.full((k, h, w), sent),
         "o_length": np.full((h, w), sent, np.float32), "o_colour_f32": np.full((k, h, w, 3), sent, np.float32)}
    assert tuple(a) == BUFFERS
    return a


def test_refusals_need_no_device_and_write_nothing(mi):
    L = mi._lib()
    sc = mi.load_file(WALL, resx=8, resy=8)
    k, h, w = 2, 5, 6
    SENT = -7.5e11
    arrays = _arrays(k, h, w, SENT)
    nan, inf = float("nan"), float("inf")
    NO_HISTORY = dict(h_colour=None, h_variance=None, h_normal=None, h_ids=None, h_length=None)

    def call(entry, k=k, w=w, h=h, prm=(0.2, 32.0, 0.25), buffers_null=False, **override):
        use = dict(arrays, **override)
        buf = mi._TemporalBuffers(*(None if use[n] is None else use[n].ctypes.data for n in BUFFERS))
        p = None if prm is None else C.byref(mi._TemporalParams(*prm))
        b = None if buffers_null else C.byref(buf)
        return L.dtof_denoise_temporal_async(sc._h, b, k, w, h, p) if entry == "async" else L.dtof_denoise_temporal(b, k, w, h, p)

    cases = {
        "0 planes": dict(k=0), "5 planes": dict(k=5), "width 0": dict(w=0), "height 0": dict(h=0), "negative height": dict(h=-1), "width 65536": dict(w=65536),
        "height 65536": dict(h=65536),
        "null buffers": dict(buffers_null=True), "null params": dict(prm=None), "null colour": dict(colour=None), "null flow": dict(flow=None),
        "null o_colour": dict(o_colour=None), "null o_length": dict(o_length=None),
        "history without h_colour": dict(h_colour=None), "history without h_length": dict(h_length=None), "history without h_variance": dict(h_variance=None),
        "history without h_normal": dict(h_normal=None), "history without h_ids": dict(h_ids=None), "h_length alone": dict(NO_HISTORY, h_length=arrays["h_length"]),
        "h_variance without variance": dict(variance=None, o_variance=None), "h_normal without normal": dict(normal=None), "h_ids without ids": dict(ids=None),
        "o_variance without variance": dict(variance=None, h_variance=None), "variance without o_variance": dict(o_variance=None),
        "misaligned flow": dict(flow=np.zeros(h * w * 8 + 2, np.uint8)[2:]), "misaligned o_colour": dict(o_colour=np.zeros(k * h * w * 24 + 4, np.uint8)[4:]),
        "o_colour is h_colour": dict(o_colour=arrays["h_colour"]), "o_length is h_length": dict(o_length=arrays["h_length"]),
        "o_variance is variance": dict(o_variance=arrays["variance"]), "o_colour_f32 is colour": dict(o_colour_f32=arrays["colour"]),
        "o_colour_f32 is o_length": dict(o_colour_f32=arrays["o_length"]),
        "alpha_min 0": dict(prm=(0.0, 32.0, 0.25)), "alpha_min above 1": dict(prm=(1.5, 32.0, 0.25)), "alpha_min nan": dict(prm=(nan, 32.0, 0.25)),
        "max_length below 1": dict(prm=(0.2, 0.5, 0.25)), "max_length inf": dict(prm=(0.2, inf, 0.25)), "max_length nan": dict(prm=(0.2, nan, 0.25)),
        "tau_normal 0": dict(prm=(0.2, 32.0, 0.0)), "tau_normal inf": dict(prm=(0.2, 32.0, inf)), "tau_normal nan": dict(prm=(0.2, 32.0, nan)),
        "tau_normal squared underflows": dict(prm=(0.2, 32.0, 1e-200)),
    }
    for entry in ("async", "host"):
        for name, kw in cases.items():
            assert call(entry, **kw) == INVALID, (entry, name, L.dtof_last_error())
            assert b"dtof_denoise_temporal" in L.dtof_last_error(), (entry, name)
        # an output that only shares its last bytes with an input
        big = np.ones(h * w * 2 + h * w, np.float32)
        assert call(entry, flow=big[:h * w * 2].reshape(h, w, 2), o_length=big[h * w * 2 - 1:h * w * 3 - 1].reshape(h, w)) == INVALID, entry
        assert b"overlaps" in L.dtof_last_error()
        assert (big == 1.0).all()
    buf = mi._TemporalBuffers(*(arrays[n].ctypes.data for n in BUFFERS))
    assert L.dtof_denoise_temporal_async(None, C.byref(buf), k, w, h, C.byref(mi._TemporalParams(0.2, 32.0, 0.25))) == INVALID
    for n in ("o_colour", "o_variance", "o_length", "o_colour_f32"):
        assert (arrays[n] == arrays[n].dtype.type(SENT)).all(), n      # no refused call wrote
    # tau_normal is read only when normals are present
    rc = call("host", normal=None, h_normal=None, prm=(0.2, 32.0, nan))
    assert rc in (0, HIP), L.dtof_last_error()


def test_every_refusal_shape_by_shape_on_the_host(tmp_path):
    """temporal_check itself (csrc/dtof_temporal_args.h), which both entries run before their first HIP call, driven by a host program with its own main: every
    argument shape once, every message held, and what a good call packs."""
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "temporal_args_check")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc"),
                           os.path.join(ROOT, "tests", "temporal_args_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(ln.split("|", 1) for ln in out.stdout.splitlines())
    planes, small, large, null = ("between 1 and 4 colour planes can be accumulated jointly", "width and height must be at least 1",
                                  "width and height must not exceed 65535", "null argument")
    partial, orphan = "the history must be all null or hold every buffer of the current frame's", "a history buffer needs the current frame's buffer"
    mis, over_in, over_out = "misaligned buffer", "an output buffer overlaps an input buffer", "two output buffers overlap"
    alpha, length, tau, tau2 = ("alpha_min must be in (0, 1]", "max_length must be finite and >= 1", "tau_normal must be finite and > 0",
                                "tau_normal squared must be a finite double > 0")
    want = {"all buffers": "", "first frame": "", "colour and flow alone": "", "tau_normal unread without normals": "", "largest extent": "",
            "alpha_min 1, max_length 1": "", "o_length begins behind flow": "",
            "0 planes": planes, "5 planes": planes, "width 0": small, "height 0": small, "negative width": small, "width 65536": large, "height 65536": large,
            "null colour": null, "null flow": null, "null o_colour": null, "null o_length": null, "null params": null,
            "history without h_colour": partial, "history without h_length": partial, "history without h_variance": partial, "history without h_normal": partial,
            "history without h_ids": partial, "h_length alone": partial,
            "h_variance without variance": orphan, "h_normal without normal": orphan, "h_ids without ids": orphan,
            "o_variance without variance": "an output variance needs an input variance", "variance without o_variance": "an input variance needs an output variance",
            "misaligned colour": mis, "misaligned variance": mis, "misaligned h_colour": mis, "misaligned o_colour": mis, "misaligned o_length": mis,
            "misaligned o_colour_f32": mis,
            "o_colour is h_colour": over_in, "o_length is h_length": over_in, "o_variance is variance": over_in, "o_colour_f32 is colour": over_in,
            "o_length begins in the last word of flow": over_in, "o_variance begins in the last word of o_colour": over_out, "o_colour_f32 is o_length": over_out,
            "alpha_min 0": alpha, "alpha_min negative": alpha, "alpha_min above 1": alpha, "alpha_min nan": alpha,
            "max_length below 1": length, "max_length inf": length, "max_length nan": length,
            "tau_normal 0": tau, "tau_normal negative": tau, "tau_normal inf": tau, "tau_normal nan": tau,
            "tau_normal squared underflows": tau2, "tau_normal squared overflows": tau2,
            "packed": "6 5 3 1 1 1 1 %.17g 32 %.17g" % (0.2, 0.3 * 0.3), "packed first": "6 5 3 1 0 0 0 %.17g 32 1" % 0.2}
    assert got == want
    # the entries ask this function and nothing else, before their first device call
    films = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "dtof_abi_films.hip")).read()
    body = films[films.index("int dtof_denoise_temporal_async("):films.index("int dtof_develop(const float *d_film")]
    assert body.count("temporal_args(b, n_planes, width, height, params)") == 2
    assert body.index("temporal_args(b,") < body.index("ensure_device(sc)") and "temporal_check(t," in films


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
class P(C.Structure):
    _fields_ = [("alpha_min", C.c_double), ("max_length", C.c_double), ("tau_normal", C.c_double)]
class B(C.Structure):
    _fields_ = [(n, vp) for n in sys.argv[3].split(",")]
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_denoise_temporal_async.argtypes = [vp, vp, C.c_int, C.c_int32, C.c_int32, vp]
L.dtof_denoise_temporal.argtypes = [vp, C.c_int, C.c_int32, C.c_int32, vp]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
n, k = 4 * 3, 2
f = lambda count, value=1.0: (C.c_float * count)(*([value] * count))
d = lambda count, value=1.0: (C.c_double * count)(*([value] * count))
keep = [f(k * n * 3), d(k * n), f(n * 3), f(n), f(n * 2, 0.0), d(k * n * 3), d(k * n), f(n * 3), f(n), f(n), d(k * n * 3, 7.0), d(k * n, 7.0), f(n, 7.0), f(k * n * 3, 7.0)]
full = B(*[C.addressof(a) for a in keep])
first = B(*[None if 5 <= i <= 9 or i in (1, 2, 3, 11, 13) else C.addressof(a) for i, a in enumerate(keep)])
p = P(0.2, 32.0, 0.25)
print(L.dtof_denoise_temporal_async(h, C.byref(full), k, 4, 3, C.byref(p)), L.dtof_denoise_temporal(C.byref(full), k, 4, 3, C.byref(p)),
      L.dtof_denoise_temporal(C.byref(first), k, 4, 3, C.byref(p)), int(all(x == 7.0 for a in keep[10:] for x in a)))
"""


def test_entries_fail_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), WALL, ",".join(BUFFERS)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP), str(HIP), str(HIP), "1"], r.stdout


# ---------------------------------------------------------------------------- the Python class
def test_denoiser_temporal_mode_checks_its_arguments(mi, monkeypatch):
    calls = []

    class FakeLib:
        """stands in for the library: records the calls and fills the outputs, so that the shapes and the order of the stages can be held without a device"""
        def dtof_denoise_temporal(self, buffers, k, w, h, prm):
            b = C.cast(buffers, C.POINTER(mi._TemporalBuffers)).contents
            p = C.cast(prm, C.POINTER(mi._TemporalParams)).contents
            calls.append(("temporal", k, w, h, {n: getattr(b, n) is not None for n in BUFFERS}, (p.alpha_min, p.max_length, p.tau_normal)))
            C.memset(b.o_colour_f32, 0, k * w * h * 12)
            return 0

        def dtof_denoise(self, colour, k, w, h, variance, normal, position, prm, out, out_var):
            calls.append(("spatial", k, w, h, variance is not None, normal is not None, position is not None))
            return 0

    monkeypatch.setattr(mi._abi, "_lib", lambda: FakeLib())
    w, h = 7, 5
    flow = np.zeros((h, w, 2))
    plain = mi.Denoiser((w, h), temporal=True)
    out, hist = plain(np.ones((h, w, 3)), flow=flow)
    assert out.shape == (h, w, 3) and sorted(hist) == ["colour", "ids", "length", "normals", "variance"]
    assert hist["colour"].shape == (1, h, w, 3) and hist["colour"].dtype == np.float64 and hist["length"].shape == (h, w) and hist["length"].dtype == np.float32
    assert hist["variance"] is None and hist["normals"] is None and hist["ids"] is None
    present = dict.fromkeys(BUFFERS, False)
    present.update(colour=True, flow=True, o_colour=True, o_length=True, o_colour_f32=True)
    assert calls == [("temporal", 1, w, h, present, (0.2, 32.0, 0.25)), ("spatial", 1, w, h, False, False, False)]
    out, hist = plain(np.ones((h, w, 3)), flow=flow, history=hist)
    assert calls[-2][4] == dict(present, h_colour=True, h_length=True)
    full = mi.Denoiser((w, h), normals=True, position=True, variance=True, temporal=True, ids=True, alpha_min=0.1, max_length=8, tau_normal=0.5, sigma_position=1.0)
    kw = dict(normals=np.ones((h, w, 3)), position=np.ones((h, w, 3)), variance=np.ones((3, h, w)), flow=flow, ids=np.zeros((h, w)))
    out, var, hist = full(np.ones((3, h, w, 3)), **kw)
    assert out.shape == (3, h, w, 3) and var.shape == (3, h, w) and hist["variance"].shape == (3, h, w) and hist["normals"].dtype == np.float32 and hist["ids"].shape == (h, w)
    assert calls[-2][5] == (0.1, 8.0, 0.5) and calls[-1] == ("spatial", 3, w, h, True, True, True)
    out, var, hist = full(np.ones((3, h, w, 3)), history=hist, **kw)
    assert all(calls[-2][4].values())
    n_calls = len(calls)
    for make, match in ((lambda: mi.Denoiser((w, h), ids=True), "temporal=True"), (lambda: mi.Denoiser((w, h), temporal=True, alpha_min=0.0), "alpha_min"),
                        (lambda: mi.Denoiser((w, h), temporal=True, max_length=0), "max_length"), (lambda: mi.Denoiser((w, h), temporal=True, tau_normal=-1), "tau_normal"),
                        (lambda: mi.Denoiser((w, h))(np.ones((h, w, 3)), flow=flow), "temporal=True"),
                        (lambda: plain(np.ones((h, w, 3))), "flow=True"), (lambda: plain(np.ones((h, w, 3)), flow=np.zeros((h, w, 3))), "flow must have the shape"),
                        (lambda: plain(np.ones((h, w, 3)), flow=flow, ids=np.zeros((h, w))), "ids=False"),
                        (lambda: full(np.ones((3, h, w, 3)), **dict(kw, ids=None)), "ids=True"),
                        (lambda: plain(np.ones((h, w, 3)), flow=flow, history=3), "history must be"),
                        (lambda: full(np.ones((3, h, w, 3)), history={"colour": hist["colour"], "length": hist["length"]}, **kw), 'no "variance"'),
                        (lambda: full(np.ones((2, h, w, 3)), history=hist, **dict(kw, variance=np.ones((2, h, w)))), '"colour" must have the shape')):
        with pytest.raises(mi.DtofError, match=match):
            make()
    assert len(calls) == n_calls      # a refused call never reaches the library
