"""The opt-in float64 film (dtof_render_variants_f64, dtof_render_rows_variants_f64, dtof_develop_f64_async, dtof_develop_rgba_f64_async,
dtof_render_velocity_map_f64) as far as it can be held without a GPU: the header declares the entries and the library exports them, refusals that need no device come
back as DTOF_ERR_INVALID and leave the outputs alone, what passes them fails with DTOF_ERR_HIP on a host without a device (there is no CPU fallback), film= takes the
two names only, and the command line parses --film; and the expected RGBW sums of the GPU test's signed-weight case against the oracle's exact film."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import SCENES
import moments_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, HIP = 0, 1, 2
ENTRIES = ("dtof_render_variants_f64", "dtof_render_rows_variants_f64", "dtof_develop_f64_async", "dtof_develop_rgba_f64_async", "dtof_render_velocity_map_f64")
FAKE = 0x1000      # a non-null, 16-byte aligned "device pointer": a refused call never dereferences or enqueues it


def test_header_declares_and_library_exports_the_entries(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert hasattr(lib, name), name
        # each entry cites what it replaces and says what differs
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert "imageblock.cpp:414-531" in comment and "hdrfilm.cpp:305-406" in comment and "accumulator type" in comment, name
    # the films cross the boundary as doubles, and the device film's layout is an argument of the call
    args = re.search(r"\bint\s+dtof_render_rows_variants_f64\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert re.search(r"double\s*\*\s*d_film", args) and re.search(r"int32_t\s+planes", args) and re.search(r"uint64_t\s+plane_stride_doubles", args)
    assert re.search(r"double\s*\*\s*out_films_or_null", re.search(r"\bint\s+dtof_render_variants_f64\s*\(([^;]*)\)\s*;", hdr).group(1))
    # the velocity map takes the arguments of the float32 entry
    flat = lambda name: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1))      # noqa: E731
    assert flat("dtof_render_velocity_map_f64") == flat("dtof_render_velocity_map")


def test_expected_rgbw_against_the_exact_oracle(orc):
    """what test_film64_gpu.py holds its signed-weight case to (moments_ref.expected_rgbw) is, on the tent case, the raw film of orc_render_exact within
    2^-40 * sum |term| per pixel: both add the same float32 terms in double, in different orders"""
    osc = orc.Scene(os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16))
    pd = osc.params()
    w, h = osc.size
    film = np.zeros((h, w, 4), np.float64)
    L = orc.lib()
    L.orc_render_exact.restype = C.c_uint64
    L.orc_render_exact.argtypes = [C.POINTER(orc.OrcScene), C.POINTER(orc.OrcParams), C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
    p = orc.make_params(pd)
    assert L.orc_render_exact(C.byref(osc.c), C.byref(p), 3, 16, 0, h, film.ctypes.data, None, ref.NCPU) == w * h * 16
    sums, mags = ref.expected_rgbw(orc, osc, pd, 3, 16)
    ratios = ref.errors_over_bound(sums, np.moveaxis(film, -1, 0), mags)
    print("expected_rgbw against orc_render_exact, largest error / bound: r %.3g g %.3g b %.3g w %.3g" % tuple(ratios))
    assert np.abs(film[..., :3]).max() > 0 and (film[..., 3] > 0).all()
    assert (ratios <= 1.0).all(), ratios


def _wall(mi, **kw):
    return mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), **dict(dict(resx=8, resy=8), **kw))


def test_refusals_that_need_no_device(mi):
    L = mi._lib()
    sc = _wall(mi)
    px = 64
    SENT = 123.25
    img, films = np.full((5, px, 3), SENT, np.float32), np.full((5, px, 4), SENT)
    var = np.asarray([(0, 0), (0, .25), (1, 0), (1, .25), (1, .5)], np.float32)
    off = np.asarray([0.0, 0.25] * 9, np.float32)
    v, pairs, tof = np.full(px, SENT), np.full((18, px), SENT), np.full((36, px), SENT, np.float32)
    st = mi._Stats()

    def host(scene=sc._h, variants=var.ctypes.data, n=4, out=img.ctypes.data, out_films=films.ctypes.data):
        return L.dtof_render_variants_f64(scene, 0, 4, variants, n, out, out_films, C.byref(st))

    def rows(scene=sc._h, variants=var.ctypes.data, n=4, film=FAKE, planes=4, stride=0, r0=0, r1=8):
        return L.dtof_render_rows_variants_f64(scene, 0, 4, r0, r1, variants, n, film, planes, stride, C.byref(st))

    def develop(scene=sc._h, film=FAKE, rgb=FAKE, n_px=px):
        return L.dtof_develop_f64_async(scene, film, rgb, n_px)

    def develop_rgba(scene=sc._h, film=FAKE, alpha=FAKE, rgba=FAKE, n_px=px):
        return L.dtof_develop_rgba_f64_async(scene, film, alpha, rgba, n_px)

    def vmap(scene=sc._h, n_passes=1, offsets=off.ctypes.data, n=2, T=0.0015, wg=30.0, out=v.ctypes.data):
        return L.dtof_render_velocity_map_f64(scene, n_passes, 4, offsets, n, T, wg, out, pairs.ctypes.data, tof.ctypes.data, C.byref(st))

    row = 8 * 4      # one film row in doubles
    cases = {"host null scene": lambda: host(scene=None), "host null images": lambda: host(out=None), "host 5 variants": lambda: host(n=5),
             "rows null scene": lambda: rows(scene=None), "rows null film": lambda: rows(film=None), "rows 5 variants": lambda: rows(n=5, planes=5),
             "rows 3 planes for 4": lambda: rows(planes=3), "rows 0 planes": lambda: rows(n=0, planes=0), "rows negative planes": lambda: rows(planes=-1),
             "rows odd stride": lambda: rows(stride=4 * px + 2), "rows stride below a row": lambda: rows(n=1, planes=1, stride=row - 4),
             # rows [2, 4) and the tent's halo of 1 reach rows [1, 5): four rows; [0, 8) the whole film
             "rows overlapping planes": lambda: rows(stride=4 * px - 4), "rows band overlapping planes": lambda: rows(r0=2, r1=4, stride=3 * row),
             "rows misaligned film": lambda: rows(film=FAKE + 4),
             "develop null scene": lambda: develop(scene=None), "develop null film": lambda: develop(film=None), "develop null rgb": lambda: develop(rgb=None),
             "develop negative pixels": lambda: develop(n_px=-1), "develop misaligned film": lambda: develop(film=FAKE + 4),
             "rgba null scene": lambda: develop_rgba(scene=None), "rgba null film": lambda: develop_rgba(film=None), "rgba null alpha": lambda: develop_rgba(alpha=None),
             "rgba null image": lambda: develop_rgba(rgba=None), "rgba negative pixels": lambda: develop_rgba(n_px=-1), "rgba misaligned image": lambda: develop_rgba(rgba=FAKE + 4),
             "map null scene": lambda: vmap(scene=None), "map null offsets": lambda: vmap(offsets=None), "map null out": lambda: vmap(out=None),
             "map 0 offsets": lambda: vmap(n=0), "map 17 offsets": lambda: vmap(n=17), "map 0 passes": lambda: vmap(n_passes=0),
             "map exposure 0": lambda: vmap(T=0.0), "map w_g nan": lambda: vmap(wg=float("nan"))}
    for name, call in cases.items():
        assert call() == INVALID, (name, L.dtof_last_error())
        assert len(L.dtof_last_error()) > 0, name
    for plugin in ("path", "velocity"):      # variants under a non-Doppler integrator
        sc.set_integrator(dict(type=plugin))
        for name, call in (("host", host), ("rows", rows), ("map", vmap)):
            assert call() == INVALID, (plugin, name)
            assert L.dtof_last_error() == b"modulation offsets only apply to the dopplertofpath integrator", (plugin, name, L.dtof_last_error())
    assert (img == np.float32(SENT)).all() and (films == SENT).all() and (v == SENT).all() and (pairs == SENT).all() and (tof == np.float32(SENT)).all()      # no refused call wrote
    # an rgba scene writes the alpha plane behind the colour planes: K planes are one too few
    xml = open(os.path.join(SCENES, "cornell_wall.xml")).read()
    assert '<string name="pixel_format" value="rgb" />' in xml
    rgba = mi.load_string(xml.replace('<string name="pixel_format" value="rgb" />', '<string name="pixel_format" value="rgba" />'), resx=8, resy=8)
    assert rgba.info()["has_alpha"]
    assert rows(scene=rgba._h, planes=4) == INVALID and b"writes 5" in L.dtof_last_error()


def test_film_argument_takes_the_two_names_only(mi):
    sc = _wall(mi)
    integrator = mi.load_dict(dict(type="dopplertofpath", max_depth=2))
    calls = {"render": lambda f: sc.render(seed=0, spp=4, film=f), "render offsets": lambda f: sc.render(seed=0, spp=4, offsets=[0.0, 0.5], film=f),
             "render variants": lambda f: sc.render(seed=0, spp=4, variants=[(0, 0), (1, 0)], film=f),
             "velocity map": lambda f: sc.render_velocity_map(1, 4, film=f), "integrator": lambda f: integrator.render(sc, seed=0, spp=4, film=f),
             "multi pass": lambda f: mi.render_multi_pass(sc, integrator, 4, film=f)}
    from mitsuba3dopplertof_amd import harness
    calls["harness host"] = lambda f: harness.run_scene_velocity_map(sc, total_spp=4, film=f)
    calls["harness device"] = lambda f: harness.run_scene_velocity_map_device(sc, total_spp=4, film=f)
    for name, call in calls.items():
        for bad in ("float17", "double", "", None, 64):
            with pytest.raises(mi.DtofError, match="float32.*float64"):
                call(bad)
    assert mi.FILMS == ("float32", "float64")
    with pytest.raises(mi.DtofError, match="at most 4"):      # render_film64 is ONE traversal
        sc.render_film64(0, 4, variants=[(0, 0.1 * i) for i in range(5)])
    with pytest.raises(mi.DtofError, match="sensor index 1"):
        sc.render(seed=0, spp=4, sensor=1, film="float64")


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_render_variants_f64.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_int, vp, vp, vp]
L.dtof_render_rows_variants_f64.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, vp, C.c_int, vp, C.c_int32, C.c_uint64, vp]
L.dtof_develop_f64_async.argtypes = [vp, vp, vp, C.c_int64]
L.dtof_develop_rgba_f64_async.argtypes = [vp, vp, vp, vp, C.c_int64]
L.dtof_render_velocity_map_f64.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
off, v = (C.c_float * 2)(0.0, 0.25), (C.c_double * 64)(*([7.0] * 64))
var = (C.c_float * 8)(0, 0, 0, .25, 1, 0, 1, .25)
img, films = (C.c_float * (4 * 64 * 3))(*([7.0] * 768)), (C.c_double * (4 * 64 * 4))(*([7.0] * 1024))
FAKE = 0x1000
print(L.dtof_render_variants_f64(h, 0, 4, var, 4, img, films, None), L.dtof_render_variants_f64(h, 0, 4, None, 0, img, None, None),
      L.dtof_render_rows_variants_f64(h, 0, 4, 0, 8, var, 4, FAKE, 4, 0, None), L.dtof_develop_f64_async(h, FAKE, FAKE, 64),
      L.dtof_develop_rgba_f64_async(h, FAKE, FAKE, FAKE, 64), L.dtof_render_velocity_map_f64(h, 1, 4, off, 2, 0.0015, 30.0, v, None, None, None),
      int(all(x == 7.0 for x in v) and all(x == 7.0 for x in img) and all(x == 7.0 for x in films)))
"""


def test_compute_entries_fail_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    import subprocess
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), os.path.join(SCENES, "cornell_wall.xml")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP)] * 6 + ["1"], r.stdout


def test_command_line_parses_film(mi, monkeypatch, capsys):
    from mitsuba3dopplertof_amd import __main__ as cli
    assert cli.parser().parse_args(["scene.xml"]).film == "float32"
    assert cli.parser().parse_args(["scene.xml", "--film", "float64"]).film == "float64"
    args = cli.parser().parse_args(["scene.xml", "--velocity-map", "0,0.25", "--film", "float64", "--spp", "64"])
    assert (args.velocity_map, args.film, args.spp) == ("0,0.25", "float64", 64)
    scene = os.path.join(SCENES, "cornell_wall.xml")
    with pytest.raises(SystemExit) as e:      # argparse refuses any other name
        cli.main([scene, "--film", "float17"])
    assert e.value.code == 2 and "float17" in capsys.readouterr().err
    refused = {"ranks": ([scene, "--film", "float64"], "2"), "stripes": ([scene, "--film", "float64", "--stripes", "4"], "1")}
    for what, (argv, world) in refused.items():
        monkeypatch.setenv("WORLD_SIZE", world)
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and "single-GPU" in capsys.readouterr().err, what
