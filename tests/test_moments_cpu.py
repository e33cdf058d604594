"""The per-pixel moment film (dtof_moment_planes, dtof_render_moments; Scene.render_moments, harness.moment_statistics / velocity_standard_error / run_scene_moments,
<integrator type="moment">, --moments) as far as it can be held without a GPU:
  - the expected-value helper of the GPU tests (moments_ref.py) against the oracle ALONE: its sums of w and w * rgb must be the raw film of orc_render_exact within
    2^-40 * sum |term| per pixel (both add the same float32 terms in double, in different orders; <= 2^12 terms a pixel, 2^-53 per addition) -- this pins the numpy
    mirror of the footprint arithmetic to the reference before any GPU run depends on it
  - the header declares and the library exports the entries, the plane counts, the refusals that need no device, DTOF_ERR_HIP without one
  - the loader's `moment` wrapper, the harness statistics on synthetic moments, the command line."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENES
import moments_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, HIP = 0, 1, 2
WALL = os.path.join(SCENES, "cornell_wall.xml")


def _edited(scene, edit):
    xml = open(os.path.join(SCENES, scene)).read()
    old, new = '<rfilter type="tent" />', '<rfilter type="%s" />' % edit
    assert old in xml
    return xml.replace(old, new)


@pytest.mark.parametrize("scene,params,spp,edit", [("cornell_wall.xml", dict(resx=16, resy=16), 16, None), ("cornell_wall.xml", dict(resx=16, resy=16), 16, "box"),
                                                   ("cornell_rough.xml", dict(resx=24, resy=24, max_depth=5), 8, "gaussian")], ids=["tent", "box", "gaussian"])
def test_helper_against_the_exact_oracle(orc, scene, params, spp, edit):
    osc = orc.Scene(_edited(scene, edit), params, is_string=True) if edit else orc.Scene(os.path.join(SCENES, scene), params)
    pd = osc.params()
    w, h = osc.size
    film = np.zeros((h, w, 4), np.float64)
    L = orc.lib()
    L.orc_render_exact.restype = C.c_uint64
    L.orc_render_exact.argtypes = [C.POINTER(orc.OrcScene), C.POINTER(orc.OrcParams), C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
    p = orc.make_params(pd)
    assert L.orc_render_exact(C.byref(osc.c), C.byref(p), 3, spp, 0, h, film.ctypes.data, None, ref.NCPU) == w * h * spp
    lanes = ref.lanes_of(orc, osc, pd, 3, spp)
    spw, n_passes = ref.pass_layout(orc, osc, pd, spp)
    assert (spw, n_passes) == (spp, 1)
    fp = ref.footprint(orc, osc, lanes["sample_pos"], spw)
    values = np.concatenate([lanes["rgb"], np.ones((len(lanes), 1), np.float32)], axis=1)      # r, g, b, 1: the film's channels
    sums, mags = ref.splat(osc, fp, values)
    ratios = ref.errors_over_bound(sums, np.moveaxis(film, -1, 0), mags)
    print("%s: helper against orc_render_exact, largest error / bound: r %.3g g %.3g b %.3g w %.3g" % ((edit or "tent",) + tuple(ratios)))
    assert np.abs(film[..., :3]).max() > 0 and (film[..., 3] > 0).all()
    assert (ratios <= 1.0).all(), ratios


def test_header_declares_and_library_exports_the_entries(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ("dtof_moment_planes", "dtof_render_moments"):
        assert re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr), name
        assert hasattr(lib, name), name
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert "moment.cpp" in comment and "imageblock.cpp:414-531" in comment, name
    args = re.sub(r"\s+", " ", re.search(r"\bint\s+dtof_render_moments\s*\(([^;]*)\)\s*;", hdr).group(1))
    assert re.search(r"uint32_t n_passes", args) and re.search(r"int developed", args) and re.search(r"double \*out_planes", args)
    assert [lib.dtof_moment_planes(k) for k in (1, 2, 3, 4)] == [7, 14, 22, 31] and lib.dtof_moment_planes(0) == 7
    assert [lib.dtof_moment_planes(k) for k in (-1, 5, 100)] == [-1, -1, -1]
    assert [mi.MOMENT_PLANES(k) for k in (0, 1, 2, 3, 4, 5)] == [7, 7, 14, 22, 31, -1]
    assert [ref.n_planes(k) for k in (1, 2, 3, 4)] == [7, 14, 22, 31]


def test_refusals_that_need_no_device(mi):
    L = mi._lib()
    sc = mi.load_file(WALL, resx=8, resy=8)
    SENT = 123.25
    out = np.full((31, 64), SENT)
    var = np.asarray([(0, 0), (0, .25), (1, 0), (1, .25), (1, .5)], np.float32)
    st = mi._Stats()

    def call(scene=sc._h, n_passes=1, variants=var.ctypes.data, n=2, planes=out.ctypes.data):
        return L.dtof_render_moments(scene, 0, 4, n_passes, variants, n, 1, planes, C.byref(st))

    cases = {"null scene": lambda: call(scene=None), "null output": lambda: call(planes=None), "0 passes": lambda: call(n_passes=0),
             "5 variants": lambda: call(n=5), "-1 variants": lambda: call(n=-1), "a count without variants": lambda: call(variants=None, n=2)}
    for name, f in cases.items():
        assert f() == INVALID, (name, L.dtof_last_error())
        assert len(L.dtof_last_error()) > 0, name
    for plugin in ("path", "velocity"):      # variants under a non-Doppler integrator: the rule of the other variants entries
        sc.set_integrator(dict(type=plugin))
        assert call() == INVALID
        assert L.dtof_last_error() == b"modulation offsets only apply to the dopplertofpath integrator", (plugin, L.dtof_last_error())
    assert (out == SENT).all()      # no refused call wrote
    with pytest.raises(mi.DtofError, match="between 1 and 4"):
        sc.render_moments(variants=[(0, 0)] * 5)
    with pytest.raises(mi.DtofError):
        sc.render_moments(variants=[])
    with pytest.raises(mi.DtofError, match="moment.*scene file.*render_moments"):      # a property dictionary cannot carry the nested plugin
        sc.set_integrator({"type": "moment", "nested": {"type": "path"}})
    with pytest.raises(mi.DtofError, match="render_moments"):
        mi.Integrator({"type": "moment"})


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_render_moments.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_int, vp, vp]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
var = (C.c_float * 4)(0, 0, 1, 0)
out = (C.c_double * (14 * 64))(*([7.0] * (14 * 64)))
print(L.dtof_render_moments(h, 0, 4, 1, var, 2, 1, out, None), L.dtof_render_moments(h, 0, 4, 2, None, 0, 0, out, None), int(all(x == 7.0 for x in out)))
"""


def test_render_moments_fails_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), WALL], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP), str(HIP), "1"], r.stdout


def _wrap(xml, inner=None, copies=1):
    """the scene's integrator inside <integrator type="moment">: `copies` of it, or of `inner`"""
    m = re.search(r"<integrator type=\"dopplertofpath\">.*?</integrator>", xml, re.S)
    assert m
    body = m.group(0) if inner is None else inner
    return xml[:m.start()] + '<integrator type="moment">' + "".join(body.replace("<integrator", '<integrator name="nested_%d"' % i, 1) for i in range(copies)) + "</integrator>" + xml[m.end():]


def test_loader_takes_the_moment_wrapper(mi):
    xml = open(WALL).read()
    params = dict(resx=16, resy=16, max_depth=3)
    plain, wrapped = mi.load_string(xml, **params), mi.load_string(_wrap(xml), **params)
    assert wrapped.info() == plain.info() and plain.info()["max_depth"] == 3      # the nested plugin is the scene's integrator, with all its properties
    with pytest.raises(mi.DtofError, match="moment.*2 nested integrators"):
        mi.load_string(_wrap(xml, copies=2), **params)
    with pytest.raises(mi.DtofError, match="moment.*none was given"):
        mi.load_string(_wrap(xml, copies=0), **params)
    with pytest.raises(mi.DtofError, match=r'unsupported integrator plugin "volpath" \(this library implements'):      # the message of a scene-level integrator
        mi.load_string(_wrap(xml, inner='<integrator type="volpath"></integrator>'), **params)
    with pytest.raises(mi.DtofError, match='unsupported integrator plugin "volpath"'):
        mi.load_string(re.sub(r"<integrator type=\"dopplertofpath\">.*?</integrator>", '<integrator type="volpath"></integrator>', xml, flags=re.S), **params)
    with pytest.raises(mi.DtofError, match="moment"):      # the wrapper queries nothing but its child
        mi.load_string(_wrap(xml).replace('<integrator type="moment">', '<integrator type="moment"><integer name="max_depth" value="2" />'), **params)


def _two_point(lo, hi, shape=(1, 2, 2)):
    """the moments of a sample that is `lo` or `hi` with probability 1/2 each, in every channel"""
    mean, m2 = np.full(shape + (3,), (lo + hi) / 2.0), np.full(shape + (3,), (lo * lo + hi * hi) / 2.0)
    return mean, m2


def test_moment_statistics_of_a_two_point_distribution(mi):
    from mitsuba3dopplertof_amd import harness
    # variant 0: Y in {1, 3}; variant 1 = 2 Y of the same paths: {2, 6}.  var 1 and 4, covariance E[Y 2Y] - 2 * 4 = 10 - 8 = 2 -- all exact in binary
    mean0, m20 = _two_point(1.0, 3.0)
    mean1, m21 = _two_point(2.0, 6.0)
    m = {"weight": np.full((2, 2), 8.0), "mean": np.concatenate([mean0, mean1]), "m2": np.concatenate([m20, m21]), "cross": np.zeros((2, 2, 2, 2))}
    m["cross"][0, 0], m["cross"][1, 1], m["cross"][0, 1], m["cross"][1, 0] = 5.0, 20.0, 10.0, 10.0
    st = harness.moment_statistics(m, 16)
    assert st["variance"].shape == (2, 2, 2, 3) and (st["variance"][0] == 1.0).all() and (st["variance"][1] == 4.0).all()
    assert (st["cov_y"][0, 1] == 2.0).all() and (st["cov_y"][1, 0] == 2.0).all() and (st["cov_y"][0, 0] == 1.0).all() and (st["cov_y"][1, 1] == 4.0).all()
    assert (st["stderr"][0] == 0.25).all() and (st["stderr"][1] == 0.5).all()      # sqrt(1 / 16), sqrt(4 / 16)
    m["m2"][0, 0, 0, 0] = 3.0      # rounding can leave m2 below mean^2: the standard error clamps, the variance does not
    st = harness.moment_statistics(m, 16)
    assert st["variance"][0, 0, 0, 0] == -1.0 and st["stderr"][0, 0, 0, 0] == 0.0


def _moments_of(a, b, var_a, var_b, cov):
    """a one-pixel dict whose Y means are a (variant 0) and b (variant 1) with the given second central moments"""
    mean = np.zeros((2, 1, 1, 3)); m2 = np.zeros((2, 1, 1, 3)); cross = np.zeros((2, 2, 1, 1))
    mean[0, ..., 1], mean[1, ..., 1] = a, b
    m2[0, ..., 1], m2[1, ..., 1] = var_a + a * a, var_b + b * b
    cross[0, 0], cross[1, 1], cross[0, 1], cross[1, 0] = m2[0, ..., 1], m2[1, ..., 1], cov + a * b, cov + a * b
    return {"weight": np.ones((1, 1)), "mean": mean, "m2": m2, "cross": cross}


def test_velocity_standard_error_is_the_delta_method(mi):
    from mitsuba3dopplertof_amd import harness
    T, wg, n, h = 0.0015, 30, 64, 1e-6
    for a, r in ((2.0, -0.5), (-3.0, 0.25), (0.5, 0.9)):      # three ratios inside the clip interval (-1, 0.999)
        sigma_b = 0.125
        se = harness.velocity_standard_error(_moments_of(a, r * a, 0.0, sigma_b ** 2, 0.0), 0, 1, n, T, wg)
        slope = (harness._velocity_from_ratio(r + h, T, wg) - harness._velocity_from_ratio(r - h, T, wg)) / (2 * h)      # central finite difference
        want = abs(slope) * sigma_b / (abs(a) * np.sqrt(n))
        assert se.shape == (1, 1) and abs(se[0, 0] - want) <= 1e-6 * want, (a, r, se, want)
    # the shared paths of a homodyne / heterodyne pair: a positive covariance with r > 0 lowers the error
    apart = harness.velocity_standard_error(_moments_of(2.0, 1.0, 0.04, 0.01, 0.0), 0, 1, n, T, wg)[0, 0]
    shared = harness.velocity_standard_error(_moments_of(2.0, 1.0, 0.04, 0.01, 0.015), 0, 1, n, T, wg)[0, 0]
    assert 0 < shared < apart
    # the variants are picked by index: swapped, the ratio is 2 and lies outside the clip interval
    assert np.isnan(harness.velocity_standard_error(_moments_of(2.0, 1.0, 0.04, 0.01, 0.0), 1, 0, n, T, wg)[0, 0])
    # NaN exactly where a == 0 or r is outside the OPEN interval (-1, 0.999)
    cases = [(0.0, 1.0, True), (1.0, -1.0, True), (1.0, 0.999, True), (1.0, 1.5, True), (1.0, -2.0, True), (1.0, 0.998, False), (1.0, -0.999, False), (1.0, 0.0, False)]
    for a, b, nan in cases:
        se = harness.velocity_standard_error(_moments_of(a, b, 0.01, 0.01, 0.0), 0, 1, n, T, wg)[0, 0]
        assert np.isnan(se) == nan, (a, b, se)
        assert nan or se > 0


def test_command_line_parses_moments(mi, monkeypatch, capsys):
    from mitsuba3dopplertof_amd import __main__ as cli
    args = cli.parser().parse_args(["scene.xml", "--moments", "--variants", "0:0,1:0", "--passes", "3", "-o", "m.npz"])
    assert args.moments and (args.variants, args.passes, args.output) == ("0:0,1:0", 3, "m.npz")
    assert cli.parse_variants(args.variants) == [(0.0, 0.0), (1.0, 0.0)]
    assert not cli.parser().parse_args(["scene.xml"]).moments
    refused = {"velocity-map": [WALL, "--moments", "--velocity-map", "0,0.25"], "stripes": [WALL, "--moments", "--stripes", "4"],
               "float64": [WALL, "--moments", "--film", "float64"], "pairs": [WALL, "--moments", "--variants", "0,1"],
               "between 1 and 4": [WALL, "--moments", "--variants", "0:0,0:.1,0:.2,0:.3,0:.4"], ".npz": [WALL, "--moments", "-o", "m.npy"],
               "belong to --moments": [WALL, "--passes", "2"]}
    for what, argv in refused.items():
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and what in capsys.readouterr().err, what
