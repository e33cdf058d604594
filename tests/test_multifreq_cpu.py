"""A modulation frequency per variant (dtof_render_variants_freq, dtof_render_variants_freq_f64, dtof_sample_lanes_variants_freq) as far as it can be held without a
GPU: the header declares the entries and the library exports them, every refusal comes back as DTOF_ERR_INVALID before a device is touched and leaves the outputs
alone, what passes them fails with DTOF_ERR_HIP on a host without a device (there is no CPU fallback), variants are all pairs or all triples, and the command line
parses hetero_frequency:hetero_offset:w_g triples."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, HIP = 0, 1, 2
ENTRIES = ("dtof_render_variants_freq", "dtof_render_variants_freq_f64", "dtof_sample_lanes_variants_freq")
WALL = os.path.join(SCENES, "cornell_wall.xml")


def test_header_declares_and_library_exports_the_entries(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl and hasattr(lib, name), name
        assert re.search(r"const\s+float\s*\*\s*w_g_mhz_or_null\s*,\s*int\s+n_variants", decl.group(1)), name      # the frequencies sit in front of their count
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert re.search(r"\.(cpp|h):\d+", comment), name      # each entry cites what it replaces
    assert "keep the\n * integrator's single w_g" in hdr          # what is out of scope is said


def test_refusals_that_need_no_device(mi):
    L = mi._lib()
    sc = mi.load_file(WALL, resx=8, resy=8)
    SENT = 123.25
    out, films = np.full((5, 8, 8, 3), SENT, np.float32), np.full((5, 8, 8, 4), SENT)
    lanes, valid, rgb = np.full((64, 12), SENT, np.float32), np.full(64, 7, np.uint32), np.full((5, 64, 3), SENT, np.float32)
    st = mi._Stats()
    var = np.ascontiguousarray([(0.0, 0.1 * i) for i in range(5)], np.float32)
    nan, inf = float("nan"), float("inf")

    alive = []      # the arrays whose addresses the calls below hold

    def calls(v, f, n, scene=sc._h):
        alive.extend([v, f])
        v, f = (None if v is None else v.ctypes.data), (None if f is None else f.ctypes.data)
        return {"render": lambda: L.dtof_render_variants_freq(scene, 0, 4, v, f, n, out.ctypes.data, C.byref(st)),
                "render_f64": lambda: L.dtof_render_variants_freq_f64(scene, 0, 4, v, f, n, out.ctypes.data, films.ctypes.data, C.byref(st)),
                "lanes": lambda: L.dtof_sample_lanes_variants_freq(scene, 0, 4, v, f, n, 0, 64, lanes.ctypes.data, valid.ctypes.data, rgb.ctypes.data)}

    def freq(*values):
        return np.asarray(values, np.float32)

    refused = {"five variants": (calls(var, freq(30, 30, 30, 30, 30), 5), b"at most 4 modulation variants"),
               "five variants, no frequencies": (calls(var, None, 5), b"at most 4 modulation variants"),
               "frequencies without variants": (calls(None, freq(30, 40), 2), b"frequencies come with the variants"),
               "frequencies with n_variants 0": (calls(var, freq(30, 40), 0), b"frequencies come with the variants"),
               "null scene": (calls(var, freq(30, 40), 2, scene=None), b"null argument")}
    for bad in (0.0, -30.0, nan, inf, -inf):
        refused["frequency %r" % bad] = (calls(var, freq(30, bad), 2), b"w_g_mhz[1] must be finite and > 0")
    for what, (group, message) in refused.items():
        for name, call in group.items():
            assert call() == INVALID, (what, name)
            assert message in L.dtof_last_error(), (what, name, L.dtof_last_error())
    for plugin in ("path", "velocity"):      # the refusal of the variants forms
        sc.set_integrator(dict(type=plugin))
        for name, call in calls(var, freq(30, 40), 2).items():
            assert call() == INVALID, (plugin, name)
            assert L.dtof_last_error() == b"modulation offsets only apply to the dopplertofpath integrator", (plugin, name, L.dtof_last_error())
    sc.set_integrator(dict(type="dopplertofpath"))
    two = freq(30, 40)
    assert L.dtof_render_variants_freq(sc._h, 0, 4, var.ctypes.data, two.ctypes.data, 2, None, C.byref(st)) == INVALID
    assert L.dtof_sample_lanes_variants_freq(sc._h, 0, 4, var.ctypes.data, two.ctypes.data, 2, 0, 64, None, None, rgb.ctypes.data) == INVALID
    assert L.dtof_sample_lanes_variants_freq(sc._h, 0, 4, var.ctypes.data, two.ctypes.data, 2, 0, 64, lanes.ctypes.data, None, None) == INVALID
    assert (out == np.float32(SENT)).all() and (films == SENT).all() and (lanes == np.float32(SENT)).all() and (valid == 7).all() and (rgb == np.float32(SENT)).all()


def test_variants_are_all_pairs_or_all_triples(mi):
    pairs, freq = mi._variant_freq([(0.0, 0.25), (1.0, 0.5)])
    assert freq is None and pairs.dtype == np.float32 and pairs.tolist() == [[0.0, 0.25], [1.0, 0.5]]
    pairs, freq = mi._variant_freq([(0.0, 0.25, 30.0), (1.0, 0.5, 40.0)])
    assert pairs.tolist() == [[0.0, 0.25], [1.0, 0.5]] and freq.tolist() == [30.0, 40.0]
    assert pairs.flags["C_CONTIGUOUS"] and freq.flags["C_CONTIGUOUS"] and pairs.dtype == freq.dtype == np.float32
    pairs, freq = mi._variant_freq(np.asarray([(0.0, 0.25, 17.3)], np.float64))      # an array of triples
    assert freq.tolist() == [float(np.float32(17.3))]
    for mixed in ([(0.0, 0.25), (1.0, 0.5, 40.0)], [(0.0, 0.25, 30.0), (1.0, 0.5)]):
        with pytest.raises(mi.DtofError, match="not a mixture"):
            mi._variant_freq(mixed)
    for bad in ([(0.0,)], [(0.0, 1.0, 2.0, 3.0)], [1.0, 2.0]):
        with pytest.raises(mi.DtofError, match="pairs"):
            mi._variant_freq(bad)
    sc = mi.load_file(WALL, resx=8, resy=8)
    for call in (lambda v: sc.render(spp=4, variants=v), lambda v: sc.render(spp=4, variants=v, film="float64"), lambda v: sc.render_film64(spp=4, variants=v),
                 lambda v: sc.sample_lanes_variants(0, 4, 0, 64, v)):
        with pytest.raises(mi.DtofError, match="not a mixture"):
            call([(0.0, 0.25), (1.0, 0.5, 40.0)])
        with pytest.raises(mi.DtofError, match="must be finite and > 0"):      # the library's refusal, through the binding
            call([(0.0, 0.25, 30.0), (0.0, 0.25, 0.0)])


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_render_variants_freq.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int, vp, vp]
L.dtof_render_variants_freq_f64.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int, vp, vp, vp]
L.dtof_sample_lanes_variants_freq.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
var, freq = (C.c_float * 4)(0.0, 0.0, 0.0, 0.25), (C.c_float * 2)(30.0, 40.0)
out, lanes, rgb = (C.c_float * 384)(*([7.0] * 384)), (C.c_float * 768)(), (C.c_float * 384)(*([7.0] * 384))
print(L.dtof_render_variants_freq(h, 0, 4, var, freq, 2, out, None), L.dtof_render_variants_freq_f64(h, 0, 4, var, freq, 2, out, None, None),
      L.dtof_sample_lanes_variants_freq(h, 0, 4, var, freq, 2, 0, 64, lanes, None, rgb), int(all(x == 7.0 for x in out) and all(x == 7.0 for x in rgb)))
"""


def test_compute_entries_fail_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), WALL], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP)] * 3 + ["1"], r.stdout


def test_command_line_parses_triples(mi, monkeypatch, capsys):
    from mitsuba3dopplertof_amd import __main__ as cli
    assert cli.parse_variants("0:0,1:0.25") == [(0.0, 0.0), (1.0, 0.25)]
    assert cli.parse_variants("0:0:30,0:0.25:40", triples=True) == [(0.0, 0.0, 30.0), (0.0, 0.25, 40.0)]
    for text, triples in (("0:0:30", False), ("0:0", True), ("0:0:30,0:0.25", True), ("0:0,0:0.25:40", False), ("a:b:c", True)):
        with pytest.raises(ValueError):
            cli.parse_variants(text, triples=triples)
    monkeypatch.setenv("WORLD_SIZE", "1")
    refused = {"all of them triples": [WALL, "--variants", "0:0:30,0:0.25"], "belong to --moments": [WALL, "--variants", "0:0"],
               "replaces --offsets": [WALL, "--variants", "0:0:30", "--offsets", "0,0.5"], "single-GPU": [WALL, "--variants", "0:0:30", "--stripes", "4"],
               "plain images": [WALL, "--variants", "0:0:30", "--velocity-map", "0,0.25"],
               "pairs": [WALL, "--moments", "--variants", "0:0:30"],                         # the moment film keeps the integrator's w_g
               "hetero_frequency:hetero_offset pairs": [WALL, "--adaptive", "0.1", "--variants", "0:0:30"]}
    for message, argv in refused.items():
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err, message
