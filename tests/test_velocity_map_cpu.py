"""The device velocity map (dtof_develop_accumulate_async, dtof_velocity_map_async, dtof_render_velocity_map) as far as it can be held without a GPU: the header
declares the entries and the library exports them, refusals that need no device come back as DTOF_ERR_INVALID and leave the outputs alone, what passes them fails
with DTOF_ERR_HIP on a host without a device (there is no CPU fallback), offsets are grouped two per traversal, and the command line parses --velocity-map."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, HIP = 0, 1, 2
ENTRIES = ("dtof_develop_accumulate_async", "dtof_velocity_map_async", "dtof_velocity_map_variants", "dtof_render_velocity_map")
FAKE = 0x1000      # a non-null, 16-byte aligned "device pointer": a refused call never dereferences or enqueues it


def test_header_declares_and_library_exports_the_entries(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        assert hasattr(lib, name), name
    # the doubles of the numpy route cross the boundary as doubles
    for name in ("dtof_velocity_map_async", "dtof_render_velocity_map"):
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1)
        assert re.search(r"double\s+exposure_time", args) and re.search(r"double\s+w_g_mhz", args), name
    # each entry cites what it replaces
    for name in ("dtof_develop_accumulate_async", "dtof_velocity_map_async", "dtof_render_velocity_map"):
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert "doppler_tutorials/src/utils/image_utils.py:20-31,140-199" in comment and "program_runner.py:11-31" in comment, name


def test_offsets_are_grouped_two_per_traversal(mi):
    """(0, o0), (0, o1), (1, o0), (1, o1) per group; the odd last offset is a group of its own -- the films harness.run_scene_velocity_map renders"""
    assert mi.velocity_map_variants([0.0, 0.25]).tolist() == [[0, 0], [0, 0.25], [1, 0], [1, 0.25]]
    assert mi.velocity_map_variants([0.5]).tolist() == [[0, 0.5], [1, 0.5]]
    got = mi.velocity_map_variants([0.0, 0.25, 0.5])
    assert got.tolist() == [[0, 0], [0, 0.25], [1, 0], [1, 0.25], [0, 0.5], [1, 0.5]]
    offsets = [0.125 * i for i in range(7)]
    expect = []
    for g in range(0, len(offsets), 2):      # the loop of harness.run_scene_velocity_map
        expect += [(0.0, o) for o in offsets[g:g + 2]] + [(1.0, o) for o in offsets[g:g + 2]]
    assert np.array_equal(mi.velocity_map_variants(offsets), np.asarray(expect, np.float32))
    assert mi.velocity_map_variants([0.1] * 16).shape == (32, 2)
    for bad in ([], [0.0] * 17):
        with pytest.raises(mi.DtofError, match="between 1 and 16 offsets"):
            mi.velocity_map_variants(bad)
    L = mi._lib()
    one = np.zeros(1, np.float32)
    out = np.zeros((2, 2), np.float32)
    assert L.dtof_velocity_map_variants(None, 1, out.ctypes.data) == INVALID
    assert L.dtof_velocity_map_variants(one.ctypes.data, 1, None) == INVALID


def _wall(mi):
    return mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=8, resy=8)


def test_refusals_that_need_no_device(mi):
    L = mi._lib()
    sc = _wall(mi)
    px = 64
    off = np.asarray([0.0, 0.25] * 9, np.float32)
    SENT = 123.25
    v, pairs, tof = np.full(px, SENT), np.full((18, px), SENT), np.full((36, px), SENT, np.float32)
    st = mi._Stats()
    hom, het = np.asarray([0, 1] * 9, np.int32), np.asarray([2, 3] * 9, np.int32)

    def render(scene=sc._h, n_passes=1, offsets=off.ctypes.data, n=2, T=0.0015, wg=30.0, out=v.ctypes.data):
        return L.dtof_render_velocity_map(scene, n_passes, 4, offsets, n, T, wg, out, pairs.ctypes.data, tof.ctypes.data, C.byref(st))

    def vmap(scene=sc._h, d_sum=FAKE, n=2, h=hom.ctypes.data, t=het.ctypes.data, n_passes=1, T=0.0015, wg=30.0, n_px=px, d_v=FAKE):
        return L.dtof_velocity_map_async(scene, d_sum, n, h, t, n_passes, T, wg, n_px, None, None, d_v)

    def accumulate(scene=sc._h, film=FAKE, planes=4, stride=0, d_sum=FAKE, n_px=px):
        return L.dtof_develop_accumulate_async(scene, film, planes, stride, d_sum, n_px, 1)

    nan, inf = float("nan"), float("inf")
    cases = {"render null scene": lambda: render(scene=None), "render null offsets": lambda: render(offsets=None), "render null out": lambda: render(out=None),
             "render 0 offsets": lambda: render(n=0), "render 17 offsets": lambda: render(n=17), "render 0 passes": lambda: render(n_passes=0),
             "map null scene": lambda: vmap(scene=None), "map null sum": lambda: vmap(d_sum=None), "map null homodyne": lambda: vmap(h=None),
             "map null heterodyne": lambda: vmap(t=None), "map null velocity": lambda: vmap(d_v=None), "map 0 pairs": lambda: vmap(n=0),
             "map 17 pairs": lambda: vmap(n=17), "map 0 passes": lambda: vmap(n_passes=0), "map negative pixels": lambda: vmap(n_px=-1),
             "map plane 4 of 4": lambda: vmap(h=np.asarray([0, 4], np.int32).ctypes.data), "map plane -1": lambda: vmap(t=np.asarray([-1, 3], np.int32).ctypes.data),
             "map plane 2 of 2": lambda: vmap(n=1, t=np.asarray([2], np.int32).ctypes.data),
             "accumulate null scene": lambda: accumulate(scene=None), "accumulate null film": lambda: accumulate(film=None),
             "accumulate null sum": lambda: accumulate(d_sum=None), "accumulate 0 planes": lambda: accumulate(planes=0),
             "accumulate negative pixels": lambda: accumulate(n_px=-1), "accumulate short stride": lambda: accumulate(stride=4 * px - 4),
             "accumulate odd stride": lambda: accumulate(stride=4 * px + 2), "accumulate misaligned film": lambda: accumulate(film=FAKE + 4)}
    for what, bad in (("exposure_time", dict(T=0.0)), ("exposure_time", dict(T=-1.0)), ("exposure_time", dict(T=nan)), ("exposure_time", dict(T=inf)),
                      ("w_g_mhz", dict(wg=0.0)), ("w_g_mhz", dict(wg=-30.0)), ("w_g_mhz", dict(wg=nan)), ("w_g_mhz", dict(wg=inf))):
        cases["render %s %r" % (what, bad)] = lambda bad=bad: render(**bad)
        cases["map %s %r" % (what, bad)] = lambda bad=bad: vmap(**bad)
    for name, call in cases.items():
        assert call() == INVALID, (name, L.dtof_last_error())
        assert len(L.dtof_last_error()) > 0, name
    for plugin in ("path", "velocity"):
        sc.set_integrator(dict(type=plugin))
        assert render() == INVALID, plugin
        assert L.dtof_last_error() == b"modulation offsets only apply to the dopplertofpath integrator", (plugin, L.dtof_last_error())
    assert (v == SENT).all() and (pairs == SENT).all() and (tof == np.float32(SENT)).all()      # no refused call wrote
    for wrapper in (lambda: sc.render_velocity_map(1, 4), lambda: sc.render_velocity_map(0, 4, offsets=(0.0,)), lambda: sc.render_velocity_map(1, 4, w_g=0)):
        with pytest.raises(mi.DtofError):
            wrapper()


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_render_velocity_map.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp]
L.dtof_velocity_map_async.argtypes = [vp, vp, C.c_int, vp, vp, C.c_uint32, C.c_double, C.c_double, C.c_int64, vp, vp, vp]
L.dtof_develop_accumulate_async.argtypes = [vp, vp, C.c_int32, C.c_uint64, vp, C.c_int64, C.c_int]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
off, v = (C.c_float * 2)(0.0, 0.25), (C.c_double * 64)(*([7.0] * 64))
hom, het = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(2, 3)
FAKE = 0x1000
print(L.dtof_render_velocity_map(h, 1, 4, off, 2, 0.0015, 30.0, v, None, None, None),
      L.dtof_velocity_map_async(h, FAKE, 2, hom, het, 1, 0.0015, 30.0, 64, None, None, FAKE),
      L.dtof_develop_accumulate_async(h, FAKE, 4, 0, FAKE, 64, 1), int(all(x == 7.0 for x in v)))
"""


def test_compute_entries_fail_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    import subprocess
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), os.path.join(SCENES, "cornell_wall.xml")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP)] * 3 + ["1"], r.stdout


def test_command_line_parses_velocity_map(mi, monkeypatch, capsys):
    from mitsuba3dopplertof_amd import __main__ as cli
    args = cli.parser().parse_args(["scene.xml", "--velocity-map", "0,0.25"])
    assert args.velocity_map == "0,0.25" and args.w_g == 30.0 and args.exposure_time == 0.0015
    args = cli.parser().parse_args(["scene.xml", "--velocity-map", "0,0.25,0.5", "--w-g", "150", "--exposure-time", "0.002", "--spp", "64", "-o", "v.npy"])
    assert (args.velocity_map, args.w_g, args.exposure_time, args.spp, args.output) == ("0,0.25,0.5", 150.0, 0.002, 64, "v.npy")
    assert cli.parser().parse_args(["scene.xml"]).velocity_map is None
    scene = os.path.join(SCENES, "cornell_wall.xml")
    refused = {"single-GPU": [scene, "--velocity-map", "0,0.25"], "--offsets": [scene, "--velocity-map", "0", "--offsets", "0,0.5"],
               "--seed": [scene, "--velocity-map", "0", "--seed", "3"], ".npy": [scene, "--velocity-map", "0", "-o", "v.exr"],
               "numbers": [scene, "--velocity-map", "a,b"]}
    for message, argv in refused.items():
        monkeypatch.setenv("WORLD_SIZE", "2" if message == "single-GPU" else "1")
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err, message
