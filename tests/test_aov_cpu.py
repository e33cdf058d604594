"""The geometry channels of the `aov` integrator (dtof_aov_parse, dtof_scene_get_aovs, dtof_render_aovs, dtof_sample_aov_lanes; mi.aov_channels, Scene.aovs,
Scene.render_aovs, harness.run_scene_aovs, <integrator type="aov">, --aovs) as far as they can be held without a GPU:
  - the parse: channel names and their order for every type (src/integrators/aov.cpp:118-171), the reference's tokenizer, every refusal message
  - the 31-channel cap and the other refusals that need no device, DTOF_ERR_HIP from every compute entry without one
  - the loader's `aov` wrapper: zero / two nested integrators, `moment` / `aov` nesting, the spec surviving $parameters
  - the expected-value helper of the GPU tests (aov_ref.py) on the oracle alone: the conditions its far-plane-less query needs hold at the GPU tests' shapes
  - the command line."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENES
import aov_ref as aref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, HIP = 0, 1, 2
WALL = os.path.join(SCENES, "cornell_wall.xml")


def test_channel_names_of_every_type(mi):
    want = {"depth": ["n.T"], "position": ["n.X", "n.Y", "n.Z"], "uv": ["n.U", "n.V"], "geo_normal": ["n.X", "n.Y", "n.Z"], "sh_normal": ["n.X", "n.Y", "n.Z"],
            "dp_du": ["n.X", "n.Y", "n.Z"], "dp_dv": ["n.X", "n.Y", "n.Z"], "prim_index": ["n.I"], "shape_index": ["n.I"]}
    assert tuple(want) == mi.AOV_TYPES == aref.TYPES
    for typ, names in want.items():
        assert mi.aov_channels("n:" + typ) == names, typ
    allnine = mi.aov_channels(aref.ALL_NINE)
    assert allnine == aref.channel_names(aref.ALL_NINE) and len(allnine) == 20
    assert allnine == ["d.T", "p.X", "p.Y", "p.Z", "u.U", "u.V", "g.X", "g.Y", "g.Z", "s.X", "s.Y", "s.Z", "a.X", "a.Y", "a.Z", "b.X", "b.Y", "b.Z", "i.I", "h.I"]
    # string::tokenize with its default delimiters ", " (include/mitsuba/core/string.h:104-106): commas, blanks and runs of them; empty tokens are dropped
    assert mi.aov_channels("dd:depth, nn:sh_normal") == mi.aov_channels("dd:depth nn:sh_normal") == mi.aov_channels(" ,dd:depth,, nn:sh_normal, ") == ["dd.T", "nn.X", "nn.Y", "nn.Z"]
    assert mi.aov_channels("a::depth") == ["a.T"]      # ... and so are the empty parts of a token split at ':'
    assert mi.aov_channels("a:depth,b:depth,a:position") == ["a.T", "b.T", "a.X", "a.Y", "a.Z"]      # a type may repeat, the order is the spec's
    assert mi.aov_channels("") == [] and mi.aov_channels(" , ") == []
    assert mi.aov_channels("my.depth:depth") == ["my.depth.T"]


def test_parse_through_the_c_abi(mi):
    L = mi._lib()
    types, nt, nc = np.full(16, -7, np.int32), C.c_int(-1), C.c_int(-1)
    buf = C.create_string_buffer(256)
    assert L.dtof_aov_parse(aref.ALL_NINE.encode(), types.ctypes.data, 16, C.byref(nt), buf, 256, C.byref(nc)) == OK
    assert (nt.value, nc.value) == (9, 20) and types[:9].tolist() == list(range(9)) and (types[9:] == -7).all()
    assert buf.raw.split(b"\0")[:20] == [n.encode() for n in aref.channel_names(aref.ALL_NINE)]
    assert L.dtof_aov_parse(b"a:uv,b:depth", None, 0, C.byref(nt), None, 0, C.byref(nc)) == OK and (nt.value, nc.value) == (2, 3)      # counting only
    assert L.dtof_aov_parse(b"a:uv,b:depth", types.ctypes.data, 1, C.byref(nt), None, 0, C.byref(nc)) == INVALID and b"2 types" in L.dtof_last_error()
    assert L.dtof_aov_parse(b"a:uv,b:depth", None, 0, C.byref(nt), buf, 8, C.byref(nc)) == INVALID and b"bytes" in L.dtof_last_error()
    assert L.dtof_aov_parse(None, None, 0, C.byref(nt), None, 0, C.byref(nc)) == INVALID
    # more channels than a film holds still parse: the cap is the film's
    many = ",".join("p%d:position" % i for i in range(12))
    assert len(mi.aov_channels(many)) == 36


def test_refusal_messages(mi):
    cases = {"x:albedo": r'"albedo" is not supported.*eval_diffuse_reflectance', "x:boundary_test": r'"boundary_test" is not supported',
             "x:duv_dx": r'"duv_dx" is not supported.*ray differentials', "x:duv_dy": r'"duv_dy" is not supported.*ray differentials',
             "x:foo": r'^Invalid AOV type "foo"!$', "a:depth,b:Depth": r'^Invalid AOV type "Depth"!$',
             "depth": r'Invalid AOV specification "depth": require <name>:<type> pair', ":depth": r'require <name>:<type> pair', "a:": r'require <name>:<type> pair',
             "a:b:depth": r'Invalid AOV specification "a:b:depth"', "a:depth;b:uv": r'Invalid AOV specification'}
    for spec, pattern in cases.items():
        with pytest.raises(mi.DtofError, match=pattern):
            mi.aov_channels(spec)
    L = mi._lib()
    nt, nc = C.c_int(0), C.c_int(0)
    assert L.dtof_aov_parse(b"x:albedo", None, 0, C.byref(nt), None, 0, C.byref(nc)) == INVALID


FULL = ",".join("p%d:position" % i for i in range(10)) + ",d:depth"      # 31 channels: the whole cell


def test_refusals_that_need_no_device(mi):
    L = mi._lib()
    sc = mi.load_file(WALL, resx=8, resy=8)
    SENT = 123.25
    out = np.full((40, 64), SENT)
    st = mi._Stats()
    depth = np.asarray([0], np.int32)

    def render(scene=sc._h, n_passes=1, types=depth, n=None, planes=out.ctypes.data):
        return L.dtof_render_aovs(scene, 0, 4, n_passes, None if types is None else types.ctypes.data, len(types) if n is None else n, 1, planes, C.byref(st))

    lanes12, values = np.full((4, 12), SENT, np.float32), np.full((4, 40), SENT, np.float32)

    def sample(scene=sc._h, types=depth, n=None, a=lanes12.ctypes.data, b=values.ctypes.data):
        return L.dtof_sample_aov_lanes(scene, 0, 4, None if types is None else types.ctypes.data, len(types) if n is None else n, 0, 4, a, b)

    t32 = np.asarray([1] * 10 + [2], np.int32)      # 32 channels
    t31 = np.asarray([1] * 10 + [0], np.int32)
    cases = {"null scene": lambda: render(scene=None), "null output": lambda: render(planes=None), "0 passes": lambda: render(n_passes=0),
             "null types": lambda: render(types=None, n=1), "no types": lambda: render(n=0), "type 9": lambda: render(types=np.asarray([9], np.int32)),
             "type -1": lambda: render(types=np.asarray([0, -1], np.int32)), "32 channels": lambda: render(types=t32),
             "lanes: null scene": lambda: sample(scene=None), "lanes: null lanes": lambda: sample(a=None), "lanes: null values": lambda: sample(b=None),
             "lanes: no types": lambda: sample(n=0), "lanes: type 9": lambda: sample(types=np.asarray([9], np.int32)), "lanes: 32 channels": lambda: sample(types=t32)}
    for name, f in cases.items():
        assert f() == INVALID, (name, L.dtof_last_error())
        assert len(L.dtof_last_error()) > 0, name
    assert render(types=t32) == INVALID and b"at most 31 channels" in L.dtof_last_error()
    assert (out == SENT).all() and (lanes12 == SENT).all() and (values == SENT).all()      # no refused call wrote
    assert len(mi.aov_channels(FULL)) == 31 and mi._aov_parse(FULL)[0].tolist() == t31.tolist()
    with pytest.raises(mi.DtofError, match="at most 31 channels"):
        sc.render_aovs(FULL + ",e:depth")
    with pytest.raises(mi.DtofError, match="No AOVs were specified"):
        sc.render_aovs("")
    assert sc.aovs is None
    with pytest.raises(mi.DtofError, match="no \"aov\" integrator"):
        sc.render_aovs()
    with pytest.raises(mi.DtofError, match="aov.*scene file.*render_aovs"):      # a property dictionary cannot carry the nested plugin
        sc.set_integrator({"type": "aov", "aovs": "d:depth"})
    with pytest.raises(mi.DtofError, match="render_aovs"):
        mi.Integrator({"type": "aov"})


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_render_aovs.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_int, vp, vp]
L.dtof_sample_aov_lanes.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_uint64, C.c_uint64, vp, vp]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
types = (C.c_int32 * 2)(0, 1)
out = (C.c_double * (5 * 64))(*([7.0] * (5 * 64)))
lanes, vals = (C.c_float * 48)(*([7.0] * 48)), (C.c_float * 16)(*([7.0] * 16))
print(L.dtof_render_aovs(h, 0, 4, 1, types, 2, 1, out, None), L.dtof_render_aovs(h, 0, 4, 2, types, 1, 0, out, None),
      L.dtof_sample_aov_lanes(h, 0, 4, types, 2, 0, 4, lanes, vals), int(all(x == 7.0 for x in list(out) + list(lanes) + list(vals))))
"""


def test_compute_entries_fail_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), WALL], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP), str(HIP), str(HIP), "1"], r.stdout


def test_header_declares_and_library_exports_the_entries(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    lib = C.CDLL(mi.lib_path())
    for name in ("dtof_aov_parse", "dtof_scene_get_aovs", "dtof_render_aovs", "dtof_sample_aov_lanes"):
        assert re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr), name
        assert hasattr(lib, name), name
        comment = hdr[:hdr.index("int " + name)].rsplit("/*", 1)[1]
        assert "src/integrators/aov.cpp:" in comment, name
    for i, typ in enumerate(mi.AOV_TYPES):
        assert re.search(r"#define DTOF_AOV_%s\s+%d\b" % (typ.upper(), i), hdr), typ
    assert re.search(r"#define DTOF_AOV_MAX_CHANNELS\s+31\b", hdr)


def _wrap(xml, spec="dd:depth,nn:sh_normal", inner=None, copies=1, wrapper="aov"):
    """the scene's integrator inside <integrator type="aov">: `copies` of it, or of `inner`"""
    m = re.search(r"<integrator type=\"dopplertofpath\">.*?</integrator>", xml, re.S)
    assert m
    body = m.group(0) if inner is None else inner
    own = '<string name="aovs" value="%s" />' % spec if spec is not None else ""
    return (xml[:m.start()] + '<integrator type="%s">' % wrapper + own + "".join(body.replace("<integrator", '<integrator name="nested_%d"' % i, 1) for i in range(copies))
            + "</integrator>" + xml[m.end():])


def test_loader_takes_the_aov_wrapper(mi):
    xml = open(WALL).read()
    params = dict(resx=16, resy=16, max_depth=3)
    plain, wrapped = mi.load_string(xml, **params), mi.load_string(_wrap(xml), **params)
    assert wrapped.info() == plain.info() and plain.info()["max_depth"] == 3      # the nested plugin is the scene's integrator, with all its properties
    assert wrapped.aovs == "dd:depth,nn:sh_normal" and plain.aovs is None
    # the spec survives $parameters
    templ = _wrap(xml, spec="$what:depth, n:$typ").replace('<default name="resx"', '<default name="typ" value="sh_normal" /><default name="resx"', 1)
    assert mi.load_string(templ, what="zz", **params).aovs == "zz:depth, n:sh_normal"
    assert mi.load_string(templ, what="zz", typ="uv", **params).aovs == "zz:depth, n:uv"
    with pytest.raises(mi.DtofError, match='Invalid AOV type "nope"!'):      # the constructor's checks run at load time
        mi.load_string(templ, what="zz", typ="nope", **params)
    with pytest.raises(mi.DtofError, match='"albedo" is not supported'):
        mi.load_string(_wrap(xml, spec="a:albedo"), **params)
    with pytest.raises(mi.DtofError, match='require <name>:<type> pair'):
        mi.load_string(_wrap(xml, spec="depth"), **params)
    with pytest.raises(mi.DtofError, match="aov.*2 nested integrators"):
        mi.load_string(_wrap(xml, copies=2), **params)
    with pytest.raises(mi.DtofError, match="aov.*none was given"):
        mi.load_string(_wrap(xml, copies=0), **params)
    with pytest.raises(mi.DtofError, match='Property "aovs" has not been specified'):
        mi.load_string(_wrap(xml, spec=None), **params)
    with pytest.raises(mi.DtofError, match="aov"):      # the wrapper queries nothing but `aovs` and its child
        mi.load_string(_wrap(xml).replace('<integrator type="aov">', '<integrator type="aov"><integer name="max_depth" value="2" />'), **params)
    for plugin in ("path", "velocity"):
        sc = mi.load_string(_wrap(xml, inner='<integrator type="%s"></integrator>' % plugin), **params)
        assert sc.aovs == "dd:depth,nn:sh_normal"
    with pytest.raises(mi.DtofError, match='unsupported integrator plugin "volpath"'):
        mi.load_string(_wrap(xml, inner='<integrator type="volpath"></integrator>'), **params)
    # `moment` inside `aov` and the reverse
    inner_m = re.search(r"<integrator type=\"dopplertofpath\">.*?</integrator>", xml, re.S).group(0)
    with pytest.raises(mi.DtofError, match=r'aov: a nested "moment" integrator is not supported'):
        mi.load_string(_wrap(xml, inner='<integrator type="moment">' + inner_m + "</integrator>"), **params)
    with pytest.raises(mi.DtofError, match=r'moment: a nested "aov" integrator is not supported'):
        mi.load_string(_wrap(xml, spec=None, wrapper="moment", inner='<integrator type="aov"><string name="aovs" value="d:depth" />' + inner_m + "</integrator>"), **params)
    with pytest.raises(mi.DtofError, match=r'aov: a nested "aov" integrator is not supported'):
        mi.load_string(_wrap(xml, inner='<integrator type="aov"><string name="aovs" value="d:depth" />' + inner_m + "</integrator>"), **params)


# (scene, -D parameters, spp, integrator override, open): the shapes of test_aov_gpu's per-lane cases
LANE_SHAPES = {"wall": ("cornell_wall.xml", dict(resx=16, resy=16), 4, None, False), "spheres": ("cornell_spheres.xml", dict(resx=16, resy=16), 2, None, False),
               "cylinders": ("cornell_cylinders.xml", dict(resx=16, resy=16), 2, None, False), "disk": ("cornell_disk.xml", dict(resx=16, resy=16), 2, None, False),
               "domino_small": ("domino_small.xml", dict(resx=32, resy=32), 2, None, False), "open_veils": ("open_veils.xml", dict(resx=16, resy=16), 2, None, True),
               "thinlens": ("cornell_thinlens.xml", dict(resx=16, resy=16), 2, None, False),
               "wall_path": ("cornell_wall.xml", dict(resx=16, resy=16), 4, {"type": "path", "max_depth": 4}, False)}


@pytest.mark.parametrize("case", list(LANE_SHAPES))
def test_oracle_conditions_at_the_gpu_shapes(orc, case):
    """aov_ref on the oracle alone: (a) every hit lies in front of far_clip - near_clip, (b) the open scene has hits and misses, and the values have the documented
    form -- so a GPU run cannot fail on a shape the oracle's query does not cover"""
    scene, params, spp, override, is_open = LANE_SHAPES[case]
    osc = orc.Scene(os.path.join(SCENES, scene), params)
    lanes, values, out25, ids, _ = aref.expected_lanes(orc, osc, aref.ALL_NINE, 3, spp, override)      # asserts (a)
    hit = ids[:, 0] >= 0
    w, h = osc.size
    assert values.shape == (w * h * spp, 20) and hit.any()
    if is_open:
        assert hit.any() and (~hit).any(), "the open scene must have hits and misses among the lanes"
    assert not values[~hit].any() and not np.signbit(values[~hit]).any()      # a miss is +0 in every channel
    known = [c for c in range(20) if c not in (4, 5, 19)]
    assert np.isfinite(values[hit][:, known]).all() and np.isnan(values[hit][:, [4, 5, 19]]).all()
    assert (values[hit, 0] > 0).all() and (values[hit, 18] == ids[hit, 2]).all()
    n = values[hit][:, 6:9].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5
    rec = aref.shape_records(osc, ids)
    assert (rec[hit] >= 0).all() and (rec[~hit] == -1).all() and len(set(rec[hit])) > 1
    if case == "wall":      # the moving wall: two samples of one pixel see it at two depths, so the ray's time is exercised
        wall = [i for i, o in enumerate(osc.flat.objects) if o["kind"] == 1]
        assert len(wall) == 1
        depth, obj = values[:, 0].reshape(h * w, spp), ids[:, 0].reshape(h * w, spp)
        on_wall = (obj == wall[0]).all(axis=1)
        assert on_wall.any() and (depth[on_wall].max(axis=1) > depth[on_wall].min(axis=1)).any()
        assert len(set(lanes["time"].tolist())) > 1


def test_command_line_parses_aovs(mi, capsys):
    from mitsuba3dopplertof_amd import __main__ as cli
    args = cli.parser().parse_args(["scene.xml", "--aovs", "dd:depth,nn:sh_normal", "--passes", "3", "--spp", "8", "-o", "a.npz"])
    assert (args.aovs, args.passes, args.spp, args.output) == ("dd:depth,nn:sh_normal", 3, 8, "a.npz") and not args.moments
    assert cli.parser().parse_args(["scene.xml"]).aovs is None
    refused = {"--moments": [WALL, "--aovs", "d:depth", "--moments"], "--velocity-map": [WALL, "--aovs", "d:depth", "--velocity-map", "0,0.25"],
               "stripes": [WALL, "--aovs", "d:depth", "--stripes", "4"], "float64": [WALL, "--aovs", "d:depth", "--film", "float64"],
               "--offsets": [WALL, "--aovs", "d:depth", "--offsets", "0,0.25"], "--variants": [WALL, "--aovs", "d:depth", "--variants", "0:0"],
               ".npz": [WALL, "--aovs", "d:depth", "-o", "a.npy"], "at least 1": [WALL, "--aovs", "d:depth", "--passes", "0"],
               'Invalid AOV type "foo"!': [WALL, "--aovs", "d:foo"], '"albedo" is not supported': [WALL, "--aovs", "a:albedo"], "names no channel": [WALL, "--aovs", ","],
               "belong to --moments": [WALL, "--passes", "2"]}
    for what, argv in refused.items():
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and what in capsys.readouterr().err, what


def test_command_line_refuses_a_multi_gpu_launch_before_the_scene_loads(mi, monkeypatch, capsys):
    from mitsuba3dopplertof_amd import __main__ as cli
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        cli.main(["/nonexistent/scene.xml", "--aovs", "d:depth"])      # refused before the scene file is looked at
    assert e.value.code == 2 and "single-GPU" in capsys.readouterr().err
