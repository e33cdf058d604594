"""Host logic of the product (no GPU): the C++ scene.xml loader against the oracle's independent Python
restatement (bit-exact float32 exports), constructor parity, the reference loader's error behaviour, and that
the C-ABI library loads and exports every symbol include/dtof.h declares (no compute calls here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES


def _export_all(sc):
    return [sc.export(k) for k in range(4)]


def _oracle_all(fs):
    obj = np.concatenate([np.concatenate([np.asarray(o["key_time"], np.float32), np.asarray(o["key"], np.float32).reshape(-1)])
                          for o in fs.objects]) if fs.objects else np.zeros(0, np.float32)
    shp = np.concatenate([np.concatenate([s["to_world"].reshape(-1), s["to_object"].reshape(-1)]) for s in fs.shapes])
    se = fs.sensor
    sen = np.concatenate([se["to_world"].reshape(-1), np.array([se["x_fov"], se["near_clip"], se["far_clip"],
                                                                 se["shutter_open"], se["shutter_close"],
                                                                 se["kind"], se["aperture_radius"], se["focus_distance"]], np.float32)])
    em = np.concatenate([np.concatenate([e["position"], e["intensity"]]) for e in fs.emitters]) if fs.emitters else np.zeros(0, np.float32)
    return [obj.astype(np.float32), shp.astype(np.float32), sen.astype(np.float32), em.astype(np.float32)]


@pytest.mark.parametrize("xml,params", [
    ("cornell_boxes.xml", dict(resx=64, resy=48)),
    ("cornell_wall.xml", dict()),
    ("domino_small.xml", dict()),
    ("domino.xml", dict()),
    ("cornell_thinlens.xml", dict()),
])
def test_loader_matches_oracle_loader_bit_exact(mi, orc, xml, params):
    path = os.path.join(SCENES, xml)
    sc = mi.load_file(path, **params)
    from oracle import scene_xml
    fs = scene_xml.load(path, params)
    for got, exp in zip(_export_all(sc), _oracle_all(fs)):
        assert got.shape == exp.shape
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    info = sc.info()
    assert (info["n_shapes"], info["n_groups"], info["n_objects"], info["n_emitters"]) == \
        (len(fs.shapes), len(fs.groups), len(fs.objects), len(fs.emitters))
    assert info["crop_width"] == fs.sensor["crop_w"] and info["crop_height"] == fs.sensor["crop_h"]


REFERENCE_SCENE = "/root/reference/configs_example/scene.xml"


@pytest.mark.skipif(not os.path.exists(REFERENCE_SCENE), reason="build container only: reads the reference's own example scene (absent on the GPU box)")
def test_the_reference_example_scene_loads_unchanged(mi, orc):
    """north_star: "a scene.xml that names dopplertofpath / correlated renders unchanged".  The reference's own configs_example/scene.xml goes
    through the product loader and through the oracle loader AS IT IS, and both give the scene the generated scenes/cornell_boxes.xml
    describes -- same shapes, transforms, keyframes, materials, light and camera, bit for bit (the generated file only sets a smaller
    default sample count and film size, overridden here)."""
    from oracle import scene_xml
    text = open(REFERENCE_SCENE).read()
    assert 'type="dopplertofpath"' in text and 'type="correlated"' in text
    try:
        ref_sc = mi.load_file(REFERENCE_SCENE)
    except mi.DtofError as e:                                        # an unused <default> is fine; an unused loader parameter is not
        raise AssertionError("the reference's example scene does not load unchanged: %s" % e)
    ref_fs = scene_xml.load(REFERENCE_SCENE, {})
    w, h = ref_sc.size
    own = os.path.join(SCENES, "cornell_boxes.xml")
    own_sc = mi.load_file(own, resx=w, resy=h)
    own_fs = scene_xml.load(own, dict(resx=w, resy=h))
    for a, b in zip(_export_all(ref_sc), _export_all(own_sc)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for a, b in zip(_oracle_all(ref_fs), _oracle_all(own_fs)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ri, oi = ref_sc.info(), own_sc.info()
    for k in ("n_shapes", "n_groups", "n_objects", "n_emitters", "n_triangles", "time", "w_g", "hetero_frequency", "antithetic_shift", "wave_type", "time_sampling",
              "path_correlation_depth", "max_depth", "time_correlate_number", "path_correlate_number"):
        assert ri[k] == oi[k], (k, ri[k], oi[k])
    assert ri["sample_count"] == 1024                                # the example file's sampler block says so


def test_transform_ops_compose_like_the_reference(mi):
    """ops left-multiply (xml.cpp:902-1007): translate after rotate after scale; lookat; 3x3 matrix."""
    from oracle import scene_xml
    xml = """<scene version="3.0.0">
      <integrator type="dopplertofpath"/>
      <sensor type="perspective"><float name="fov" value="35"/><string name="fov_axis" value="y"/>
        <transform name="to_world"><lookat origin="1, 2, 3" target="0, 0.5, -1" up="0, 1, 0"/></transform>
        <sampler type="correlated"/><film type="hdrfilm"><integer name="width" value="40"/><integer name="height" value="20"/>
        <rfilter type="box"/></film></sensor>
      <shape type="rectangle"><transform name="to_world"><scale x="2" y="3" z="1"/><rotate x="0.3" y="1" z="0.2" angle="33"/>
        <translate x="1" y="-2" z="0.5"/></transform></shape>
      <shape type="cube"><boolean name="flip_normals" value="true"/><transform name="to_world">
        <matrix value="0 1 0 0 0 2 0 0 0 3"/><translate value="0.25"/></transform>
        <bsdf type="diffuse"><rgb name="reflectance" value="0.2"/></bsdf></shape>
      <emitter type="point"><point name="position" x="1" y="2" z="3"/><spectrum name="intensity" value="7"/></emitter>
    </scene>""".replace('value="0 1 0 0 0 2 0 0 0 3"', 'value="0 1 0 1 0 0 0 0 2"')
    sc = mi.load_string(xml)
    fs = scene_xml.load(xml, {}, is_string=True)
    for got, exp in zip(_export_all(sc), _oracle_all(fs)):
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert sc.size == (40, 20)
    assert sc.export(3).tolist() == [1, 2, 3, 7, 7, 7]


def test_constructor_parameters_match_oracle(mi, orc):
    path = os.path.join(SCENES, "cornell_boxes.xml")
    cases = [None,
             dict(type="dopplertofpath", max_depth=7, w_g=24.0, hetero_frequency=0.5, hetero_offset=0.25, wave_function_type="triangular",
                  time_sampling_method="stratified", path_correlation_depth=3, rr_depth=3),
             dict(type="dopplertofpath", w_s=30.002, g_1=0.7, g_0=0.3, low_frequency_component_only=False, time_sampling_method="antithetic_mirror"),
             dict(type="dopplertofpath", sensor_phase_offset=0.3, time=0.002, use_stratified_sampling_for_each_interval=False)]
    sc = mi.load_file(path)
    osc = orc.Scene(path)
    for c in cases:
        if c is not None:
            sc.set_integrator(c)
        pd = osc.params(integrator=c) if c is not None else osc.params()
        info = sc.info()
        for ok, ik in [("time", "time"), ("w_g_mhz", "w_g"), ("g_1", "g_1"), ("g_0", "g_0"), ("w_s_mhz", "w_s"), ("phase_offset", "phase_offset"),
                       ("hetero_frequency", "hetero_frequency"), ("antithetic_shift", "antithetic_shift")]:
            assert np.float32(pd[ok]).view(np.uint32) == np.float32(info[ik]).view(np.uint32), (c, ok)
        for ok, ik in [("wave_type", "wave_type"), ("low_frequency_component_only", "low_frequency_component_only"),
                       ("time_sampling", "time_sampling"), ("stratify_each_interval", "stratify_each_interval"),
                       ("path_correlation_depth", "path_correlation_depth"), ("max_depth", "max_depth"), ("rr_depth", "rr_depth"),
                       ("time_correlate_number", "time_correlate_number"), ("path_correlate_number", "path_correlate_number")]:
            assert int(pd[ok]) == int(info[ik]), (c, ok)


def test_error_behaviour_mirrors_the_reference_loader(mi):
    path = os.path.join(SCENES, "cornell_boxes.xml")
    text = open(path).read()
    with pytest.raises(mi.DtofError, match="undefined parameter"):
        mi.load_string(text.replace("$resx", "$nosuchparam"))
    with pytest.raises(mi.DtofError, match="missing version"):
        mi.load_string(text.replace(' version="3.0.0"', ""))
    with pytest.raises(mi.DtofError, match="unsupported integrator plugin"):
        mi.load_string(text.replace('type="dopplertofpath"', 'type="volpath"'))
    with pytest.raises(mi.DtofError, match="unsupported sampler plugin"):
        mi.load_string(text.replace('type="correlated"', 'type="ldsampler"'))
    with pytest.raises(mi.DtofError, match="unreferenced property"):   # `independent` has no time_correlate_number (independent.cpp:70-74)
        mi.load_string(text.replace('type="correlated"', 'type="independent"'))
    with pytest.raises(mi.DtofError, match="unreferenced property"):
        mi.load_string(text.replace('<float name="w_g" value="30" />', '<float name="w_g" value="30" /><float name="bogus" value="1" />'))
    with pytest.raises(mi.DtofError, match="wrong type"):
        mi.load_string(text.replace('<integer name="max_depth" value="$max_depth" />', '<float name="max_depth" value="4.0" />'))
    with pytest.raises(mi.DtofError, match="unknown wave_function_type"):
        mi.load_string(text, wave_function_type="sawtooth")
    with pytest.raises(mi.DtofError, match="unknown object"):
        mi.load_string(text.replace('<ref id="FloorBSDF" />', '<ref id="NoSuchBSDF" />'))
    with pytest.raises(mi.DtofError, match="strictly monotonically increasing"):
        mi.load_string(text.replace('<transform time="0.0015">', '<transform time="0">'))
    with pytest.raises(mi.DtofError, match="max_depth"):
        mi.load_string(text, max_depth=-3)
    with pytest.raises(mi.DtofError):
        mi.load_file(os.path.join(SCENES, "does_not_exist.xml"))
    with pytest.raises(mi.DtofError, match="unsupported"):
        mi.load_dict({"type": "volpath"})
    sc = mi.load_string(text)
    with pytest.raises(mi.DtofError, match="rr_depth"):
        sc.set_integrator(dict(type="dopplertofpath", rr_depth=0))
    with pytest.raises(mi.DtofError, match="out of bounds"):
        sc.render(spp=2, sensor=3)


def test_capi_exports_every_declared_symbol(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    names = set(re.findall(r"\b(dtof_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 28 and {"dtof_ray_intersect", "dtof_flat_query", "dtof_tree_query"} <= names
    lib = ctypes.CDLL(mi.lib_path())
    for n in sorted(names):
        assert hasattr(lib, n), n
    lib.dtof_version.restype = ctypes.c_char_p
    assert b"dopplertofpath" in lib.dtof_version()


def test_the_exported_dtof_symbols_are_exactly_the_declared_functions(mi):
    """Both ways, from the symbol table: a function of include/dtof.h that a move between the library's translation units left `static` is missing here, and
    nothing named dtof_* leaves the library undeclared.  The header does not declare the two traversal-counter entries of the DTOF_TRAVERSAL_STATS build
    (tools and tests declare them where they use them): libdtof_stats.so exports the header's set and those two, libdtof.so the header's set alone."""
    import subprocess
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dtof.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dtof_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 28 and not any(n.startswith("dtof_debug_") for n in declared)
    stats_only = {"dtof_debug_traversal_stats", "dtof_debug_traversal_stats_n"}
    stats_lib = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_stats.so")
    assert os.path.exists(stats_lib), "libdtof_stats.so is not built (make -C mitsuba3dopplertof_amd/csrc stats; build() makes it)"
    for path, expected in ((os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof.so"), declared), (stats_lib, declared | stats_only)):
        table = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {m.group(1) for m in re.finditer(r"^[0-9a-f]+ T (dtof_\w+)$", table, re.M)}
        assert exported == expected, (path, sorted(expected - exported), sorted(exported - expected))


def test_plugin_shims_export_the_discovery_symbols(mi):
    """MI_EXPORT_PLUGIN's two extern "C" symbols with the reference's strings (dopplertofpath.cpp:330, correlated.cpp:195)."""
    for so, name, descr in [("dopplertofpath", b"DopplerToFPathIntegrator", b"Doppler ToF Path Tracer integrator"),
                            ("correlated", b"CorrelatedSampler", b"Independent Sampler")]:
        lib = ctypes.CDLL(os.path.join(ROOT, "mitsuba3dopplertof_amd", "plugins", so + ".so"))
        lib.plugin_name.restype = ctypes.c_char_p
        lib.plugin_descr.restype = ctypes.c_char_p
        assert lib.plugin_name() == name and lib.plugin_descr() == descr


def test_no_cpu_fallback_in_the_product_path():
    """The product may not import or link anything under oracle/; outside tests/ only bench.py (cpu_baseline leg) and
    __graft_entry__.smoke() may touch it."""
    for sub in ("mitsuba3dopplertof_amd", "tools", "scenes", "include"):
        for base, _dirs, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".py", ".cpp", ".hip", ".h", ".sh", "Makefile")):
                    text = open(os.path.join(base, f), errors="replace").read()
                    assert "import oracle" not in text and "from oracle" not in text and "dtof_oracle" not in text, os.path.join(sub, f)
    bench = open(os.path.join(ROOT, "bench.py")).read()
    assert bench.count("from oracle import") == 1 and bench.split("from oracle import")[0].rsplit("\ndef ", 1)[1].startswith("cpu_baseline(")


def test_header_is_plain_c_and_links_from_a_c_program(mi, tmp_path):
    """The boundary is a C ABI: include/dtof.h compiles as strict C99 and a C program linked against libdtof.so can load a
    scene and read it back (host-side calls only -- no GPU here)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "dtof.h"
int main(int argc, char **argv) {
    dtof_scene *sc = NULL; dtof_scene_info info; const char *n[1] = { "resx" }, *v[1] = { "40" };
    if (argc < 2) return 2;
    if (dtof_scene_load_file(argv[1], n, v, 1, &sc) != 0) { fprintf(stderr, "%s\n", dtof_last_error()); return 3; }
    if (dtof_scene_get_info(sc, &info) != 0) return 4;
    printf("%d %d %u %s\n", info.crop_width, info.crop_height, info.n_objects, dtof_version());
    if (dtof_scene_load_file("/nonexistent.xml", NULL, NULL, 0, &sc) == 0 || strlen(dtof_last_error()) == 0) return 5;
    dtof_scene_destroy(sc);
    return 0;
}
''')
    libdir = os.path.dirname(mi.lib_path())
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", libdir, "-ldtof", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe), os.path.join(SCENES, "cornell_boxes.xml")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    w, h, nobj = out.stdout.split()[:3]
    assert (int(w), int(h), int(nobj)) == (40, 256, 7)


def test_half_float_node_boxes_round_outward(tmp_path):
    """DNode16 (round 5): the builder rounds a child box's minima DOWN and its maxima UP to IEEE halves (csrc/dtof_half.h), so that the half box contains the float box and the
    hits of the ray kernels that walk it cannot change.  A C++ harness over 4 M random floats of every magnitude a box can have (|x| <= 65 000) plus the edge cases: the
    result is on the right side, equal to x whenever x is a half, and TIGHT -- one half nearer to x is on the wrong side."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "half.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <random>
#include "dtof_half.h"
static double h2d(uint16_t h) {   // exact value of a binary16
    const int e = (h >> 10) & 31, m = h & 1023; const double s = (h & 0x8000) ? -1.0 : 1.0;
    return s * (e == 0 ? std::ldexp((double) m, -24) : std::ldexp((double) (1024 + m), e - 25));
}
static uint16_t next_up(uint16_t h) { return (h & 0x7fff) == 0 ? 0x0001 : (h & 0x8000) ? (uint16_t) (h - 1) : (uint16_t) (h + 1); }      // the next half above (towards +inf)
static uint16_t next_down(uint16_t h) { return (h & 0x7fff) == 0 ? 0x8001 : (h & 0x8000) ? (uint16_t) (h + 1) : (uint16_t) (h - 1); }
int main() {
    std::mt19937 rng(7); long n = 0, bad = 0;
    auto check = [&](float x) {
        for (int up = 0; up < 2; ++up) {
            const uint16_t h = dtof::half_toward(x, up); const double y = h2d(h); ++n;
            if ((h & 0x7c00) == 0x7c00) { ++bad; continue; }                                  // never an infinity / NaN
            if (up ? y < (double) x : y > (double) x) { ++bad; continue; }                     // the right side
            if (y != (double) x) {                                                           // tight: the neighbouring half on x's side lies beyond x
                const double z = h2d(up ? next_down(h) : next_up(h));
                if (up ? z >= (double) x : z <= (double) x) ++bad;
            }
        }
    };
    for (int i = 0; i < 4000000; ++i) { uint32_t u = rng(); float x; memcpy(&x, &u, 4); if (std::fabs(x) <= 65000.f) check(x); }
    for (int i = 0; i < 65536; ++i) { const uint16_t h = (uint16_t) i; if ((h & 0x7c00) == 0x7c00) continue; const float x = (float) h2d(h); if (std::fabs(x) <= 65000.f) { check(x); if (dtof::half_toward(x, false) != (x == 0.f ? 0 : h) || dtof::half_toward(x, true) != (x == 0.f ? 0 : h)) ++bad; } }
    const float edge[] = { 0.f, -0.f, 1.f, -1.f, 65000.f, -65000.f, 6.1035156e-5f, 6.1e-5f, 5.9604645e-8f, 3e-8f, -3e-8f, 1e-30f, -1e-30f, 2047.9999f, 0.33333334f, 1.0004883f, 1.0004884f };
    for (float x : edge) check(x);
    printf("%ld %ld\n", n, bad);
    return bad != 0;
}
''')
    exe = tmp_path / "half"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    n, bad = (int(v) for v in out.stdout.split())
    assert n > 1000000 and bad == 0


def test_plugin_objects_validate_like_the_reference_constructors(mi):
    """dtof_integrator_create / dtof_sampler_plugin_create = PluginManager::create_object -> new T(props): unknown plugins,
    unknown or mistyped properties and out-of-range values fail at construction (no scene, no GPU involved)."""
    ok = mi.load_dict(dict(type="dopplertofpath", max_depth=4, w_g=30.0, time_sampling_method="antithetic_mirror"))
    assert ok._h.value
    for bad, msg in ((dict(type="volpath"), "unsupported plugin type"),
                     (dict(type="dopplertofpath", bogus=1), "unreferenced property"),
                     (dict(type="dopplertofpath", max_depth=4.0), "wrong type"),
                     (dict(type="dopplertofpath", rr_depth=0), "rr_depth"),
                     (dict(type="dopplertofpath", wave_function_type="sawtooth"), "unknown wave_function_type"),
                     (dict(type="path", max_depth=-2), "max_depth")):
        with pytest.raises(mi.DtofError, match=msg):
            mi.load_dict(bad)
    L, h = mi._lib(), ctypes.c_void_p()
    args = mi._plugin_args(dict(type="timestratified", sample_count=16, jitter=False))
    assert L.dtof_sampler_plugin_create(*(args + (ctypes.byref(h),))) == 0 and h.value
    L.dtof_sampler_plugin_destroy(h)
    args = mi._plugin_args(dict(type="independent", time_correlate_number=2))
    assert L.dtof_sampler_plugin_create(*(args + (ctypes.byref(h),))) != 0 and b"unreferenced property" in L.dtof_last_error()


def test_non_finite_geometry_is_rejected_not_crashed(mi):
    """Found by tests/dev/gpu_fuzz.py: a matrix entry that overflows float32 used to reach the BVH builder as inf / NaN and crash
    it; non-finite vertices, transforms and animation keys are load errors now."""
    text = open(os.path.join(SCENES, "cornell_boxes.xml")).read()
    import re
    m = re.search(r'<matrix value="([^"]+)"', text[text.index('type="cube"'):])
    first = m.group(1).split()
    for bad in ("1e39", "nan", "-inf"):
        broken = text.replace(m.group(1), " ".join([bad] + first[1:]), 1)
        assert broken != text
        with pytest.raises(mi.DtofError, match="non-finite"):
            mi.load_string(broken)
    wall = open(os.path.join(SCENES, "cornell_wall.xml")).read()
    i = wall.index("<animation")
    k = re.search(r'<translate[^>]*z="([^"]+)"', wall[i:]) or re.search(r'<matrix value="([^"]+)"', wall[i:])
    broken = wall[:i] + wall[i:].replace(k.group(1), "1e39" if " " not in k.group(1) else " ".join(["1e39"] + k.group(1).split()[1:]), 1)
    with pytest.raises(mi.DtofError, match="non-finite"):
        mi.load_string(broken)


def _write_include_scene(d, which="a"):
    """a Cornell-like scene split over files the way scene packs are: main.xml includes the geometry (a <scene> root, chosen by a $parameter),
    the sensor (an object root) and, from a <path> directory, the light; a texture is found through the same <path>; an <alias> renames a BSDF"""
    from scenes import make_scenes as ms
    os.makedirs(os.path.join(d, "assets"))
    ms.write_png(os.path.join(d, "assets", "checker.png"), [[(255, 0, 0), (0, 255, 0)], [(0, 0, 255), (255, 255, 255)]])
    sensor = ('<sensor type="perspective"><float name="fov" value="35"/><transform name="to_world"><lookat origin="0, 1, 5" target="0, 1, 0" up="0, 1, 0"/></transform>'
              '<sampler type="correlated"><integer name="sample_count" value="$spp"/></sampler>'
              '<film type="hdrfilm"><integer name="width" value="$res"/><integer name="height" value="$res"/><rfilter type="tent"/></film>'
              '<float name="shutter_close" value="0.0015"/></sensor>')
    light = '<emitter type="point"><point name="position" x="0" y="1.8" z="1"/><rgb name="intensity" value="$power"/></emitter>'
    bsdfs = ('<bsdf type="twosided" id="white"><bsdf type="diffuse"><rgb name="reflectance" value="0.7"/></bsdf></bsdf>'
             '<bsdf type="twosided" id="tex"><bsdf type="diffuse"><texture type="bitmap" name="reflectance"><string name="filename" value="checker.png"/></texture></bsdf></bsdf>')
    shapes = ('<shape type="rectangle" id="floor"><transform name="to_world"><rotate x="1" angle="-90"/><scale value="2"/></transform><ref id="floor_material"/></shape>'
              '<shape type="rectangle" id="back"><transform name="to_world"><scale value="2"/><translate z="-2" y="1"/></transform><ref id="tex"/></shape>')
    geometry = '<scene version="3.0.0"><default name="res" value="12"/>%s<alias id="white" as="floor_material"/>%s<include filename="light.xml"/></scene>' % (bsdfs, shapes)
    integrator = '<integrator type="dopplertofpath"><integer name="max_depth" value="3"/></integrator>'
    files = {"main.xml": '<scene version="3.0.0"><default name="spp" value="4"/><default name="which" value="%s"/><path value="assets"/>%s'
                         '<include filename="geometry_$which.xml"/><include filename="sensor.xml"/></scene>' % (which, integrator),
             "geometry_a.xml": geometry, "sensor.xml": sensor, os.path.join("assets", "light.xml"): light}
    for name, text in files.items():
        with open(os.path.join(d, name), "w") as f:
            f.write(text)
    flat = ('<scene version="3.0.0"><default name="spp" value="4"/><default name="res" value="12"/>%s%s%s%s%s</scene>'
            % (integrator, bsdfs.replace("checker.png", os.path.join(d, "assets", "checker.png")), shapes.replace("floor_material", "white"), light, sensor))
    return os.path.join(d, "main.xml"), flat


def test_include_alias_and_path_tags(mi, orc, tmp_path):
    """xml.cpp:608-628 (<alias>), :651-668 (<path>), :670-725 (<include>): a scene split over files loads to the same records as its flattened
    text, in both loaders; parameters cross file boundaries in both directions; the reference's error cases."""
    from oracle import scene_xml
    d = str(tmp_path / "pack")
    main, flat = _write_include_scene(d)
    for params in (dict(power="20"), dict(power="5", res=8, spp=2)):
        split, whole = mi.load_file(main, **params), mi.load_string(flat, **params)
        for a, b in zip(_export_all(split), _export_all(whole)):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert split.info() == whole.info() and np.array_equal(split.export(10), whole.export(10))       # texture table (the PNG found through <path>)
        fs = scene_xml.load(main, params)
        for got, exp in zip(_export_all(split), _oracle_all(fs)):
            assert got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
        assert split.info()["crop_width"] == (8 if "res" in params else 12)
    with pytest.raises(mi.DtofError, match="undefined parameter"):                        # $power has no default anywhere
        mi.load_file(main)
    with pytest.raises(ValueError, match="undefined parameter"):
        scene_xml.load(main, {})

    def both(text, match, name="bad.xml", params=None):
        p = os.path.join(d, name)
        with open(p, "w") as f:
            f.write(text)
        with pytest.raises(mi.DtofError, match=match):
            mi.load_file(p, **(params or {}))
        with pytest.raises(ValueError, match=match):
            scene_xml.load(p, params or {})
    both('<scene version="3.0.0"><include filename="nope.xml"/></scene>', 'included file ".*nope.xml" not found')
    both('<scene version="3.0.0"><include filename="loop.xml"/></scene>', "Exceeded <include> recursion limit of 15", name="loop.xml")
    both('<scene version="3.0.0"><include filename="sensor.xml" id="x"/></scene>', 'unexpected attribute "id" in element "include"', params=dict(spp=1, res=4))
    both('<scene version="3.0.0"><path value="no_such_dir"/></scene>', '<path>: folder ".*no_such_dir" not found')
    both('<scene version="3.0.0"><shape type="rectangle"><path value="assets"/></shape></scene>', "<path>: path can only be child of root")
    both('<scene version="3.0.0"><alias id="ghost" as="b"/></scene>', 'referenced id "ghost" not found')
    both('<scene version="3.0.0"><bsdf type="diffuse" id="a"/><bsdf type="diffuse" id="b"/><alias id="a" as="b"/></scene>', '"alias" has duplicate id "b"')


@pytest.mark.gpu
def test_included_scene_renders_like_its_flattened_text(mi, tmp_path):
    main, flat = _write_include_scene(str(tmp_path / "pack"))
    split, whole = mi.load_file(main, power="20"), mi.load_string(flat, power="20")
    a, b = split.sample_lanes(2, 4, 0, 12 * 12 * 4), whole.sample_lanes(2, 4, 0, 12 * 12 * 4)
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)), k
    assert (a["rgb"] != 0).any()


def test_bsdf_of_an_emitter_shape_keeps_its_reflectance(mi, orc):
    """Shape::Shape (src/render/shape.cpp:66-72): only the DEFAULT BSDF of an emitter shape is black (reflectance 0); a BSDF given in the file keeps
    its reflectance whether or not the shape emits -- paths that reach a light source go on from its surface"""
    def scene(bsdf, emitter):
        return ('<scene version="3.0.0"><sensor type="perspective"><film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="4"/></film></sensor>'
                '<shape type="rectangle">%s%s</shape></scene>'
                % (bsdf, '<emitter type="area"><rgb name="radiance" value="3"/></emitter>' if emitter else ""))
    given = '<bsdf type="diffuse"><rgb name="reflectance" value="0.3, 0.5, 0.7"/></bsdf>'
    black = '<bsdf type="diffuse"><rgb name="reflectance" value="0"/></bsdf>'
    rec = lambda xml: mi.load_string(xml).export(9)
    assert np.array_equal(rec(scene(given, True)), rec(scene(given, False)))
    assert np.array_equal(rec(scene("", True)), rec(scene(black, True))) and not np.array_equal(rec(scene("", True)), rec(scene("", False)))
    from oracle import scene_xml
    for bsdf, emitter, want in ((given, True, [0.3, 0.5, 0.7]), ("", True, [0, 0, 0]), ("", False, [0.5, 0.5, 0.5])):
        assert np.allclose(scene_xml.load(scene(bsdf, emitter), {}, is_string=True).shapes[0]["reflectance"], want)
        assert np.allclose(sorted(set(np.float32(want).tolist())), sorted(set(v for v in rec(scene(bsdf, emitter)).tolist() if v in np.float32(want).tolist())))
