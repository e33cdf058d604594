"""GPU twin of tests/test_oracle_reference_kats.py: the known answers of the reference's own unit tests
(tests/golden/reference_kats.json.gz) held against the PRODUCT -- the device functions of the HIP kernels through
dtof_eval_component, and the TLAS / BLAS traversal + surface interaction through dtof_ray_intersect / dtof_ray_test."""
import ctypes as C

import numpy as np
import pytest

import refkat

pytestmark = pytest.mark.gpu


class ProductBackend:
    """the facade's backend over libdtof.so (GPU); what has no C-ABI entry point raises Skip"""

    def __init__(self, mi):
        self.mi = mi

    def load_scene(self, xml):
        try:
            return self.mi.load_string(xml)
        except self.mi.DtofError as e:
            raise refkat.Skip("loader: %s" % str(e)[:60])

    def ray_intersect(self, sc, o, d, t):
        r = sc.ray_intersect(o, d, t)
        hit = r["ids"][0, 0] >= 0
        vals = np.zeros(25, np.float32)
        vals[0] = r["t"][0]
        # facade layout: p, n, sh_n, sh_s, sh_t, dp_du, dp_dv, wi  (dp_du / dp_dv are internal to compute_surface on the GPU)
        vals[1:4], vals[4:7], vals[7:10], vals[10:13], vals[13:16], vals[22:25] = r["p"][0], r["n"][0], r["sh_n"][0], r["sh_s"][0], r["sh_t"][0], r["wi"][0]
        vals[16:22] = np.nan
        return bool(hit), vals

    def ray_test(self, sc, o, d, t):
        return bool(sc.ray_test(o, d, t)[0])

    def microfacet(self, type_, au, av, visible, fn, inp):
        name = ("microfacet_eval", "microfacet_pdf", "microfacet_g1", "microfacet_sample")[fn]
        out = self.mi.eval_component(name, inp, [type_, au, av, int(visible)])
        res = np.zeros((len(inp), 4), np.float32)
        res[:, :out.shape[1]] = out
        return res

    def fresnel(self, c, eta):
        return self.mi.eval_component("fresnel", [[c]], [eta])[0]

    def filter_eval(self, kind, radius, stddev, B, C, x):
        return float(self.mi.eval_component("rfilter", [[x]], [kind, radius, stddev, B, C])[0, 0])

    def tea_float32(self, v0, v1, rounds):
        if rounds != 4:
            raise refkat.Skip("the sampler seeds with 4 rounds")
        bits = np.array([[v0, v1]], np.uint32).view(np.float32)
        return float(self.mi.eval_component("tea_float32", bits)[0, 0])

    def coordinate_system(self, n):
        out = self.mi.eval_component("coordinate_system", [n])[0]
        return out[:3].copy(), out[3:].copy()

    def warp(self, fn, sx, sy):
        name = {0: "warp_cosine_hemisphere", 1: "warp_disk_concentric", 3: "warp_uniform_triangle", 4: "warp_uniform_sphere"}[fn]
        out = self.mi.eval_component(name, [[sx, sy]])[0]
        return np.concatenate([out, np.zeros(3 - len(out), np.float32)])

    def sensor_info(self, sc):
        s = sc.export(2)
        return dict(shutter_open=float(s[19]), shutter_close=float(s[20]), focus_distance=float(s[23]), to_world=s[:16].astype(np.float64).reshape(4, 4))

    def film_info(self, sc):
        i = sc.info()
        return dict(size=(i["film_width"], i["film_height"]), crop_size=(i["crop_width"], i["crop_height"]), crop_offset=(i["crop_x"], i["crop_y"]))

    def camera_ray(self, sc, px, py, ax=.5, ay=.5):   # film position in pixels -> position sample of the crop window; the device function of the first-bounce kernel
        i = sc.info()
        o, d, _ = sc.camera_rays([[(np.float32(px) - i["crop_x"]) / np.float32(i["crop_width"]), (np.float32(py) - i["crop_y"]) / np.float32(i["crop_height"]), ax, ay]])
        return o[0].copy(), d[0].copy()

    def bsdf(self, sc, i, wi, wo, s3):   # the shade kernels' own BSDF function (dtof_bsdf_eval), flat local frame, uv = 0
        q = np.concatenate([np.asarray(wi, np.float32), np.asarray(wo, np.float32), np.asarray(s3, np.float32), np.zeros(2, np.float32)])
        return sc.bsdf_eval(i, [q])[0, :13].copy()

    def __getattr__(self, name):       # shape_area, sphere_sample_direction, splat, gauss_legendre, solve_quadratic
        def missing(*a, **k):
            raise refkat.Skip("no C-ABI entry point for '%s' (pinned through the oracle; the kernels are lane-for-lane bit-exact with it)" % name)
        return missing


@pytest.fixture(scope="module")
def results(mi):
    return refkat.run_all(ProductBackend(mi))


PINNED = {
    "src/render/tests/test_microfacet.py": 20, "src/render/tests/test_fresnel.py": 10, "src/rfilters/tests/test_rfilter.py": 8,
    "src/core/tests/test_warp.py": 10, "src/core/tests/test_random.py": 8, "src/core/tests/test_frame.py": 3,
    "src/shapes/tests/test_rectangle.py": 15, "src/shapes/tests/test_sphere.py": 500, "src/shapes/tests/test_disk.py": 500,
    "src/shapes/tests/test_cube.py": 100, "src/shapes/tests/test_instance.py": 400, "src/shapes/tests/test_cylinder.py": 60,
    "src/bsdfs/tests/test_diffuse.py": 30, "src/bsdfs/tests/test_dielectric.py": 15, "src/bsdfs/tests/test_twosided.py": 2,
    "src/sensors/tests/test_perspective.py": 90, "src/sensors/tests/test_orthographic.py": 60, "src/sensors/tests/test_thinlens.py": 120,
}


def test_no_reference_assertion_fails_on_the_gpu(results):
    bad = {f: st["fail"][:8] for f, st in results.items() if st["fail"]}
    assert not bad, bad


@pytest.mark.parametrize("ref_file", sorted(PINNED))
def test_component_is_pinned_on_the_gpu(results, ref_file):
    st = results.get(ref_file)
    assert st is not None and st["pass"] >= PINNED[ref_file], (ref_file, st and st["pass"], st and st["skip"].most_common(5))


def test_instance_relations_on_the_gpu(results):
    st = results["src/shapes/tests/test_instance.py"]
    assert len(st.get("edge", [])) <= 0.01 * st["pass"], st.get("edge")


def test_report(results, capsys):
    total = sum(st["pass"] for st in results.values())
    with capsys.disabled():
        print("\nreference known answers reproduced by the GPU product: %d" % total)
        for f in sorted(results):
            st = results[f]
            print("  %-46s pass %5d  fail %3d  skip %5d" % (f, st["pass"], len(st["fail"]), sum(st["skip"].values())))
    assert total >= 2500


def test_restated_math_matches_the_oracle_bit_for_bit(mi, orc):
    """exp / log / tan / erf / erfinv / sin / cos / acos: device == oracle on a dense sweep (the Beckmann lanes depend on it), and on the special values: +-0,
    denormals, the ends of each function's range, arguments next to the octant boundaries of the range reduction, huge arguments, +-inf and NaN where the
    function is defined there (dtof_math.h: sincos_ / tan_ for |x| 4 / pi < 2^31, exp_ / erf_ for everything but NaN).  Two NaNs are equal.
    tests/test_math_sweep_gpu.py holds the device against the host compilation on all 2^32 inputs; this is the device <-> oracle leg through the C ABI."""
    L = orc.lib()
    s_, c_ = C.c_float(), C.c_float()

    def orc_sin(x):
        L.orc_sincos(x, C.byref(s_), C.byref(c_))
        return s_.value

    def orc_cos(x):
        L.orc_sincos(x, C.byref(s_), C.byref(c_))
        return c_.value

    sweeps = {0: ("orc_expf", np.linspace(-104, 89, 20001)), 1: ("orc_logf", np.exp(np.linspace(-100, 88, 20001))), 2: ("orc_tanf", np.linspace(-20, 20, 20001)),
              3: ("orc_erff", np.linspace(-6, 6, 20001)), 4: ("orc_erfinvf", np.linspace(-0.999999, 0.999999, 20001)), 7: ("orc_acos", np.linspace(-1, 1, 20001)),
              5: (orc_sin, np.linspace(-20, 20, 20001)), 6: (orc_cos, np.linspace(-20, 20, 20001))}
    f32 = lambda bits: np.array(bits, np.uint32).view(np.float32)
    octants = (np.arange(1, 65, dtype=np.float64) * (np.pi / 4)).astype(np.float32).view(np.uint32)
    near_octants = f32(np.concatenate([octants + np.uint32(k) for k in (-2 & 0xffffffff, -1 & 0xffffffff, 0, 1, 2)]))
    finite = np.concatenate([f32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000, 0x3f7fffff,
                                  0xbf7fffff, 0x3f800001, 0xbf800001, 0x3f000000, 0xbf000000, 0x3effffff, 0x3f000001]), near_octants, -near_octants])
    huge = f32([0x4b800000, 0xcb800000, 0x4e000000, 0x4ec90fda, 0xcec90fda])          # 2^24, 2^29, the last float of sincos_'s range
    out_of_trig_range = f32([0x4ec90fdb, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000])
    nan = f32([0x7fc00000, 0xffc00000, 0x7f800001])
    special = {0: np.concatenate([finite, huge, out_of_trig_range, f32([0x42b17217, 0x42b17218, 0x42b17219, 0xc2ce8ed0, 0xc2ce8ed1, 0xc2cff1b4, 0xc2cff1b5])]),   # around 88.72 / -103.28
               1: np.concatenate([finite, huge, out_of_trig_range, nan]), 2: np.concatenate([finite, huge]),
               3: np.concatenate([finite, huge, out_of_trig_range, f32([0x40400000, 0x40c00000, 0x41200000, 0xc1200000])]),
               4: np.concatenate([finite, huge, out_of_trig_range, nan]), 7: np.concatenate([finite, huge, out_of_trig_range, nan]),
               5: np.concatenate([finite, huge]), 6: np.concatenate([finite, huge])}
    for fn, (name, xs) in sweeps.items():
        xs = np.concatenate([xs.astype(np.float32), special[fn]])
        gpu = mi.eval_component("math", xs.reshape(-1, 1), [fn])[:, 0]
        f = getattr(L, name) if isinstance(name, str) else name
        cpu = np.array([f(float(x)) for x in xs], np.float32)
        same = (gpu.view(np.uint32) == cpu.view(np.uint32)) | (np.isnan(gpu) & np.isnan(cpu))
        assert same.all(), (name if isinstance(name, str) else name.__name__, [(hex(a), hex(b), hex(c)) for a, b, c in
                                                                                zip(xs.view(np.uint32)[~same][:5], gpu.view(np.uint32)[~same][:5], cpu.view(np.uint32)[~same][:5])])
    assert len(sweeps) == 8 and all(len(v) >= 60 for v in special.values())
