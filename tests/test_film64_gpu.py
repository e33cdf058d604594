"""The opt-in float64 film (k_splat_f64 and the double instantiations k_develop<double, ADD>, k_develop_rgba<double> of dtof_develop.hip; Scene.render(film="float64"), render_film64, render_rows_f64,
develop_f64_async, render_velocity_map(film="float64")) against the oracle's order-independent film: orc_render_exact sums the same float32 splat terms in float64
and develops in float64, orc_render_alpha does the same for the alpha channel.

Criteria (derived, not measured):
  developed images   rel_linf_px(img, exact) <= 2^-23 -- one float32 ulp of a pixel above the floor.  Both sides add the SAME float32 terms in double; the order noise of a
                     double sum of at most ~2^12 terms (relative 2^-53 * 2^12 of the sum of magnitudes) is far below half a float32 ulp of the quotient unless a pixel
                     cancels by more than 2^17, so the rounded quotient moves by at most one ulp
  weight channel     of the raw film, all terms positive: relative difference from the oracle's at most 2^-40 (2^12 additions of relative error 2^-53 each)
  signed weights     (12_wall_lanczos, the wide per-lane path) all four raw channels against the sums of the oracle's lanes (moments_ref.expected_rgbw, which
                     test_film64_cpu.py holds to orc_render_exact): |device - expected| <= 2^-40 * sum |term| per pixel, the moment film's criterion
Every case also prints how many floats differ from the oracle at all (a CPU simulation of 20 random orders found none on the tent scenes); 0 is not asserted."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import SCENES
import moments_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_pattern.so")
IMG_BOUND, W_BOUND = 2.0 ** -23, 2.0 ** -40
NCPU = os.cpu_count() or 1
SEED = 3
K4 = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]


def rel_linf_px(a, ref, eps=1e-3):
    """test_gpu_parity.rel_linf_px: max over pixels and channels of |a - ref| / max(|ref_px|, eps * max|ref|)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    floor = eps * max(np.abs(ref).max(), 1e-30)
    return float((np.abs(a - ref) / np.maximum(np.abs(ref), floor)).max())


def differing(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def develop(film):
    """orc_render_exact's last loop in numpy: (float) (RGB / (W == 0 ? 1 : W)) in float64"""
    w = np.where(film[..., 3] == 0.0, 1.0, film[..., 3])[..., None]
    return (film[..., :3] / w).astype(np.float32)


def integrator_of(osc, **override):
    """the scene file's integrator as the dictionary Scene.params(integrator=...) takes, with properties replaced (test_variants.integrator_of)"""
    ip = osc.flat.integrator
    conv = {"float": float, "int": int, "bool": bool}
    d = {"type": ip.plugin}
    d.update({k: conv.get(t, str)(v) for k, (t, v) in ip.items()})
    d.update(override)
    return d


def oracle_exact(orc, osc, pd, seed, spp):
    """orc_render_exact with a film array of our own -> (developed image (H, W, 3) float32, raw film (H, W, 4) float64)"""
    w, h = osc.size
    film, img = np.zeros((h, w, 4), np.float64), np.zeros((h, w, 3), np.float32)
    L = orc.lib()
    L.orc_render_exact.restype = C.c_uint64
    L.orc_render_exact.argtypes = [C.POINTER(orc.OrcScene), C.POINTER(orc.OrcParams), C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int]
    p = orc.make_params(pd)
    n = L.orc_render_exact(C.byref(osc.c), C.byref(p), seed, spp or pd["sample_count"], 0, h, film.ctypes.data, img.ctypes.data, NCPU)
    assert n == w * h * (spp or pd["sample_count"])
    return img, film


def hold(what, img, film, ref_img, ref_film):
    """one colour plane against the oracle: prints every figure, then asserts the two criteria"""
    err = rel_linf_px(img, ref_img)
    w, wr = film[..., 3], ref_film[..., 3]
    w_err = float((np.abs(w - wr) / np.where(wr == 0.0, 1.0, wr)).max())
    print("%s: rel_linf_px %.3g (bound %.3g), %d of %d floats differ, weight channel rel %.3g (bound %.3g), raw film %d of %d doubles differ"
          % (what, err, IMG_BOUND, differing(img, ref_img), img.size, w_err, W_BOUND, int((film != ref_film).sum()), film.size))
    assert np.abs(ref_img).max() > 0 and (wr > 0).any(), what
    assert err <= IMG_BOUND, (what, err)
    assert ((w == 0.0) == (wr == 0.0)).all() and w_err <= W_BOUND, (what, w_err)
    assert differing(develop(film), img) == 0, (what, "the returned image is not its film developed in float64")


def hold_signed(what, img, film, osc, orc, pd, spp):
    """a film whose weights are signed (the Lanczos filter): hold()'s weight criterion assumes positive terms, so all four raw channels are held to the sums of the
    oracle's lanes by the moment film's derived criterion, |device - expected| <= 2^-40 * sum |term| per pixel (moments_ref.errors_over_bound)"""
    want, mags = ref.expected_rgbw(orc, osc, pd, SEED, spp)
    ratios = ref.errors_over_bound(np.moveaxis(film, -1, 0), want, mags)
    print("%s: largest error / bound: r %.3g g %.3g b %.3g w %.3g" % ((what,) + tuple(ratios)))
    assert np.abs(want[:3]).max() > 0 and (want[3] > 0).any(), what
    assert (ratios <= 1.0).all(), (what, ratios)
    assert (want[3] < 0).any() or (mags[3] > np.abs(want[3])).any(), "the Lanczos filter has negative weights"
    assert differing(develop(film), img) == 0, (what, "the returned image is not its film developed in float64")


def _edit(xml, case):
    if case == "gauss":      # tests/test_device_film.py::_gauss: stddev 0.5, radius 2, a 5 x 5 footprint and a halo of 2
        old, new = '<rfilter type="tent" />', '<rfilter type="gaussian" />'
    elif case in ("box", "lanczos"):      # lanczos: 3 lobes, a 7 x 7 footprint, negative weights
        old, new = '<rfilter type="tent" />', '<rfilter type="%s" />' % case
    elif case == "crop":
        old, new = '<string name="file_format"', ('<integer name="crop_offset_x" value="5" /><integer name="crop_offset_y" value="3" />'
                                                   '<integer name="crop_width" value="16" /><integer name="crop_height" value="12" /><string name="file_format"')
    elif case == "rgba":
        old, new = '<string name="pixel_format" value="rgb" />', '<string name="pixel_format" value="rgba" />'
    assert old in xml, case
    return xml.replace(old, new)


# id -> (scene, -D parameters, spp, edit of the XML, integrator override, environment)
CASES = {
    "1_wall_64spp_default": ("cornell_wall.xml", dict(resx=16, resy=16), 64, None, None, {}),                 # the float32 route of this frame splats inside k_shade
    "2_wall_64spp_split": ("cornell_wall.xml", dict(resx=16, resy=16), 64, None, None, {"DTOF_PIPELINE": "split"}),
    "3_sphere_light_64spp": ("cornell_sphere_light.xml", dict(resx=16, resy=16), 64, None, None, {}),         # the float32 film is 8.8e-3 off here
    "4_area_24spp": ("cornell_area.xml", dict(resx=16, resy=16), 24, None, None, {}),                         # runs that straddle waves
    "5_wall_15x13_3spp": ("cornell_wall.xml", dict(resx=15, resy=13), 3, None, None, {}),                     # short runs, a lane count that is no multiple of 64
    "6_wall_100spp": ("cornell_wall.xml", dict(resx=16, resy=16), 100, None, None, {}),                       # a run longer than a wave
    "7_rough_gaussian": ("cornell_rough.xml", dict(resx=24, resy=24, max_depth=5), 8, "gauss", None, {}),     # 5 x 5 footprint
    "8_wall_box": ("cornell_wall.xml", dict(resx=16, resy=16), 16, "box", None, {}),
    "9_domino_small": ("domino_small.xml", dict(resx=32, resy=32), 4, None, None, {}),                        # mesh kernels
    "10_wall_crop": ("cornell_wall.xml", dict(resx=32, resy=24), 8, "crop", None, {}),                        # a crop window at (5, 3)
    "11_wall_multi_pass": ("cornell_wall.xml", dict(resx=16, resy=16), 16, None, dict(samples_per_pass=4), {}),
    "12_wall_lanczos": ("cornell_wall.xml", dict(resx=16, resy=16), 4, "lanczos", None, {}),                  # the wide per-lane path, negative weights: hold_signed
}


def load(mi, orc, scene, params, edit=None, override=None):
    """(product scene, oracle scene, the oracle's parameter dictionary)"""
    path = os.path.join(SCENES, scene)
    if edit:
        xml = open(path).read()
        for e in edit.split("+"):
            xml = _edit(xml, e)
        sc, osc = mi.load_string(xml, **params), orc.Scene(xml, params, is_string=True)
    else:
        sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    if override:
        integ = integrator_of(osc, **override)
        sc.set_integrator(integ)
        return sc, osc, osc.params(integrator=integ)
    return sc, osc, osc.params()


@pytest.mark.parametrize("case", list(CASES))
def test_float64_film_against_the_exact_oracle(mi, orc, case, monkeypatch):
    scene, params, spp, edit, override, env = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, osc, pd = load(mi, orc, scene, params, edit, override)
    ref_img, ref_film = oracle_exact(orc, osc, pd, SEED, spp)
    images, films = sc.render_film64(SEED, spp)
    st = sc.last_stats
    w, h = sc.size
    assert images.shape == (1, h, w, 3) and films.shape == (1, h, w, 4) and st["n_paths"] == w * h * spp
    assert st["n_fused_splat_launches"] == 0 and st["ms_splat"] > 0, st      # the separate splat stage ran, whatever the float32 route of this frame does
    if env.get("DTOF_PIPELINE") == "split":
        assert st["ms_trace"] > 0, st
    if case == "12_wall_lanczos":
        hold_signed(case, images[0], films[0], osc, orc, pd, spp)
    else:
        hold(case, images[0], films[0], ref_img, ref_film)
    again = sc.render(seed=SEED, spp=spp, film="float64")      # the plain form: the same image, from a second traversal
    print("%s: a second call differs in %d floats" % (case, differing(again, images[0])))
    assert again.shape == (h, w, 3) and rel_linf_px(again, images[0]) <= IMG_BOUND
    if case.startswith("1_"):
        f32 = sc.render(seed=SEED, spp=spp)
        print("%s: float32 route: %d fused splat launches, rel_linf_px against the exact film %.3g" % (case, sc.last_stats["n_fused_splat_launches"], rel_linf_px(f32, ref_img)))


@pytest.fixture(scope="module")
def wall_variants(mi, orc):
    """cornell_wall 16 x 16 x 16 spp: the oracle's exact image and film of every pair of K4, each rendered once"""
    params = dict(resx=16, resy=16)
    path = os.path.join(SCENES, "cornell_wall.xml")
    osc = orc.Scene(path, params)
    refs = {}
    for f, o in K4 + [(1.0, 0.5)]:
        pd = osc.params(integrator=integrator_of(osc, hetero_frequency=float(np.float32(f)), hetero_offset=float(np.float32(o))))
        refs[f, o] = oracle_exact(orc, osc, pd, SEED, 16)
    return path, params, refs


@pytest.mark.parametrize("K", [4, 2, 3])
def test_variant_planes_against_the_exact_oracle(mi, wall_variants, K):
    path, params, refs = wall_variants
    sc = mi.load_file(path, **params)
    images, films = sc.render_film64(SEED, 16, variants=K4[:K])
    assert images.shape == (K, 16, 16, 3) and films.shape == (K, 16, 16, 4) and sc.last_stats["n_fused_splat_launches"] == 0
    for k, pair in enumerate(K4[:K]):
        hold("K=%d plane %d %s" % (K, k, pair), images[k], films[k], *refs[pair])
    assert differing(images[0], images[K - 1]) > 0
    if K == 4:      # the other forms of Scene.render: five variants are two traversals, offsets are variants at the integrator's own frequency (1 in this scene)
        five = sc.render(seed=SEED, spp=16, variants=K4 + [(1.0, 0.5)], film="float64")
        assert five.shape == (5, 16, 16, 3)
        for k, pair in enumerate(K4 + [(1.0, 0.5)]):
            assert rel_linf_px(five[k], refs[pair][0]) <= IMG_BOUND, pair
        assert sc.info()["hetero_frequency"] == 1.0
        offs = sc.render(seed=SEED, spp=16, offsets=[0.0, 0.25, 0.5], film="float64")
        for k, o in enumerate((0.0, 0.25, 0.5)):
            assert rel_linf_px(offs[k], refs[1.0, o][0]) <= IMG_BOUND, o


@pytest.mark.parametrize("scene,params,spp,edit", [("cornell_wall.xml", dict(resx=16, resy=16), 16, "rgba"),
                                                   ("open_veils.xml", dict(resx=32, resy=32, max_depth=5, pixel_format="rgba"), 8, None)], ids=["wall", "open_veils"])
def test_rgba_film_against_the_exact_oracle(mi, orc, scene, params, spp, edit):
    """the colour planes as above; the alpha plane lies behind them and is held against orc_render_alpha"""
    sc, osc, _ = load(mi, orc, scene, params, edit)
    assert sc.info()["has_alpha"]
    variants = K4[:2] if scene == "cornell_wall.xml" else None
    pairs = variants or [None]
    images, films = sc.render_film64(SEED, spp, variants=variants)
    K = len(pairs)
    w, h = sc.size
    assert images.shape == (K, h, w, 4) and films.shape == (K + 1, h, w, 4)
    alpha_ref = osc.render_alpha(osc.params(), seed=SEED, spp=spp, threads=NCPU)
    for k, pair in enumerate(pairs):
        pd = osc.params() if pair is None else osc.params(integrator=integrator_of(osc, hetero_frequency=pair[0], hetero_offset=pair[1]))
        hold("%s rgba plane %d" % (scene, k), images[k][..., :3], films[k], *oracle_exact(orc, osc, pd, SEED, spp))
        a_err = rel_linf_px(images[k][..., 3], alpha_ref)
        print("%s alpha of image %d: rel_linf_px %.3g, %d floats differ" % (scene, k, a_err, differing(images[k][..., 3], alpha_ref)))
        assert a_err <= IMG_BOUND, (scene, k, a_err)
    a = films[K]      # (A, 0, 0, W): the weights of the colour planes, the alpha developed like them
    assert not a[..., 1:3].any() and (np.abs(a[..., 3] - films[0][..., 3]) <= W_BOUND * films[0][..., 3]).all()
    wa = np.where(a[..., 3] == 0.0, 1.0, a[..., 3])
    assert differing((a[..., 0] / wa).astype(np.float32), images[0][..., 3]) == 0
    if scene == "open_veils.xml":
        assert 0 < alpha_ref.min() < 1 or (alpha_ref == 0).any(), "the open scene has pixels that are not fully covered"


def test_two_identical_calls_agree(mi):
    sc = mi.load_file(os.path.join(SCENES, "cornell_sphere_light.xml"), resx=16, resy=16)
    a, fa = sc.render_film64(SEED, 64)
    b, fb = sc.render_film64(SEED, 64)
    print("two identical calls: %d of %d floats differ, rel_linf_px %.3g; %d of %d film doubles differ" % (differing(a, b), a.size, rel_linf_px(a, b), int((fa != fb).sum()), fa.size))
    assert rel_linf_px(a, b) <= IMG_BOUND and rel_linf_px(b, a) <= IMG_BOUND


def test_device_film_bands_into_padded_float64_slabs(mi, wall_variants):
    """render_rows_f64, K = 4, the three bands of distributed.row_band(H, 3, r), each into a padded float64 slab with margins; develop_f64_async on the device"""
    import torch
    from mitsuba3dopplertof_amd import distributed as D
    path, params, refs = wall_variants
    sc = mi.load_file(path, **params)
    W, H = sc.size
    halo, WORLD, K, spp = sc.info()["filter_halo"], 3, 4, 16
    assert halo == 1
    prow = D.padded_rows(H, WORLD, halo)
    stride = prow * W * 4
    margin = stride + 24      # more than a plane: a fifth plane written behind the four declared ones would land here
    total = np.zeros((K, H, W, 4), np.float64)
    n_paths = 0
    for r in range(WORLD):
        r0, r1 = D.row_band(H, WORLD, r)
        buf = torch.zeros(2 * margin + K * stride, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ptr = buf.data_ptr() + 8 * (margin + halo * W * 4)      # film row 0 of plane 0: the slab has `halo` rows above it
        st = sc.render_rows_f64(ptr, SEED, spp, r0, r1, variants=K4, planes=K, plane_stride_doubles=stride)
        n_paths += st["n_paths"]
        assert st["n_paths"] == (r1 - r0) * W * spp and st["n_fused_splat_launches"] == 0
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert not host[:margin].any() and not host[margin + K * stride:].any(), ("margins", r)
        slab = host[margin:margin + K * stride].reshape(K, prow, W, 4)
        lo, hi = max(r0 - halo, 0), min(r1 + halo, H)
        assert not slab[:, :halo + lo].any() and not slab[:, halo + hi:].any(), ("rows outside the band and its halo", r)      # item (e) of test_device_film.py
        assert all(slab[k, halo + lo:halo + hi, :, 3].any() for k in range(K)), r
        total += slab[:, halo:halo + H]
        if r == 1:      # a stride that would make the planes overlap is refused, and nothing is written
            again = torch.zeros_like(buf)
            torch.cuda.synchronize()
            with pytest.raises(mi.DtofError, match="the planes would overlap"):
                sc.render_rows_f64(again.data_ptr() + 8 * margin, SEED, spp, r0, r1, variants=K4, planes=K, plane_stride_doubles=(hi - lo) * W * 4 - 4)
            with pytest.raises(mi.DtofError, match="this call writes 4"):
                sc.render_rows_f64(again.data_ptr() + 8 * margin, SEED, spp, r0, r1, variants=K4, planes=3, plane_stride_doubles=stride)
            torch.cuda.synchronize()
            assert not again.cpu().numpy().any()
    assert n_paths == W * H * spp
    for k, pair in enumerate(K4):      # the overlap-add of the slabs
        hold("bands, plane %d %s" % (k, pair), develop(total[k]), total[k], *refs[pair])
    # the whole frame into a dense film, developed on the device plane by plane: the numpy develop, bit for bit
    dense = torch.zeros((K, H, W, 4), dtype=torch.float64, device="cuda")
    rgb = torch.zeros((K, H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sc.render_rows_f64(dense.data_ptr(), SEED, spp, 0, H, variants=K4)
    for k in range(K):
        sc.develop_f64_async(dense.data_ptr() + 8 * k * H * W * 4, rgb.data_ptr() + 4 * k * H * W * 3, H * W)
    sc.collect()
    torch.cuda.synchronize()
    films, developed = dense.cpu().numpy(), rgb.cpu().numpy()
    for k, pair in enumerate(K4):
        assert differing(developed[k], develop(films[k])) == 0, k
        hold("dense device film, plane %d" % k, developed[k], films[k], *refs[pair])


SYNTHETIC_SIZES = (1, 255, 257)      # one lane, a block less one lane, a block and one lane
MARGIN, SENT32 = 64, np.float32(-7.5e11)      # sentinel floats on both sides of every output (64 floats keep the rgba image 16-byte aligned)


def synthetic_film64(rng, n):
    """(colour film, alpha film) [n][4] float64, as a splat leaves them: doubles with all 53 bits in use, so that rounding the operands to float32 before the division
    moves the quotient; W in [0.25, 64).  With room for them: a pixel with W = 0, one with a colour of -0.0, one whose alpha film has a weight of 0"""
    film = rng.standard_normal((n, 4)) * 10.0 ** rng.uniform(-3, 3, (n, 4))
    film[:, 3] = rng.uniform(0.25, 64.0, n)
    alpha = np.zeros((n, 4))
    alpha[:, 3] = film[:, 3]
    alpha[:, 0] = alpha[:, 3] * rng.uniform(0.0, 1.0, n)
    if n >= 3:
        film[0, 3] = 0.0
        film[1, :3] = -0.0
        alpha[2, 3] = 0.0
    return film, alpha


def develop_in_float32(film):
    """what a kernel that rounded the film to float32 before dividing would return"""
    f = film.astype(np.float32)
    return f[..., :3] / np.where(f[..., 3] == 0, np.float32(1), f[..., 3])[..., None]


def test_synthetic_float64_films_are_developed_in_double(mi):
    """dtof_develop_f64_async and dtof_develop_rgba_f64_async on constructed films: numpy's float64 quotient rounded to float32 once, bit for bit, -0.0 and the
    W = 0 pixels included, nothing written outside the image; at least a quarter of the expected floats are not what a division in float32 gives"""
    import torch
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=8, resy=8)
    rng = np.random.default_rng(64)
    moved = total = 0
    for n in SYNTHETIC_SIZES:
        film, alpha = synthetic_film64(rng, n)
        want_rgb = develop(film)
        want_rgba = np.concatenate([want_rgb, develop(alpha)[:, :1]], axis=1)
        in_f32 = np.concatenate([develop_in_float32(film), develop_in_float32(alpha)[:, :1]], axis=1)
        moved += differing(want_rgba, in_f32); total += want_rgba.size
        d_film, d_alpha = torch.from_numpy(film).cuda(), torch.from_numpy(alpha).cuda()
        d_rgb = torch.full((3 * n + 2 * MARGIN,), float(SENT32), dtype=torch.float32, device="cuda")
        d_rgba = torch.full((4 * n + 2 * MARGIN,), float(SENT32), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        sc.develop_f64_async(d_film.data_ptr(), d_rgb.data_ptr() + 4 * MARGIN, n)
        sc.develop_f64_async(d_film.data_ptr(), d_rgba.data_ptr() + 4 * MARGIN, n, d_alpha_film_ptr=d_alpha.data_ptr())
        sc.collect()
        torch.cuda.synchronize()
        for name, got, want in (("rgb", d_rgb.cpu().numpy(), want_rgb), ("rgba", d_rgba.cpu().numpy(), want_rgba)):
            bad = differing(got[MARGIN:MARGIN + want.size].reshape(want.shape), want)
            print("n %d %s: %d of %d floats differ from numpy's" % (n, name, bad, want.size))
            assert bad == 0, (n, name, bad)
            assert (got[:MARGIN] == SENT32).all() and (got[MARGIN + want.size:] == SENT32).all(), ("margins", n, name)
        if n >= 3:      # the constructed pixels are what they were meant to be: divided by 1, -0.0, divided by 1
            assert differing(want_rgb[0], film[0, :3].astype(np.float32)) == 0 and want_rgb[0].all()
            assert np.signbit(want_rgb[1]).all() and not want_rgb[1].any()
            assert want_rgba[2, 3] == np.float32(alpha[2, 0]) != 0
    print("%d of %d expected floats differ from a division in float32" % (moved, total))
    assert 4 * moved >= total, (moved, total)


def same(got, expected):
    """test_velocity_map_device.same: bit patterns equal where `expected` is not a NaN, NaN where it is; the number of elements that differ"""
    got, expected = np.ascontiguousarray(got), np.ascontiguousarray(expected)
    assert got.dtype == expected.dtype and got.shape == expected.shape, (got.dtype, expected.dtype, got.shape, expected.shape)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    nan = np.isnan(expected)
    return int(np.where(nan, ~np.isnan(got), got.view(u) != expected.view(u)).sum())


@pytest.mark.parametrize("offsets", [(0.0, 0.25), (0.0, 0.25, 0.5)], ids=["two_offsets", "three_offsets"])
def test_velocity_map_of_the_float64_film(mi, offsets):
    """map, pair maps and ToF images are, bit for bit, what numpy makes of render(seed=i, spp=16, variants=..., film="float64"), i = 0, 1"""
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=16, resy=16)
    v, films, pairs = sc.render_velocity_map(2, 16, offsets, pairs=True, film="float64")
    st = sc.last_stats
    assert st["n_paths"] == 16 * 16 * 16 * 2 * ((len(offsets) + 1) // 2) and st["n_fused_splat_launches"] == 0
    homo, hetero = [], []
    for g in range(0, len(offsets), 2):      # the odd last offset is a group of two films
        group = list(offsets[g:g + 2])
        variants = [(0.0, o) for o in group] + [(1.0, o) for o in group]
        acc = None
        for i in range(2):
            img = sc.render(seed=i, spp=16, variants=variants, film="float64")
            acc = img if acc is None else acc + img
        images = acc / np.float32(2)
        homo += [mi.to_tof_image(im, 0.0015) for im in images[:len(group)]]
        hetero += [mi.to_tof_image(im, 0.0015) for im in images[len(group):]]
    with np.errstate(all="ignore"):
        expected = harness.calc_velocity_from_homo_heteros(homo, hetero, 0.0015, 30)
        for j in range(len(offsets)):
            assert same(films["homodyne"][j], homo[j]) == 0 and same(films["heterodyne"][j], hetero[j]) == 0, j
            assert same(pairs[j], harness.calc_velocity_from_homo_hetero(homo[j], hetero[j], 0.0015, 30)) == 0, j
        assert same(v, expected) == 0, same(v, expected)
    assert np.isfinite(expected).mean() > 0.9
    v2, _ = harness.run_scene_velocity_map_device(sc, total_spp=16, offsets=offsets, film="float64")
    assert v2.shape == v.shape and np.isfinite(v2).mean() > 0.9


def test_cases_on_the_pattern_initialised_build():
    """cases 1 and 4 and the K = 4 planes against libdtof_pattern.so (every uninitialised automatic variable a NaN pattern), the way test_pattern_build.py runs it"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    env = dict(os.environ, DTOF_LIB=PATTERN_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "1_wall_64spp_default or 4_area_24spp or (variant_planes and [4])"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "\n3 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
