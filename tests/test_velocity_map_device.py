"""The radial-velocity map reconstructed on the device (k_develop<float, ADD> of dtof_develop.hip, k_velocity_map; dtof_develop_accumulate_async, dtof_velocity_map_async,
dtof_render_velocity_map) against the numpy route of harness.py (to_tof_image, calc_velocity_from_homo_hetero(s), which mirror the reference's image_utils.py).

Every comparison of reconstructed values is EXACT: equal bit patterns wherever the expected value is not a NaN (+-0 and +-inf included), a NaN wherever it is one
(payload and sign of a NaN are not compared: x86 and the GPU produce different default NaNs), no pixel left out.

  synthetic  RGBW planes uploaded with torch: sizes around the block and wave boundaries, 1 - 3 passes, 1 - 3 pairs with permuted plane indices, dense and padded
             strides, two (T, w_g); values of every magnitude, special values, W of 0, ratios on and beyond the clip bounds, a vanishing homodyne; sentinel margins
  rendered   dtof_render_velocity_map on the wall (an even and an odd number of offsets, both pipelines) and an rgba scene: the map is numpy's of the call's own ToF
             images, the ToF images are the host route's within IMG_TOL, the statistics, the caller's film layout
  physics    harness.run_scene_velocity_map_device: the wall's -10 m/s
  refusals   every refused call returns DTOF_ERR_INVALID and leaves sentinel-filled device buffers alone
  stream     the async pair on the caller's stream, ordered behind a render without a host wait"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SCENES

pytestmark = pytest.mark.gpu

IMG_TOL = 5e-5     # test_gpu_parity.IMG_TOL: relative to max|ref|; two atomic orders of the same lanes
INVALID = 1
MARGIN = 64        # sentinel elements on both sides of every output buffer
SENT32, SENT64 = np.float32(-7.5e11), np.float64(-7.5e111)
SIZES = (1, 63, 64, 65, 255, 257, 1000)
SETTINGS = ((0.0015, 30), (0.002, 150))
# (homodyne planes, heterodyne planes) of 1, 2, 3 pairs: permutations of the 2 * n_pairs planes of the sum
PAIRS = {1: ((1,), (0,)), 2: ((2, 0), (3, 1)), 3: ((4, 0, 3), (1, 5, 2))}
SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-38, 3e38, 1.0, -1.0], np.float32)
# heterodyne = factor * homodyne at the constructed pixels: the ratio on -1 and beyond it, around 0.999, on 1 (where only the clip keeps ratio - 1 from 0) and beyond
FACTORS = np.array([-1.0, -1.0 - 2.0 ** -10, -1.25, -1.0 + 2.0 ** -10, 0.999, 0.9995, 0.9985, 1.0, 1.5], np.float32)
N_CONSTRUCTED = len(FACTORS) + 4


def same(got, expected):
    """bit patterns equal where `expected` is not a NaN, NaN where it is; returns the number of elements that differ"""
    got, expected = np.ascontiguousarray(got), np.ascontiguousarray(expected)
    assert got.dtype == expected.dtype and got.shape == expected.shape, (got.dtype, expected.dtype, got.shape, expected.shape)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    nan = np.isnan(expected)
    return int(np.where(nan, ~np.isnan(got), got.view(u) != expected.view(u)).sum())


def make_films(rng, n, passes, n_pairs):
    """[passes][planes][n][4] float32 RGBW films: normal deviates scaled by 10^U(-6, 2); about a tenth of the pixels carry a special value in one channel of one
    plane per pass; W is 0 or positive; with room for them, the first pixels are constructed (FACTORS, a homodyne of +-0 under a heterodyne that is not 0)"""
    hom, het = PAIRS[n_pairs]
    planes = 2 * n_pairs
    film = (rng.standard_normal((passes, planes, n, 4)) * 10.0 ** rng.uniform(-6, 2, (passes, planes, n, 4))).astype(np.float32)
    film[..., 3] = np.where(rng.random((passes, planes, n)) < 0.15, 0.0, rng.uniform(0.25, 64.0, (passes, planes, n))).astype(np.float32)
    for i in np.nonzero(rng.random(n) < 0.1)[0]:
        for p in range(passes):
            film[p, rng.integers(planes), i, rng.integers(3)] = SPECIALS[rng.integers(len(SPECIALS))]
    if n >= 4 * N_CONSTRUCTED:
        base = np.array([0.5, 0.25, 0.125], np.float32)
        for i, f in enumerate(FACTORS):   # the same in every pass and pair, W = 2: the float32 chain of the heterodyne is the homodyne's times f up to its rounding
            for k in range(n_pairs):
                film[:, hom[k], i, :3], film[:, het[k], i, :3] = base * np.float32(k + 1), base * np.float32(k + 1) * f
                film[:, hom[k], i, 3] = film[:, het[k], i, 3] = 2.0
        for j, (zero, w) in enumerate(((0.0, 1.0), (-0.0, 1.0), (0.0, 0.0), (-0.0, 0.0))):   # homodyne +-0 (with and without a weight), heterodyne not 0
            i = len(FACTORS) + j
            for k in range(n_pairs):
                film[:, hom[k], i, :3], film[:, hom[k], i, 3] = np.float32(zero), w
                film[:, het[k], i, :3], film[:, het[k], i, 3] = np.array([0.3, -0.2, 0.7], np.float32), 1.5
    return film


def numpy_route(mi, developed, n_pairs, exposure_time, w_g):
    """developed: [passes][planes][n][3] float32 -> (ToF images [planes][n] float32, per-pair maps [n_pairs][n], combined map [n]) as harness.py computes them"""
    from mitsuba3dopplertof_amd import harness
    hom, het = PAIRS[n_pairs]
    with np.errstate(all="ignore"):
        acc = None
        for img in developed:      # render_multi_pass
            acc = img if acc is None else acc + img
        mean = acc / np.float32(len(developed))
        tof = mi.to_tof_image(mean, exposure_time)
        assert tof.dtype == np.float32
        pair_maps = np.stack([harness.calc_velocity_from_homo_hetero(tof[h], tof[t], exposure_time, w_g) for h, t in zip(hom, het)])
        v = harness.calc_velocity_from_homo_heteros([tof[h] for h in hom], [tof[t] for t in het], exposure_time, w_g)
    return tof, pair_maps, v


@pytest.fixture(scope="module")
def torch_scene(mi):
    """a scene whose library calls are enqueued on torch's current stream: torch.cuda.synchronize() then waits for them"""
    import torch
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=8, resy=8)
    sc.set_stream(torch.cuda.current_stream().cuda_stream)
    yield sc
    torch.cuda.synchronize()
    sc.set_stream(None)


def guarded(torch, n, dtype, sentinel):
    """a device buffer of n elements between two margins, all sentinel -> (tensor, pointer to the payload)"""
    t = torch.full((n + 2 * MARGIN,), float(sentinel), dtype=dtype, device="cuda")
    return t, t.data_ptr() + MARGIN * t.element_size()


def split_margins(t, n):
    a = t.cpu().numpy()
    return a[MARGIN:MARGIN + n], np.concatenate([a[:MARGIN], a[MARGIN + n:]])


def run_synthetic(mi, sc, film, n_pairs, exposure_time, w_g, padded):
    """upload the films, accumulate and reconstruct on the device; numpy develops the same planes for its route (rgb / (W == 0 ? 1 : W) in float32), and dtof_develop
    on every padded plane is held to numpy's develop bit for bit as well -> (mismatch counts, expected map)"""
    import torch
    L = mi._lib()
    passes, planes, n = film.shape[:3]
    stride = 4 * n + (12 if padded else 0)
    hom, het = PAIRS[n_pairs]
    d_sum, p_sum = guarded(torch, planes * n * 3, torch.float32, SENT32)
    d_tof, p_tof = guarded(torch, planes * n, torch.float32, SENT32)
    d_pairs, p_pairs = guarded(torch, n_pairs * n, torch.float64, SENT64)
    d_v, p_v = guarded(torch, n, torch.float64, SENT64)
    with np.errstate(all="ignore"):      # HDRFilm::develop in numpy: float32 throughout
        developed = film[..., :3] / np.where(film[..., 3] == 0, np.float32(1), film[..., 3])[..., None]
    assert developed.dtype == np.float32 and developed.shape == (passes, planes, n, 3)
    d_rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    for p in range(passes):
        host = np.full((planes, stride), 9.0e9, np.float32)      # what lies in the padding must not matter
        host[:, :4 * n] = film[p].reshape(planes, 4 * n)
        d_film = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        sc.develop_accumulate_async(d_film.data_ptr(), planes, p_sum, n, first=(p == 0), plane_stride_floats=stride if padded else 0)
        for k in range(planes):      # the store form of the same kernel, on the very same plane
            assert L.dtof_develop(d_film.data_ptr() + 4 * stride * k, d_rgb.data_ptr(), n) == 0, L.dtof_last_error()
            assert same(d_rgb.cpu().numpy(), developed[p, k]) == 0, ("dtof_develop against numpy", n, padded, p, k)
        torch.cuda.synchronize()
    sc.velocity_map_async(p_sum, hom, het, passes, n, p_v, exposure_time=exposure_time, w_g=w_g, d_tof_ptr=p_tof, d_velocity_pairs_ptr=p_pairs)
    torch.cuda.synchronize()
    tof, pair_maps, v = numpy_route(mi, developed, n_pairs, exposure_time, w_g)
    got_tof, m_tof = split_margins(d_tof, planes * n)
    got_pairs, m_pairs = split_margins(d_pairs, n_pairs * n)
    got_v, m_v = split_margins(d_v, n)
    _, m_sum = split_margins(d_sum, planes * n * 3)
    for name, margin, sentinel in (("sum", m_sum, SENT32), ("tof", m_tof, SENT32), ("pairs", m_pairs, SENT64), ("velocity", m_v, SENT64)):
        assert (margin == sentinel).all(), ("margin of " + name, n, padded)
    bad = {"tof": same(got_tof.reshape(planes, n), tof), "pairs": same(got_pairs.reshape(n_pairs, n), pair_maps), "velocity": same(got_v, v)}
    # without the optional outputs the map is the same and nothing else is written
    d_v2, p_v2 = guarded(torch, n, torch.float64, SENT64)
    sc.velocity_map_async(p_sum, hom, het, passes, n, p_v2, exposure_time=exposure_time, w_g=w_g)
    torch.cuda.synchronize()
    got_v2, m_v2 = split_margins(d_v2, n)
    assert (m_v2 == SENT64).all()
    bad["velocity alone"] = same(got_v2, v)
    return bad, v, pair_maps


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=["T1.5ms_30MHz", "T2ms_150MHz"])
@pytest.mark.parametrize("n_pairs", [1, 2, 3])
@pytest.mark.parametrize("passes", [1, 2, 3])
def test_synthetic_films_are_reconstructed_bit_for_bit(mi, torch_scene, passes, n_pairs, setting):
    exposure_time, w_g = SETTINGS[setting]
    rng = np.random.default_rng(1000 + 100 * passes + 10 * n_pairs + setting)
    finite = total = clipped_lo = clipped_hi = 0
    for n in SIZES:
        film = make_films(rng, n, passes, n_pairs)
        for padded in (False, True):
            bad, v, pair_maps = run_synthetic(mi, torch_scene, film, n_pairs, exposure_time, w_g, padded)
            print("n", n, "padded", padded, "mismatches", bad, "finite", int(np.isfinite(v).sum()))
            assert not any(bad.values()), (n, padded, bad)
        finite += int(np.isfinite(v).sum()); total += n
        if n >= 4 * N_CONSTRUCTED:      # the constructed pixels reach both clip bounds: -1 -> c / (4 w_g T), 0.999 -> 999 c / (2 w_g T)
            lo, hi = 3e8 / (4 * w_g * 1e6 * exposure_time), 999 * 3e8 / (2 * w_g * 1e6 * exposure_time)
            clipped_lo += int(np.isclose(pair_maps[:, :N_CONSTRUCTED], -lo, rtol=1e-9).sum())
            clipped_hi += int(np.isclose(pair_maps[:, :N_CONSTRUCTED], hi, rtol=1e-9).sum())
    # the comparison is about numbers: a generator that drowned it in NaN == NaN would not test the arithmetic
    print("finite expected pixels: %d of %d" % (finite, total))
    assert finite >= 0.8 * total, (finite, total)
    assert clipped_lo >= 3 * n_pairs and clipped_hi >= 3 * n_pairs, (clipped_lo, clipped_hi)


def test_first_pass_assigns_so_that_a_negative_zero_survives(mi, torch_scene):
    """acc = img, not 0 + img: -0.0 / W stays -0.0 in the sum of one pass, and the sum's previous content (here NaN) is overwritten, not added to"""
    import torch
    n = 65
    film = np.zeros((2, n, 4), np.float32)
    film[..., :3], film[..., 3] = -0.0, 2.0
    d_film = torch.from_numpy(film).cuda()
    d_sum = torch.full((2, n, 3), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    torch_scene.develop_accumulate_async(d_film.data_ptr(), 2, d_sum.data_ptr(), n, first=True)
    torch.cuda.synchronize()
    assert same(d_sum.cpu().numpy(), np.full((2, n, 3), -0.0, np.float32)) == 0
    torch_scene.develop_accumulate_async(d_film.data_ptr(), 2, d_sum.data_ptr(), n, first=False)      # -0 + -0 = -0; a later pass adds
    d_film2 = torch.from_numpy(np.full((2, n, 4), 3.0, np.float32)).cuda()
    torch_scene.develop_accumulate_async(d_film2.data_ptr(), 2, d_sum.data_ptr(), n, first=False)
    torch.cuda.synchronize()
    assert same(d_sum.cpu().numpy(), np.full((2, n, 3), 1.0, np.float32)) == 0


# ---------------------------------------------------------------- rendered
def rel_linf(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def host_route_tof(mi, sc, n_passes, spp, offsets, exposure_time):
    """the ToF images of harness.run_scene_velocity_map's host renders for these passes: seeds 0 .. n_passes - 1, one traversal per group and pass, numpy after that"""
    homo, hetero = [], []
    for g in range(0, len(offsets), 2):
        group = offsets[g:g + 2]
        variants = [(0.0, o) for o in group] + [(1.0, o) for o in group]
        acc = None
        for i in range(n_passes):
            img = sc.render(seed=i, spp=spp, variants=variants).astype(np.float32)
            acc = img if acc is None else acc + img
        images = acc / np.float32(n_passes)
        homo += [mi.to_tof_image(im, exposure_time) for im in images[:len(group)]]
        hetero += [mi.to_tof_image(im, exposure_time) for im in images[len(group):]]
    return homo, hetero


def check_rendered(mi, sc, n_passes, spp, offsets, exposure_time=0.0015, w_g=30):
    from mitsuba3dopplertof_amd import harness
    W, H = sc.size
    v, films, pairs = sc.render_velocity_map(n_passes, spp, offsets, exposure_time=exposure_time, w_g=w_g, pairs=True)
    assert v.shape == (H, W) and v.dtype == np.float64 and pairs.shape == (len(offsets), H, W)
    assert len(films["homodyne"]) == len(offsets) and len(films["heterodyne"]) == len(offsets)
    assert sc.last_stats["n_paths"] == W * H * spp * n_passes * ((len(offsets) + 1) // 2)
    assert sc.last_stats["n_bounces"] == 0 and sc.last_stats["n_shadow_rays"] == 0
    with np.errstate(all="ignore"):
        expected = harness.calc_velocity_from_homo_heteros(films["homodyne"], films["heterodyne"], exposure_time, w_g)
        assert same(v, expected) == 0, same(v, expected)
        for j in range(len(offsets)):
            one = harness.calc_velocity_from_homo_hetero(films["homodyne"][j], films["heterodyne"][j], exposure_time, w_g)
            assert same(pairs[j], one) == 0, (j, same(pairs[j], one))
    assert np.isfinite(expected).mean() > 0.9
    homo, hetero = host_route_tof(mi, sc, n_passes, spp, offsets, exposure_time)
    for j in range(len(offsets)):
        for name, got, ref in (("homodyne", films["homodyne"][j], homo[j]), ("heterodyne", films["heterodyne"][j], hetero[j])):
            assert got.dtype == np.float32 and np.abs(ref).max() > 0
            e = rel_linf(got, ref)
            print(name, "offset", offsets[j], "rel_linf", e)
            assert e <= IMG_TOL, (name, j, e)
    # without the per-pair maps: the same map
    v2, films2 = sc.render_velocity_map(n_passes, spp, offsets, exposure_time=exposure_time, w_g=w_g)
    with np.errstate(all="ignore"):
        assert same(v2, harness.calc_velocity_from_homo_heteros(films2["homodyne"], films2["heterodyne"], exposure_time, w_g)) == 0
    return v


@pytest.mark.parametrize("pipeline", ["fused", "split"])
@pytest.mark.parametrize("offsets", [(0.0, 0.25), (0.0, 0.25, 0.5)], ids=["two_offsets", "three_offsets"])
def test_rendered_velocity_map_on_the_wall(mi, offsets, pipeline, monkeypatch):
    import torch
    monkeypatch.setenv("DTOF_PIPELINE", pipeline)
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    W, H = sc.size
    # a layout the caller declared before the call holds after it, and behaves as before
    sc.set_film_layout(2, 4 * W * H + 64)
    check_rendered(mi, sc, 3, 8, list(offsets))
    assert sc.film_layout == (2, 4 * W * H + 64)
    film = torch.zeros((4, 4 * W * H + 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(mi.DtofError, match="declared with 2 planes, this call writes 4"):
        sc.render_rows(film.data_ptr(), 0, 8, 0, H, variants=[(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)])
    assert float(film.abs().sum()) == 0.0
    sc.render_rows(film.data_ptr(), 0, 8, 0, H, variants=[(0.0, 0.0), (1.0, 0.0)])
    torch.cuda.synchronize()
    planes = film.cpu().numpy()
    assert np.abs(planes[0, :4 * W * H]).sum() > 0 and np.abs(planes[1, :4 * W * H]).sum() > 0      # plane 1 at the declared stride
    assert np.abs(planes[:, 4 * W * H:]).sum() == 0 and np.abs(planes[2:]).sum() == 0
    # another exposure time and frequency reach the reconstruction as doubles
    check_rendered(mi, sc, 2, 8, list(offsets), exposure_time=0.002, w_g=150)


def test_rendered_velocity_map_on_an_rgba_scene(mi):
    """the alpha film is rendered into the library's film and ignored; the device-film calls still want the caller's declaration afterwards"""
    import torch
    sc = mi.load_file(os.path.join(SCENES, "open_veils.xml"), resx=24, resy=16, max_depth=5, pixel_format="rgba")
    assert sc.info()["has_alpha"]
    check_rendered(mi, sc, 3, 8, [0.0, 0.25, 0.5])
    assert sc.film_layout == (0, 0)
    film = torch.zeros((3, 16, 24, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(mi.DtofError, match="dtof_scene_set_film_layout"):
        sc.render_rows(film.data_ptr(), 0, 8, 0, 16, variants=[(0.0, 0.0), (1.0, 0.0)])
    assert float(film.abs().sum()) == 0.0


def test_frames_the_caller_has_not_collected_stay_his(mi):
    import torch
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    film = torch.zeros((16, 24, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sc.render_rows_async(film.data_ptr(), 0, 8, 0, 16)
    sc.render_velocity_map(2, 8, (0.0, 0.25))
    assert sc.last_stats["n_paths"] == 24 * 16 * 8 * 2
    st, ms = sc.collect()
    assert st["n_paths"] == 24 * 16 * 8 and len(ms) == 1


# ---------------------------------------------------------------- physics
def test_device_route_finds_the_walls_velocity(mi):
    """the settings of test_variants.test_velocity_map_from_one_traversal_per_pass: the wall moves at -10 m/s"""
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=32, resy=32)
    v, films = harness.run_scene_velocity_map_device(sc, total_spp=4096, time_sampling_method="antithetic", path_correlation_depth=16, max_depth=2)
    assert v.shape == (32, 32) and v.dtype == np.float64 and len(films["homodyne"]) == 2 and len(films["heterodyne"]) == 2
    assert all(f.shape == (32, 32) and f.dtype == np.float32 for f in films["homodyne"] + films["heterodyne"])
    centre = v[12:20, 12:20]
    print("median of the centre 8x8:", float(np.median(centre)))
    assert abs(np.median(centre) + 10.0) < 2.5, np.median(centre)
    assert sc.last_stats["n_paths"] == 32 * 32 * 1024 * 4      # 4 passes of 1024, one traversal each


# ---------------------------------------------------------------- refusals
def test_refused_calls_leave_device_buffers_alone(mi):
    import torch
    L = mi._lib()
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=8, resy=8)
    px = 64
    d_film = torch.full((4, px, 4), float(SENT32), dtype=torch.float32, device="cuda")
    d_sum = torch.full((4, px, 3), float(SENT32), dtype=torch.float32, device="cuda")
    d_tof = torch.full((4, px), float(SENT32), dtype=torch.float32, device="cuda")
    d_pairs = torch.full((2, px), float(SENT64), dtype=torch.float64, device="cuda")
    d_v = torch.full((px,), float(SENT64), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    v, pairs, tof = np.full(px, SENT64), np.full((17, px), SENT64), np.full((34, px), SENT32, np.float32)
    off = np.asarray([0.0, 0.25] * 9, np.float32)
    hom, het = np.asarray([0, 1] * 9, np.int32), np.asarray([2, 3] * 9, np.int32)
    st = mi._Stats()

    def render(scene=sc._h, n_passes=1, offsets=off.ctypes.data, n=2, T=0.0015, wg=30.0, out=v.ctypes.data):
        return L.dtof_render_velocity_map(scene, n_passes, 4, offsets, n, T, wg, out, pairs.ctypes.data, tof.ctypes.data, C.byref(st))

    def vmap(scene=sc._h, d=d_sum.data_ptr(), n=2, h=hom.ctypes.data, t=het.ctypes.data, n_passes=1, T=0.0015, wg=30.0, n_px=px, out=d_v.data_ptr()):
        return L.dtof_velocity_map_async(scene, d, n, h, t, n_passes, T, wg, n_px, d_tof.data_ptr(), d_pairs.data_ptr(), out)

    def accumulate(scene=sc._h, film=d_film.data_ptr(), planes=4, stride=0, d=d_sum.data_ptr(), n_px=px):
        return L.dtof_develop_accumulate_async(scene, film, planes, stride, d, n_px, 1)

    nan, inf = float("nan"), float("inf")
    cases = {"render null scene": lambda: render(scene=None), "render null offsets": lambda: render(offsets=None), "render null out": lambda: render(out=None),
             "render 0 offsets": lambda: render(n=0), "render 17 offsets": lambda: render(n=17), "render 0 passes": lambda: render(n_passes=0),
             "map null scene": lambda: vmap(scene=None), "map null sum": lambda: vmap(d=None), "map null homodyne": lambda: vmap(h=None),
             "map null heterodyne": lambda: vmap(t=None), "map null velocity": lambda: vmap(out=None), "map 0 pairs": lambda: vmap(n=0),
             "map 17 pairs": lambda: vmap(n=17), "map 0 passes": lambda: vmap(n_passes=0),
             "map plane 4 of 4": lambda: vmap(h=np.asarray([0, 4], np.int32).ctypes.data), "map plane -1": lambda: vmap(t=np.asarray([-1, 3], np.int32).ctypes.data),
             "accumulate null scene": lambda: accumulate(scene=None), "accumulate null film": lambda: accumulate(film=None),
             "accumulate null sum": lambda: accumulate(d=None), "accumulate 0 planes": lambda: accumulate(planes=0),
             "accumulate short stride": lambda: accumulate(stride=4 * px - 4)}
    for bad in (dict(T=0.0), dict(T=-1.0), dict(T=nan), dict(T=inf), dict(wg=0.0), dict(wg=-30.0), dict(wg=nan), dict(wg=inf)):
        cases["render %r" % bad] = lambda bad=bad: render(**bad)
        cases["map %r" % bad] = lambda bad=bad: vmap(**bad)
    for name, call in cases.items():
        assert call() == INVALID, (name, L.dtof_last_error())
    for plugin in ("path", "velocity"):
        sc.set_integrator(dict(type=plugin))
        assert render() == INVALID, plugin
        assert L.dtof_last_error() == b"modulation offsets only apply to the dopplertofpath integrator", (plugin, L.dtof_last_error())
    sc.collect()
    torch.cuda.synchronize()
    assert (v == SENT64).all() and (pairs == SENT64).all() and (tof == SENT32).all()
    for t, sentinel in ((d_film, SENT32), (d_sum, SENT32), (d_tof, SENT32), (d_pairs, SENT64), (d_v, SENT64)):
        assert (t.cpu().numpy() == sentinel).all()


# ---------------------------------------------------------------- stream
def test_async_pair_runs_on_the_callers_stream_behind_a_render(mi):
    """set_stream(torch stream): clear -> render -> accumulate -> map are queued without a host wait; the map is numpy's of the film the render left behind, which
    it can only be if the two kernels ran after the render's last splat"""
    import torch
    from mitsuba3dopplertof_amd import harness
    L = mi._lib()
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=64, resy=64)
    W, H = sc.size
    n = W * H
    variants = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]
    stream = torch.cuda.Stream()
    sc.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            film = torch.full((4, n, 4), 5.0, dtype=torch.float32, device="cuda")
            d_sum = torch.full((4, n, 3), float("nan"), dtype=torch.float32, device="cuda")
            d_v = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            sc.clear_async(film.data_ptr(), film.numel() * 4)
            sc.render_rows_async(film.data_ptr(), 0, 64, 0, H, variants=variants)
            sc.develop_accumulate_async(film.data_ptr(), 4, d_sum.data_ptr(), n, first=True)
            sc.velocity_map_async(d_sum.data_ptr(), (0, 1), (2, 3), 1, n, d_v.data_ptr())
        stream.synchronize()
        st, _ = sc.collect()
        assert st["n_paths"] == n * 64
        planes = film.cpu().numpy()
        assert np.abs(planes).sum() > 0
        developed = np.zeros((1, 4, n, 3), np.float32)
        d_rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(4):
            assert L.dtof_develop(film.data_ptr() + 16 * n * k, d_rgb.data_ptr(), n) == 0
            developed[0, k] = d_rgb.cpu().numpy()
        with np.errstate(all="ignore"):
            tof = mi.to_tof_image(developed[0], 0.0015)
            expected = harness.calc_velocity_from_homo_heteros([tof[0], tof[1]], [tof[2], tof[3]], 0.0015, 30)
        assert np.isfinite(expected).mean() > 0.9
        assert same(d_v.cpu().numpy(), expected) == 0
    finally:
        torch.cuda.synchronize()
        sc.set_stream(None)
