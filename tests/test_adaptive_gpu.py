"""Adaptive sampling on the device: renders over a pixel list, the selection kernels, the driver loop.

  lanes      Scene.sample_lanes_pixels, bit for bit, against the oracle's render_lanes at the global indices pixel * spp + sample and against sample_lanes_variants of
             the same library there: a list is the dense render's lanes, stream for stream.
  films      the raw moment planes and the raw float64 film of ONE traversal of a list against the oracle's lanes masked to the listed pixels and pushed through
             moments_ref.footprint / splat (adaptive_ref.Lanes).  Criterion, the project's own: |device - expected| <= 2^-40 * sum |term| per pixel and plane (both sides
             add the same float32 terms in double in different orders; <= 2^12 terms a pixel, 2^-53 per addition).  A pixel outside every listed footprint has no term
             and must be exactly 0.  A request with both films is held to the same bound as a request with either alone.
  selection  mi.adaptive_select over seeded synthetic planes against adaptive_ref.select: the operation order is fixed and the device's double division and square root
             are correctly rounded, so the metric map is equal BIT FOR BIT (NaN positions equal), the list is np.flatnonzero(selected) and count is exact.
  driver     Scene.render_adaptive: the films within the bound of the sum over the passes of the oracle's lanes masked by the RETURNED lists, count from the lists, and
             (image mode) every list equal to adaptive_ref.select of the EXPECTED sums after the pass before it, outside a guard band that the reference data itself must
             leave empty (see test_driver_image_mode)."""
import os

import numpy as np
import pytest

from conftest import SCENES
import adaptive_ref as aref
import moments_ref as ref
from test_moments_gpu import _xml, planes_of

pytestmark = pytest.mark.gpu

SEED = 3
K4 = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]
FIELDS = ("sample_pos", "time", "ray_o", "ray_d")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def lists_of(n_px):
    return {"first": [0], "last": [n_px - 1], "every_other": list(range(0, n_px, 2)), "full": list(range(n_px))}


# id -> (scene, -D parameters, spp, variants, which lists, integrator dict or None, environment)
LANE_CASES = {
    "wall_64spp": ("cornell_wall.xml", dict(resx=16, resy=16), 64, None, ("first", "last", "every_other", "full"), None, {}),      # a wave per pixel (run-time wave_pixel)
    "wall_64spp_split": ("cornell_wall.xml", dict(resx=16, resy=16), 64, None, ("first", "last", "every_other", "full"), None, {"DTOF_PIPELINE": "split"}),
    "wall_128spp_K4": ("cornell_wall.xml", dict(resx=16, resy=16), 128, K4, ("every_other", "full"), None, {}),                     # two waves per pixel, four films
    "wall_4spp_three_pixels": ("cornell_wall.xml", dict(resx=16, resy=16), 4, None, ("three", "full"), None, {}),                   # 12 lanes: no whole wave
    "wall_4spp_three_pixels_K4": ("cornell_wall.xml", dict(resx=16, resy=16), 4, K4, ("three", "last"), None, {}),
    "wall_16spp_small_batches": ("cornell_wall.xml", dict(resx=16, resy=16), 16, None, ("every_other",), None, {"DTOF_BATCH_LANES": "1000"}),   # batches of 62 whole pixels
    "boxes_16spp": ("cornell_boxes.xml", dict(resx=16, resy=16), 16, None, ("first", "last", "every_other", "full"), None, {}),
    "domino_small_4spp": ("domino_small.xml", dict(resx=32, resy=32), 4, None, ("first", "last", "every_other", "full"), None, {}),
    "boxes_periodic_tcn4": ("cornell_boxes.xml", dict(resx=16, resy=16, time_correlate_number=4, time_sampling_method="periodic"), 8, None,
                            ("first", "every_other", "full"), None, {}),                                                              # groups of four by GLOBAL lane
    "wall_path_1spp": ("cornell_wall.xml", dict(resx=16, resy=16), 1, None, ("first", "last", "every_other", "full"), dict(type="path", max_depth=3, time_sampling_method="uniform"), {}),      # (1 spp: no per-interval stratification)
}


@pytest.mark.parametrize("case", list(LANE_CASES))
def test_lanes_of_a_pixel_list(mi, orc, case, monkeypatch):
    scene, params, spp, variants, which, integ, env = LANE_CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    path = os.path.join(SCENES, scene)
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    if integ:
        sc.set_integrator(integ)
    w, h = sc.size
    n_px = w * h
    if integ:
        pd = osc.params(integrator=integ)
    elif variants:
        pd = osc.params(integrator=ref.integrator_of(osc, hetero_frequency=float(variants[0][0]), hetero_offset=float(variants[0][1])))
    else:
        pd = osc.params()
    want = osc.render_lanes(pd, SEED, spp, 0, n_px * spp, threads=ref.NCPU)
    dense = sc.sample_lanes_variants(SEED, spp, 0, n_px * spp, variants)
    lists = dict(lists_of(n_px), three=[3, 100, n_px - 1])
    for name in which:
        pixels = np.asarray(lists[name], np.int64)
        idx = (pixels[:, None] * spp + np.arange(spp)[None, :]).reshape(-1)
        got = sc.sample_lanes_pixels(SEED, spp, pixels, variants)
        assert got["rgb"].shape == (len(variants) if variants else 1, len(idx), 3), (case, name)
        for f in FIELDS:
            assert np.array_equal(bits(got[f]), bits(want[f][idx])), (case, name, f, "against the oracle")
            assert np.array_equal(bits(got[f]), bits(dense[f][idx])), (case, name, f, "against the dense lanes")
        assert np.array_equal(bits(got["rgb"][0]), bits(want["rgb"][idx])), (case, name, "rgb against the oracle")
        assert np.array_equal(bits(got["rgb"]), bits(dense["rgb"][:, idx])), (case, name, "rgb of every film against the dense lanes")
        assert np.array_equal(got["valid"], want["valid"][idx]) and np.array_equal(got["valid"], dense["valid"][idx]), (case, name, "valid")
        assert np.abs(want["rgb"][idx]).max() > 0 or name in ("first", "last"), (case, name)
    assert sc.sample_lanes_pixels(SEED, spp, [], variants)["time"].shape == (0,)      # an empty list launches nothing and returns nothing


def hold(what, got, want, mags, factor=1.0):
    ratios = ref.errors_over_bound(got, want, mags)
    print("%s: largest error / bound per plane: %s" % (what, " ".join("%.3g" % r for r in ratios)))
    assert np.abs(want).max() > 0, what
    assert (ratios <= factor).all(), (what, ratios)


# id -> (scene, -D parameters, spp, edit, variants)
FILM_CASES = {
    "tent_K1": ("cornell_wall.xml", dict(resx=16, resy=16), 16, None, None),
    "tent_K2": ("cornell_wall.xml", dict(resx=16, resy=16), 16, None, K4[:2]),
    "tent_K4_64spp": ("cornell_wall.xml", dict(resx=16, resy=16), 64, None, K4),
    "box_K2": ("cornell_wall.xml", dict(resx=16, resy=16), 16, "box", K4[1:3]),
    "gaussian_K1": ("cornell_rough.xml", dict(resx=24, resy=24, max_depth=5), 8, "gaussian", None),
    "crop_K1": ("cornell_wall.xml", dict(resx=32, resy=24), 8, "crop", None),
    "rgba_K2": ("cornell_wall.xml", dict(resx=16, resy=16), 16, "rgba", K4[:2]),
}


@pytest.mark.parametrize("case", list(FILM_CASES))
def test_films_of_a_pixel_list(mi, orc, case):
    scene, params, spp, edit, variants = FILM_CASES[case]
    xml = _xml(scene, edit)
    sc, osc = mi.load_string(xml, **params), orc.Scene(xml, params, is_string=True)
    w, h = sc.size
    n_px, K, alpha = w * h, len(variants) if variants else 1, edit == "rgba"
    lanes = aref.Lanes(orc, osc, SEED, spp, variants)
    rng = np.random.default_rng(7)
    lists = {"every_other": np.arange(0, n_px, 2), "random_tenth": np.sort(rng.permutation(n_px)[:max(n_px // 10, 3)]), "full": np.arange(n_px)}
    for name, pixels in lists.items():
        want, mags, fwant, fmags = lanes.sums(pixels, film=True, alpha=alpha)
        both = sc.render_pixels(pixels, SEED, spp, variants, raw=True, films=True)
        assert sc.last_stats["n_paths"] == len(pixels) * spp and sc.last_stats["n_fused_splat_launches"] == 0, sc.last_stats
        assert both["film64"].shape == (K + (1 if alpha else 0), h, w, 4) == fwant.shape
        hold("%s %s moments (both films)" % (case, name), planes_of(both), want, mags)
        hold("%s %s float64 film (both films)" % (case, name), both["film64"], fwant, fmags)
        if name == "random_tenth":      # pixels outside every listed footprint exist, and errors_over_bound has held them to exactly 0
            assert (mags[0] == 0).any() and not planes_of(both)[:, mags[0] == 0].any() and not both["film64"][fmags == 0].any()
        alone = sc.render_pixels(pixels, SEED, spp, variants, raw=True)
        hold("%s %s moments alone" % (case, name), planes_of(alone), want, mags)
        film_alone = sc.render_pixels(pixels, SEED, spp, variants, films=True, moments=False)["film64"]
        hold("%s %s float64 film alone" % (case, name), film_alone, fwant, fmags)
    # the full list is the dense render (same bound: another order of the same terms)
    hold(case + " full list against render_moments", planes_of(both), planes_of(sc.render_moments(SEED, spp, variants=variants, raw=True)), mags)
    if alpha:
        assert fwant[K][..., 0].max() > 0 and (fwant[K][..., 1:3] == 0).all()      # the alpha film is (A, 0, 0, W), behind the colour planes; the moments never hold it
    empty = sc.render_pixels([], SEED, spp, variants, raw=True, films=True)
    assert not planes_of(empty).any() and not empty["film64"].any() and sc.last_stats["n_paths"] == 0


# ---------------------------------------------------------------------------- the selection over arrays
SIZES = (1, 63, 64, 65, 255, 256, 257, 256 * 256 + 300)      # the last: more block counts (258) than ONE scan block takes (256): two scan levels and the add between them; every other size is one level
CONFIGS = {"image_K1": ("image", 1, ()), "image_K2": ("image", 2, ()), "image_K3": ("image", 3, ()), "image_K4": ("image", 4, ()),
           "velocity_K2_1pair": ("velocity", 2, ((0, 1),)), "velocity_K3_1pair": ("velocity", 3, ((2, 1),)), "velocity_K4_2pairs": ("velocity", 4, ((0, 1), (2, 3)))}
DENSITIES = ("none", "all", "alternating", "one_percent", "half")


def _selection_inputs(config, density, n, seed):
    """(S, count, tol) with the two classes of adaptive_ref.synthetic separated by tol; edge values only where the density is a rate, not a pattern"""
    mode, K, pairs = CONFIGS[config]
    rng = np.random.default_rng(seed)
    noisy = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0, "one_percent": rng.random(n) < 0.01,
             "half": rng.random(n) < 0.5}[density]
    S, count = aref.synthetic(rng, n, K, noisy, edges=density in ("one_percent", "half"))
    # quiet pixels: var <= 2e-10, noisy: >= 0.5, count in [16, 64].  image: sqrt(var / n) / max(|mean|, 1e-3) is <= 3.6e-6 / 1e-3 against >= 0.088 / 2 (variant 0's mean
    # is at most 2); velocity: sqrt(var_r) slope with slope in (830, 16700) and |correlation| < 0.9 is <= 0.25 against >= 11.  The tolerances lie between the classes.
    tol = {"image": 1e-2, "velocity": 3.0}[mode]
    return S, count, tol, noisy


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_selection_over_arrays(mi, config, density):
    mode, K, pairs = CONFIGS[config]
    for n in SIZES:
        S, count, tol, noisy = _selection_inputs(config, density, n, 1000 * K + n)
        want_list, want_metric, want_count = aref.select(S, K, count, 8, mode, tol, floor=1e-3, pairs=pairs)
        with np.errstate(all="ignore"):
            assert not (want_metric == tol).any(), "an input sits exactly at tol: choose another seed"
        if density in ("none", "all", "alternating"):      # the classes are separated by tol: the pattern IS the selection
            assert np.array_equal(want_list, np.flatnonzero(noisy)), (config, density, n)
        got_list, got_metric, got_count = mi.adaptive_select(S, count, 8, mode=mode, tol=tol, floor=1e-3, pairs=pairs or None)
        assert np.array_equal(np.isnan(got_metric), np.isnan(want_metric)), (config, density, n)
        ok = ~np.isnan(want_metric)
        assert np.array_equal(got_metric[ok].view(np.uint64), want_metric[ok].view(np.uint64)), (config, density, n, int((got_metric[ok] != want_metric[ok]).sum()))
        assert got_list.dtype == np.uint32 and np.array_equal(got_list, want_list), (config, density, n, len(got_list), len(want_list))
        assert np.array_equal(got_count, want_count), (config, density, n)
    print("%s %s: %d of %d selected at the largest size" % (config, density, len(want_list), n))


# ---------------------------------------------------------------------------- the driver
WALL16 = ("cornell_wall.xml", dict(resx=16, resy=16))
# chosen on the CPU from the oracle alone: with them the reference selection of test_driver_image_mode leaves the guard band empty and every list is non-trivial
IMAGE_TOL, IMAGE_FLOOR, IMAGE_SEED = 0.35, 1e-3, 3
VELOCITY_TOL = 1500.0      # m/s: about the median standard error of this 16 x 16 map after one pass of 16 spp, so the lists are proper subsets


def raw_2d(planes):
    return np.asarray(planes).reshape(len(planes), -1)


def test_driver_with_an_infinite_tolerance_is_one_dense_pass(mi, orc):
    path = os.path.join(SCENES, WALL16[0])
    sc, osc = mi.load_file(path, **WALL16[1]), orc.Scene(path, WALL16[1])
    r = sc.render_adaptive(seed=SEED, spp=16, base_passes=1, max_passes=4, variants=K4[:2], mode="image", tol=float("inf"), raw=True, films=True, lists=True)
    assert list(r["pass_pixels"]) == [256] and r["lists"] == [] and (r["count"] == 16).all() and sc.last_stats["n_paths"] == 256 * 16
    want, mags, fwant, fmags = aref.Lanes(orc, osc, SEED, 16, K4[:2]).sums(np.arange(256), film=True)
    hold("tol = inf: moments", planes_of(r), want, mags)
    hold("tol = inf: float64 film", r["film64"], fwant, fmags)
    assert r["metric"].shape == (16, 16) and (r["metric"] >= 0).all()
    # an empty selection right after the base pass, and max_passes == base_passes, return cleanly
    one = sc.render_adaptive(seed=SEED, spp=16, base_passes=2, max_passes=2, variants=K4[:2], mode="image", tol=0.0, raw=True)
    assert list(one["pass_pixels"]) == [256, 256] and (one["count"] == 32).all()
    images = sc.render_adaptive(seed=SEED, spp=16, base_passes=1, max_passes=1, variants=K4[:2])["images"]
    assert images.shape == (2, 16, 16, 3) and images.dtype == np.float32
    f64 = sc.render(seed=SEED, spp=16, variants=K4[:2], film="float64")
    assert np.abs(images - f64).max() <= 2.0 ** -20 * np.abs(f64).max()      # the images are the float64 film developed: two orders of the same sums


def test_driver_image_mode(mi, orc):
    """GUARD BAND.  Device and expected sums agree to 2^-40 of their magnitudes; the metric sqrt(var / n) / |mean| with var = m2 - mean^2 amplifies a relative error of
    the sums by at most about m2 / var.  The test asserts ON THE REFERENCE DATA that m2_Y / var_Y <= 2^16 wherever var_Y > 0 -- then the device's metric is within
    2^-40 * 2^16 * (a few) < 2^-20 relative of the reference's -- and exempts pixels whose reference metric lies within 2^-20 * tol of tol.  It also asserts that the
    reference puts NO pixel into that band (a condition on tol and seed, verified with the oracle before this test was committed), so every list is compared whole."""
    path = os.path.join(SCENES, WALL16[0])
    sc, osc = mi.load_file(path, **WALL16[1]), orc.Scene(path, WALL16[1])
    spp, variants = 16, K4[:2]
    r = sc.render_adaptive(seed=IMAGE_SEED, spp=spp, base_passes=1, max_passes=4, variants=variants, mode="image", tol=IMAGE_TOL, floor=IMAGE_FLOOR, raw=True, films=True,
                           lists=True)
    got_lists = r["lists"]
    assert len(got_lists) == len(r["pass_pixels"]) - 1 and [len(x) for x in got_lists] == list(r["pass_pixels"][1:])
    # the films: the sum over the passes of the oracle's lanes masked by the RETURNED lists
    total, count = None, np.zeros(256, np.int64)
    sums_after = []
    for p, pixels in enumerate([np.arange(256)] + got_lists):
        assert (np.diff(np.asarray(pixels, np.int64)) > 0).all() and len(pixels) > 0
        part = aref.Lanes(orc, osc, IMAGE_SEED + p, spp, variants).sums(pixels, film=True)
        total = part if total is None else tuple(a + b for a, b in zip(total, part))
        sums_after.append(total[0])
        count[np.asarray(pixels, np.int64)] += spp
    hold("image mode: moments", planes_of(r), total[0], total[1])
    hold("image mode: float64 film", r["film64"], total[2], total[3])
    assert np.array_equal(r["count"].reshape(-1), count)
    assert sc.last_stats["n_paths"] == count.sum()
    # the lists: adaptive_ref's selection from the EXPECTED sums after the pass before
    cnt = np.full(256, spp, np.uint32)
    for p, got in enumerate(got_lists):
        S = raw_2d(sums_after[p])
        mean, var, _ = aref.variant_stats(S, 2)
        m2 = var + mean * mean
        assert (m2[var > 0] / var[var > 0] <= 2.0 ** 16).all(), "the metric's amplification of the sums' error is not bounded by 2^16 on this data"
        want, metric, cnt_next = aref.select(S, 2, cnt, spp, "image", IMAGE_TOL, floor=IMAGE_FLOOR)
        band = np.abs(metric - IMAGE_TOL) <= 2.0 ** -20 * IMAGE_TOL
        assert not band.any(), "the reference puts a pixel into the guard band: choose another tol or seed"
        print("image mode pass %d: %d pixels selected, closest metric to tol %.6g (tol %.3g)" % (p + 1, len(want), metric[np.argmin(np.abs(metric - IMAGE_TOL))], IMAGE_TOL))
        assert np.array_equal(np.asarray(got)[~band[got]], want[~band[want]]), (p, len(got), len(want))
        cnt = cnt_next
    assert 0 < len(got_lists[-1]) < 256 and len(got_lists) >= 2      # the loop did select, and not everything
    # the final metric is that of the final cells and counts
    final_metric, _ = aref.image_metric(raw_2d(total[0]), 2, count.astype(np.uint32), IMAGE_FLOOR)
    assert np.abs(r["metric"].reshape(-1) - final_metric).max() <= 2.0 ** -20 * final_metric.max()


def test_driver_velocity_mode(mi, orc):
    """K = 4, two pairs: the lists are ascending and inside the film, the cells within the bound given those lists, count consistent with them.  (That the selection
    is the right one in this mode rests on test_selection_over_arrays.)"""
    path = os.path.join(SCENES, WALL16[0])
    sc, osc = mi.load_file(path, **WALL16[1]), orc.Scene(path, WALL16[1])
    spp, pairs = 16, [(0, 2), (1, 3)]
    r = sc.render_adaptive(seed=SEED, spp=spp, base_passes=1, max_passes=3, variants=K4, mode="velocity", tol=VELOCITY_TOL, pairs=pairs, raw=True, films=True, lists=True)
    total, count = None, np.zeros(256, np.int64)
    for p, pixels in enumerate([np.arange(256)] + r["lists"]):
        pixels = np.asarray(pixels, np.int64)
        assert (np.diff(pixels) > 0).all() and 0 <= pixels.min() and pixels.max() < 256
        part = aref.Lanes(orc, osc, SEED + p, spp, K4).sums(pixels, film=True)
        total = part if total is None else tuple(a + b for a, b in zip(total, part))
        count[pixels] += spp
    print("velocity mode: passes of %s pixels" % list(r["pass_pixels"]))
    assert len(r["lists"]) >= 1 and [len(x) for x in r["lists"]] == list(r["pass_pixels"][1:])
    hold("velocity mode: moments", planes_of(r), total[0], total[1])
    hold("velocity mode: float64 film", r["film64"], total[2], total[3])
    assert np.array_equal(r["count"].reshape(-1), count)
    # the loop ends as soon as a list comes back empty: a tolerance no error reaches, after three base passes, which on this frame leave every pair with a usable
    # ratio well inside the clip interval (checked on the reference's sums: a pair without one selects its pixel whatever the tolerance -- after one or two base
    # passes a few pixels still do)
    base = None
    for p in range(3):
        part = aref.Lanes(orc, osc, SEED + p, spp, K4).sums(np.arange(256))
        base = part if base is None else tuple(a + b for a, b in zip(base, part))
    none, metric, _ = aref.select(raw_2d(base[0]), 4, np.full(256, 3 * spp, np.uint32), spp, "velocity", 1e30, pairs=pairs)
    mean, _, _ = aref.variant_stats(raw_2d(base[0]), 4)
    ratios = np.stack([mean[t] / mean[h] for h, t in pairs])
    print("velocity mode, three base passes: ratios in [%.4f, %.4f], largest standard error %.4g m/s" % (ratios.min(), ratios.max(), metric.max()))
    assert len(none) == 0 and np.isfinite(metric).all() and ratios.min() > -1.0 + 1e-6 and ratios.max() < 0.999 - 1e-6
    early = sc.render_adaptive(seed=SEED, spp=spp, base_passes=3, max_passes=6, variants=K4, mode="velocity", tol=1e30, pairs=pairs, lists=True)
    assert list(early["pass_pixels"]) == [256, 256, 256] and early["lists"] == [] and (early["count"] == 3 * spp).all() and np.isfinite(early["metric"]).all()
    # the harness on top: the map of calc_velocity_from_homo_heteros, its standard error and the count
    from mitsuba3dopplertof_amd import harness
    v, se, cnt = harness.velocity_map_adaptive(sc, spp, 3, VELOCITY_TOL, offsets=(0.0, 0.25), seed=SEED)
    assert v.shape == se.shape == cnt.shape == (16, 16) and np.array_equal(cnt.reshape(-1), count) and np.isfinite(v).all()
