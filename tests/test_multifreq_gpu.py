"""A modulation frequency per variant -- (hetero_frequency, hetero_offset, w_g) triples, up to four evaluated in one traversal (dtof_render_variants_freq,
dtof_render_variants_freq_f64, dtof_sample_lanes_variants_freq) -- against the CPU oracle, which is asked once per variant with the integrator's hetero_frequency,
hetero_offset AND w_g set to that triple.

  lanes     every lane of every variant through the batched kernels, rgb as bit patterns: one scene per modulation call site of k_shade (the NEE commit in its
            register form and the inline shadow commit / k_shadow on the wall, the emitter-hit term, the every-BSDF kernels, the resident several-film kernel that
            forms its weights at commit time from the parked path length), K = 1 .. 4, every waveform in the full modulation (where w_g itself enters)
  distinct  two variants equal in (f, o) and different in w_g give different lanes: a w_g shared by the films fails this
  null      no frequencies: the bits of sample_lanes_variants / render(variants=pairs)
  films     render(variants=triples) against the oracle's films; the float64 film within one float32 ulp of render_exact"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import SCENES
import test_variants as tv

pytestmark = pytest.mark.gpu

IMG_TOL, PX_TOL, NCPU = tv.IMG_TOL, tv.PX_TOL, tv.NCPU
bits, rel_linf, rel_linf_px, integrator_of = tv.bits, tv.rel_linf, tv.rel_linf_px, tv.integrator_of

# the four films of a two-frequency depth map: I and Q at 30 and at 40 MHz
SET_K4 = [(0.0, 0.0, 30.0), (0.0, 0.25, 30.0), (0.0, 0.0, 40.0), (0.0, 0.25, 40.0)]
SET_K2 = [(1.0, 0.1, 17.3), (-0.7, 0.9, 151.7)]       # frequencies float32 cannot represent
SET_K3 = [(2.5, 0.5, 23.0), (0.0, 0.125, 77.7), (-1.0, 0.7, 30.0)]
SET_K1 = [(0.37, 0.6, 53.0)]                         # one film, at a w_g other than the scene's 30 MHz
SETS = {"k4": SET_K4, "k2": SET_K2, "k3": SET_K3, "k1": SET_K1}


def oracle_params(osc, base, variant):
    f, o, g = (float(np.float32(x)) for x in variant)
    return osc.params(integrator=dict(base, hetero_frequency=f, hetero_offset=o, w_g=g))


def check_lanes(mi, orc, path, params, spp, variants, integrator=None, seed=2, what=""):
    """every lane of the frame, every variant, against the oracle; returns the scene and the GPU lanes"""
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    base = integrator if integrator is not None else integrator_of(osc)
    if integrator is not None:
        sc.set_integrator(integrator)
    w, h = sc.size
    n = w * h * spp
    g = sc.sample_lanes_variants(seed, spp, 0, n, variants)
    assert g["rgb"].shape == (len(variants), n, 3)
    lit = 0
    for k, v in enumerate(variants):
        o = osc.render_lanes(oracle_params(osc, base, v), seed, spp, 0, n, threads=NCPU)
        for f in ("sample_pos", "time", "ray_o", "ray_d"):
            assert np.array_equal(bits(g[f]), bits(o[f])), (what, v, f, int((bits(g[f]) != bits(o[f])).sum()))
        assert np.array_equal(g["valid"], o["valid"]), (what, v, "valid")
        bad = (bits(g["rgb"][k]) != bits(o["rgb"])).any(axis=1)
        assert not bad.any(), (what, "variant %d %s" % (k, (v,)), "%d of %d lanes differ" % (int(bad.sum()), n))
        lit += int((o["rgb"] != 0).any(axis=1).sum())
    assert lit > 0, what
    return sc, g


# one scene per modulation call site: (scene, -D parameters, spp, environment settings)
SCENE_CASES = {
    "wall": ("cornell_wall.xml", dict(resx=24, resy=16), 8, (tv.FUSED, tv.SPLIT)),                         # plain kernels: NEE commit in registers, inline shadow commit, k_shadow
    "area": ("cornell_area.xml", dict(resx=24, resy=16, max_depth=5), 8, (tv.FUSED,)),                     # the emitter-hit term
    "spec1": ("cornell_roughplastic.xml", dict(resx=24, resy=16, max_depth=5), 8, (tv.FUSED,)),            # every-BSDF kernels
    "domino_resident": ("domino.xml", dict(resx=48, resy=32), 4, (tv.resident(8),)),                       # the resident several-film kernel: weights formed at commit time
}
LANE_CASES = [(name, s) for name, c in SCENE_CASES.items() for s in range(len(c[3]))]


@pytest.mark.parametrize("case", LANE_CASES, ids=lambda c: c[0] + "-" + tv._env_id(SCENE_CASES[c[0]][3][c[1]]))
def test_lanes_of_every_modulation_call_site_two_frequencies(mi, orc, case, monkeypatch):
    name, s = case
    xml, params, spp, envs = SCENE_CASES[name]
    for k, v in envs[s].items():
        monkeypatch.setenv(k, v)
    check_lanes(mi, orc, os.path.join(SCENES, xml), params, spp, SET_K4, what=name)


@pytest.mark.parametrize("pipeline", ["fused", "split"])
@pytest.mark.parametrize("vset", ["k2", "k3", "k1"])
def test_lanes_other_variant_counts(mi, orc, vset, pipeline, monkeypatch):
    monkeypatch.setenv("DTOF_PIPELINE", pipeline)
    check_lanes(mi, orc, os.path.join(SCENES, "cornell_wall.xml"), dict(resx=24, resy=16), 8, SETS[vset], what=(vset, pipeline))


@pytest.mark.parametrize("wave", ["sinusoidal", "rectangular", "triangular", "trapezoidal"])
def test_lanes_full_modulation_every_waveform(mi, orc, wave, monkeypatch):
    """low_frequency_component_only = false: w_g * t - phi and (w_g + w_d) * t + phase are formed per film"""
    monkeypatch.setenv("DTOF_PIPELINE", "fused")
    integ = dict(type="dopplertofpath", max_depth=4, w_g=30.0, hetero_frequency=1.0, hetero_offset=0.4, path_correlation_depth=4, time_sampling_method="antithetic",
                 antithetic_shift=0.5, wave_function_type=wave, low_frequency_component_only=False)
    for vset in ("k4", "k2"):
        check_lanes(mi, orc, os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16), 8, SETS[vset], integrator=integ, what=(wave, vset))


def test_two_variants_that_differ_in_w_g_alone_give_different_lanes(mi):
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    n = 24 * 16 * 8
    g = sc.sample_lanes_variants(2, 8, 0, n, [(0.0, 0.25, 30.0), (0.0, 0.25, 40.0)])["rgb"]
    lit = (g[0] != 0).any(axis=1) | (g[1] != 0).any(axis=1)
    differ = (bits(g[0]) != bits(g[1])).any(axis=1)
    assert lit.sum() > n // 4
    assert differ[lit].mean() > 0.9, float(differ[lit].mean())      # a shared w_g would make every lane equal
    same = sc.sample_lanes_variants(2, 8, 0, n, [(0.0, 0.25, 30.0), (0.0, 0.25, 30.0)])["rgb"]
    assert np.array_equal(bits(same[0]), bits(same[1])) and np.array_equal(bits(same[0]), bits(g[0]))


def test_a_null_frequency_array_is_the_entry_without_frequencies(mi):
    L = mi._lib()
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    pairs = tv.SET_K4
    var = np.ascontiguousarray(pairs, np.float32)
    n, spp = 24 * 16 * 8, 8
    ref = sc.sample_lanes_variants(3, spp, 0, n, pairs)
    lanes, valid, rgb = np.zeros((n, 12), np.float32), np.zeros(n, np.uint32), np.zeros((4, n, 3), np.float32)
    assert L.dtof_sample_lanes_variants_freq(sc._h, 3, spp, var.ctypes.data, None, 4, 0, n, lanes.ctypes.data, valid.ctypes.data, rgb.ctypes.data) == 0
    assert np.array_equal(bits(rgb), bits(ref["rgb"])) and np.array_equal(valid, ref["valid"]) and np.array_equal(bits(lanes[:, 0:2]), bits(ref["sample_pos"]))
    # the scene's own 30 MHz as triples: the same lanes again
    own = sc.sample_lanes_variants(3, spp, 0, n, [(f, o, 30.0) for f, o in pairs])
    assert np.array_equal(bits(own["rgb"]), bits(ref["rgb"]))
    # the float64 film has no atomics' order in it: render(variants=pairs) bit for bit, through the _freq entry with a null array and with 30 MHz
    st = mi._Stats()
    img_ref = sc.render(seed=3, spp=spp, variants=pairs, film="float64")
    img = np.zeros_like(img_ref)
    assert L.dtof_render_variants_freq_f64(sc._h, 3, spp, var.ctypes.data, None, 4, img.ctypes.data, None, C.byref(st)) == 0
    assert np.array_equal(bits(img), bits(img_ref))
    assert np.array_equal(bits(sc.render(seed=3, spp=spp, variants=[(f, o, 30.0) for f, o in pairs], film="float64")), bits(img_ref))
    # ... and the float32 film within the order of its sums
    img32 = np.zeros_like(img_ref)
    assert L.dtof_render_variants_freq(sc._h, 3, spp, var.ctypes.data, None, 4, img32.ctypes.data, C.byref(st)) == 0
    assert rel_linf(img32, sc.render(seed=3, spp=spp, variants=pairs)) <= IMG_TOL


@pytest.fixture(scope="module")
def boxes_films(orc):
    """the oracle's films of six triples on cornell_boxes, computed once: (path, params, variants, [(render, render_exact) per variant])"""
    path, params = os.path.join(SCENES, "cornell_boxes.xml"), dict(resx=32, resy=32, wave_function_type="trapezoidal")
    osc = orc.Scene(path, params)
    variants = SET_K4 + SET_K2
    refs = []
    for v in variants:
        pd = oracle_params(osc, integrator_of(osc), v)
        refs.append((osc.render(pd, seed=2, spp=16, threads=NCPU)[0], osc.render_exact(pd, seed=2, spp=16, threads=NCPU)[0]))
    return path, params, variants, refs


def test_films_of_render_triples_match_the_oracle(mi, boxes_films):
    path, params, variants, refs = boxes_films
    sc = mi.load_file(path, **params)
    films = sc.render(seed=2, spp=16, variants=variants)
    assert films.shape == (6, 32, 32, 3)
    assert sc.last_stats["n_paths"] == 2 * 32 * 32 * 16        # two traversals for six films
    for k, v in enumerate(variants):
        e, e_px = rel_linf(films[k], refs[k][0]), rel_linf_px(films[k], refs[k][1])
        print("variant", v, "rel_linf", e, "rel_linf_px", e_px)
        assert e <= IMG_TOL, (v, e)
        assert e_px <= PX_TOL, (v, e_px)


def test_the_float64_film_of_triples_is_render_exact_to_one_ulp(mi, boxes_films):
    """tests/test_film64_gpu.py's criterion: the developed float64 film against the order-independent film, one float32 ulp"""
    path, params, variants, refs = boxes_films
    sc = mi.load_file(path, **params)
    images, films = sc.render_film64(seed=2, spp=16, variants=variants[:4])
    assert images.shape == (4, 32, 32, 3) and films.shape == (4, 32, 32, 4)
    assert sc.last_stats["n_paths"] == 32 * 32 * 16
    for k in range(4):
        err = rel_linf_px(images[k], refs[k][1])
        print("variant", variants[k], "rel_linf_px", err, "bound", 2.0 ** -23)
        assert err <= 2.0 ** -23, (variants[k], err)      # test_film64_gpu.IMG_BOUND
