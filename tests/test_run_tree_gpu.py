"""The run reduction of the double-accumulating splats (run_sum and the run walk of csrc/dtof_splat64.h, under k_splat_f64, k_splat_moments_f64 and k_aov), pinned BIT
FOR BIT where the film cannot depend on the order of its atomics.

With the box filter a lane splats at its own pixel, and lane = pixel * spp + sample (include/dtof.h): a pixel's spp lanes are consecutive.  When 64 % spp == 0 they
are exactly one run inside one wave, every film cell receives exactly ONE atomic per plane, and that atomic's value is the run's Hillis-Steele tree over the lanes'
terms in lane order.  The emulation, per run of L lanes, over the terms as doubles:
    for s = 0 .. 5 while 2^s < L:  v[2^s:] = v[2^s:] + v[:-2^s]   (from the old values);  the cell's value is the last element
The terms come from the device's own lanes (sample_lanes_variants, sample_aov_lanes), which test_gpu_parity.py, test_variants.py and test_aov_gpu.py hold to the oracle
bit for bit; the box filter adds the value itself and 1 for the weight.  A sum of zero is not added: the film keeps its +0.
Shapes: cornell_wall 16 x 16, 16 spp (four runs per wave) and 64 spp (a run is a wave)."""
import numpy as np
import pytest

import moments_ref as ref
from test_aov_gpu import SPEC6, planes_of as aov_planes_of
from test_moments_gpu import K4, SEED, load, planes_of as moment_planes_of

pytestmark = pytest.mark.gpu

SIDE = 16


def tree(terms):
    """(pixels, L, P) terms in lane order -> (pixels, P): the last lane of run_sum's tree"""
    v = np.array(terms, np.float64)
    s = 1
    while s < v.shape[1]:
        v[:, s:] = v[:, s:] + v[:, :-s]      # the right-hand side is evaluated from the old values
        s *= 2
    return v[:, -1] + 0.0                    # a sum of -0 is skipped like every zero: the film's +0


def planes(values, spp):
    """(lanes, P) float32 values -> the expected raw planes (P, H, W)"""
    v = np.ascontiguousarray(values, np.float32).astype(np.float64)
    return np.moveaxis(tree(v.reshape(SIDE * SIDE, spp, -1)), -1, 0).reshape(-1, SIDE, SIDE)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((got.view(np.uint64) != want.view(np.uint64)).sum())


@pytest.fixture(scope="module", params=[16, 64], ids=["16spp", "64spp"])
def wall_box(request, mi, orc):
    """(scene, spp, the device's lanes with K4, ones per lane); asserts the precondition: one pass, and lane i is sample i % spp of pixel i // spp"""
    spp = request.param
    assert 64 % spp == 0
    sc, osc = load(mi, orc, "cornell_wall.xml", dict(resx=SIDE, resy=SIDE), "box")
    assert ref.pass_layout(orc, osc, osc.params(), spp) == (spp, 1)
    n = SIDE * SIDE * spp
    lanes = sc.sample_lanes_variants(SEED, spp, 0, n, variants=K4)
    assert lanes["valid"].all() and lanes["rgb"].shape == (4, n, 3)
    pixel = np.arange(n) // spp
    off = lanes["sample_pos"].astype(np.float64) - np.stack([pixel % SIDE, pixel // SIDE], axis=1)
    assert (off >= 0).all() and (off <= 1).all(), "a pixel's spp lanes are not consecutive"
    return sc, spp, lanes, np.ones((n, 1), np.float32)


def test_float64_film_is_the_tree_of_its_lanes(wall_box):
    sc, spp, lanes, ones = wall_box
    _, films = sc.render_film64(SEED, spp, variants=K4)
    assert films.shape == (4, SIDE, SIDE, 4) and sc.last_stats["n_fused_splat_launches"] == 0
    for k in range(4):
        want = planes(np.concatenate([lanes["rgb"][k], ones], axis=1), spp)
        bad = same_bits(np.moveaxis(films[k], -1, 0), want)
        print("float64 film, %d spp, variant %d: %d of %d doubles differ from the tree" % (spp, k, bad, want.size))
        assert np.abs(want[:3]).max() > 0 and (want[3] == spp).all()
        assert bad == 0, (spp, k, bad)


def test_moment_film_is_the_tree_of_its_lanes(wall_box):
    sc, spp, lanes, _ = wall_box
    raw = moment_planes_of(sc.render_moments(SEED, spp, variants=K4[:2], raw=True))
    want = planes(ref.moment_values([lanes["rgb"][0], lanes["rgb"][1]]), spp)      # 1 + 12 + one pair plane
    assert want.shape == (ref.n_planes(2), SIDE, SIDE) == (14, SIDE, SIDE)
    bad = same_bits(raw, want)
    print("moment film, %d spp: %d of %d doubles differ from the tree" % (spp, bad, want.size))
    assert (want[0] == spp).all() and np.abs(want[13]).max() > 0
    assert bad == 0, (spp, bad)


def test_aov_film_is_the_tree_of_its_lanes(wall_box):
    sc, spp, _, ones = wall_box
    values = sc.sample_aov_lanes(SPEC6, SEED, spp, 0, SIDE * SIDE * spp)["values"]
    assert values.shape == (SIDE * SIDE * spp, 6)
    raw = aov_planes_of(sc.render_aovs(SPEC6, SEED, spp, raw=True), SPEC6)
    want = planes(np.concatenate([ones, values], axis=1), spp)
    bad = same_bits(raw, want)
    print("aov film, %d spp: %d of %d doubles differ from the tree" % (spp, bad, want.size))
    assert (want[0] == spp).all() and np.abs(want[1:]).max() > 0
    assert bad == 0, (spp, bad)
