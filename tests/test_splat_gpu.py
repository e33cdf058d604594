"""The raw float32 films of the hand-written splat kernels -- k_splat_x8, k_splat_pixel, k_splat_tent3, k_splat_generic (csrc/dtof_kernels.hip) and the splat fused into
k_shade -- held per pixel and channel to the exact sums of the oracle's lanes (tests/splat_ref.py):

    |device - E| <= (n + 2) * 2^-24 * M,   and exactly 0 where no term lands            (derived in splat_ref's docstring, not measured)

Every case of tests/splat_cases.py renders through render_rows into one zeroed allocation with margins (test_device_film.Film: a write outside the rows the call may
reach cannot hide), asserts that Scene.last_splat names the kernel and shape the case is there for, asserts that the device's lanes equal the oracle's BIT FOR BIT --
so a difference of the films belongs to the splat -- and prints the largest error / bound per plane before it asserts.  tests/test_splat_cpu.py shows on the CPU that
the criterion sees a lane lost, doubled, misplaced, shifted or with its channels swapped on these very cases."""
import numpy as np
import pytest

import adaptive_ref as aref
import moments_ref as ref
import splat_cases as cases
import splat_ref as sref
from test_device_film import Film, reach

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(mi, orc, name, monkeypatch):
    """render the case, hold it, return the ratios (planes, 4)"""
    c = cases.CASES[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    xml, params = cases.scene_xml(c)
    spp, variants, alpha = c["spp"], cases.variants(c), c["rgba"]
    sc, osc = mi.load_string(xml, **params), orc.Scene(xml, params, is_string=True)
    W, H = sc.size
    assert (W, H) == osc.size == tuple(cases.FRAMES[c["frame"]][1][2:] if cases.FRAMES[c["frame"]][1] else (params["resx"], params["resy"]))
    lanes = aref.Lanes(orc, osc, cases.SEED, spp, variants)
    # the device's lanes are the oracle's, bit for bit, film for film
    got = sc.sample_lanes_variants(cases.SEED, spp, 0, W * H * spp, variants)
    assert np.array_equal(bits(got["sample_pos"]), bits(lanes.lanes[0]["sample_pos"])), (name, "sample_pos")
    for k in range(lanes.K):
        assert np.array_equal(bits(got["rgb"][k]), bits(lanes.lanes[k]["rgb"])), (name, "rgb", k)
    if alpha:
        assert np.array_equal(np.asarray(got["valid"]) != 0, np.asarray(lanes.lanes[0]["valid"]) != 0), (name, "valid")
    E, M, n = sref.film(sref.LaneSet.of(lanes, alpha=alpha, rows=c["rows"]))
    planes, dense = lanes.K + alpha, H * W * 4
    halo = sc.info()["filter_halo"]
    r0, r1 = c["rows"] or (0, H)
    sc.set_film_layout(planes if (alpha or planes > 1) else 0)
    f = Film(planes, dense, W, H, 2 * dense)
    st = sc.render_rows(f.ptr, cases.SEED, spp, r0, r1, variants=variants)
    assert st["n_paths"] == (r1 - r0) * W * spp, (name, st["n_paths"])
    assert sc.last_splat == c["want"], (name, sc.last_splat, c["want"])
    assert st["n_fused_splat_launches"] == (1 if c["want"]["kernel"] == "fused" else 0), (name, st["n_fused_splat_launches"])
    hb = f.host()
    f.check_guard(hb, reach(range(r0, r1), halo, H), name)      # the margins and, for a band, the rows beyond its halo: exactly 0
    dev = np.stack([f.plane(hb, p) for p in range(planes)])
    assert np.abs(E[..., :3]).max() > 0 and (M[:lanes.K, r0:r1, :, 3] > 0).all(), name
    ratios = sref.errors_over_bound(dev, E, M, n)
    print("%s: %s, %d lanes, at most %d terms a pixel; largest error / bound per plane (r g b w): %s"
          % (name, sc.last_splat, (r1 - r0) * W * spp, n.max(), "; ".join(" ".join("%.3g" % v for v in row) for row in ratios)))
    assert (ratios <= 1.0).all(), (name, ratios)
    return ratios


@pytest.mark.parametrize("name", list(cases.CASES))
def test_raw_film_within_the_bound_of_the_lanes_exact_sums(mi, orc, name, monkeypatch):
    run(mi, orc, name, monkeypatch)
