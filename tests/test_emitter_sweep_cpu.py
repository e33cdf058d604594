"""The inputs of the emitter sweep (tests/emitter_sweep.py), judged by the oracle alone: that the array entry orc_kat_emitter_n is orc_kat_emitter_sample behind the
emitter pick, that family C lands ON the value of every compare of the emitter chain and on both sides of it, that the mesh light's faces and the mixed scene's
emitters are all picked, and that every query passes the validation rule of dtof_emitter_eval.  The device leg is test_emitter_sweep_gpu.py: it runs these very
queries through every level of the shade kernels a scene can run at."""
import ctypes as C

import numpy as np
import pytest

import emitter_sweep as es

F32 = np.float32


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    return es.write_fixtures(tmp_path_factory.mktemp("emitter_sweep"))


@pytest.fixture(scope="module")
def swept(orc, fixtures):
    """name -> (entry, oracle scene, {(mode, family, shape): queries}, {...: oracle outputs}, family C by deciding input); the last entry is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            e = {x.name: x for x in es.catalogue(fixtures)}[name]
            osc = orc.Scene(e.xml, {}, is_string=True)
            fam, c = es.families(e, orc, osc)
            cache[name] = (e, osc, fam, {k: es.oracle_eval(orc, osc, k[0], q, k[2]) for k, q in fam.items()}, c)
        return cache[name]
    return get


@pytest.mark.parametrize("name", es.NAMES)
def test_array_entry_is_the_scalar_entry_behind_the_pick(orc, swept, name):
    """orc_kat_emitter_n, mode 0, equals Scene::sample_emitter (scene.cpp:171-189) done in numpy float32 followed by orc_kat_emitter_sample, then ds.pdf *= pmf and
    weight *= ne, bit for bit: 2 000 queries of A, every 5th of B and every 20th of C"""
    e, osc, fam, out, _ = swept(name)
    L = orc.lib()
    ne = osc.c.n_emitters
    pmf = F32(1) / F32(ne)
    q = np.concatenate([fam[(0, "A", -1)][:2000], fam[(0, "B", -1)][::5]] + ([fam[(0, "C", -1)][::20]] if (0, "C", -1) in fam else []))
    got = es.oracle_eval(orc, osc, 0, q)[:, :14]
    want = np.zeros((len(q), 14), F32)
    o13 = np.zeros(13, F32)
    for i, (px, py, pz, e1, e2) in enumerate(q):
        idx, w, sx = 0, F32(1), e1
        if ne > 1:
            scaled = F32(e1 * F32(ne))
            idx = min(int(scaled), ne - 1)
            w, sx = F32(ne), F32(scaled - F32(idx))
        ref = np.array([px, py, pz], F32)
        L.orc_kat_emitter_sample(C.byref(osc.c), idx, ref.ctypes.data, float(sx), float(e2), o13.ctypes.data)
        with np.errstate(all="ignore"):
            pdf = F32(o13[4] * pmf)
            want[i] = np.concatenate([o13[9:12], o13[0:3], o13[3:4], [pdf], o13[5:6], (o13[6:9] * w).astype(F32), [F32(pdf != 0 and o13[12] != 0)], [F32(idx)]])
    assert es.same_bits(got, want).all(), es.describe_mismatch(name, 0, "A+B+C", q, got, want, "array entry vs scalar entry")


# every compare named by the emitter chain, and the entries whose families must reach it.  (below, on, above) must all be > 0, with these exceptions:
#  * no float32 squares to 0.00068523 (test_no_float_squares_to_the_sphere_switch proves it), so sin_theta_max_2 is never ON it;
#  * a textured light's density is set to 0 whenever the sample is not usable, so "a density but not usable" cannot occur there;
#  * dot(d, n) at the sampled point is EXACTLY 0 only where the arithmetic allows it: required of the lights in an axis-aligned plane (EXACT_GRAZING), where a
#    reference point shares the light's coordinate; under a general rotation the three products cancel by luck alone.  It matters for the textured lights only, where
#    `dp < 0` alone decides the sample: for the others dist2 / 0 is not finite, the density becomes 0 and `ds_pdf != 0` rejects the sample whatever `dp < 0` said;
#  * a flipped sphere's surface lies inside radius_adj = radius * (1 + eps): a coincident point never takes the outside branch there.
EXACT_GRAZING = ("rectangle_bitmap_axis_aligned", "disk")
GRAZING = ("rectangle", "rectangle_bitmap_bilinear_repeat", "rectangle_bitmap_nearest_mirror", "rectangle_checkerboard", "rectangle_bitmap_axis_aligned", "disk",
           "mesh_face_normals", "mixed")
def _required(e):
    names = []
    if e.name in ("two_points_and_a_spot", "mixed"):
        names.append("pick: e1 * ne against k")
    if e.kind in ("mesh", "mixed"):
        names.append("mesh: cdf[mid] < v")
    if e.kind.startswith("rect_bitmap"):
        names += ["texture: row search, cdf[mid] < v", "texture: column search, cdf[mid] < v"]
    if e.kind == "envmap":   # (the coarsest level of a map of 8 x 3 patches has ONE row of blocks: its r1 is 0, so sy * (r0 + r1) never exceeds r0 there)
        names += ["envmap: level %d, %s" % (lv, c) for lv in (1, 2) for c in ("sy > r0", "sx > c0")] + ["envmap: level 3, sx > c0"]
    if e.kind == "spot":
        names += ["spot: cos_theta >= cos_beam", "spot: cos_theta > cos_cutoff"]
    if e.kind in ("sphere", "mixed"):
        names += ["sphere: dc_2 > sqr(radius_adj)", "sphere: sin_theta_max_2 > 0.00068523", "hit side, shape %d: sin_alpha < 0.99999994" % (0 if e.kind == "sphere" else 1)]
    if e.kind == "sphere":
        names.append("sphere: reference at the centre, dist == 0")
    if e.name in GRAZING:
        names.append("area: dot(d, n) < 0 at the sampled point")
    if e.hit_shapes and e.kind != "sphere":
        names.append("area: ds_pdf != 0 and facing")
    names += ["hit side, shape %d: dp < 0" % s for s in e.hit_shapes]
    return names


@pytest.mark.parametrize("name", [x.name for x in es.catalogue() if _required(x)])
def test_families_sit_on_both_sides_of_every_compare_and_on_it(swept, name):
    e, osc, fam, out, _ = swept(name)
    counts = es.compares(e, fam, out)
    print(name, counts)
    for c in _required(e):
        below, on, above = counts[c]
        if c == "sphere: sin_theta_max_2 > 0.00068523":
            assert below > 0 and above > 0 and on == 0, (name, c, counts[c])
        elif c == "area: ds_pdf != 0 and facing" and e.textured:
            assert on > 0 and above > 0, (name, c, counts[c])
        elif c == "area: dot(d, n) < 0 at the sampled point" and name not in EXACT_GRAZING:
            assert below > 0 and above > 0, (name, c, counts[c])
        elif c == "sphere: reference at the centre, dist == 0":
            assert below > 0 and above > 0 and (on > 0 or name == "sphere_flipped"), (name, c, counts[c])
        else:
            assert below > 0 and on > 0 and above > 0, (name, c, counts[c])


def test_no_float_squares_to_the_sphere_switch():
    """sin_theta_max_2 = sqr(sin_theta_max): around sqrt(0.00068523) consecutive floats square to values 1.7 float32 steps apart, and none of them to the constant"""
    c = es.STM2_SWITCH
    x = F32(np.sqrt(np.float64(c)))
    xs = np.array([x], F32)
    for _ in range(64):
        xs = np.concatenate([np.nextafter(xs[:1], F32(0)), xs, np.nextafter(xs[-1:], F32(1))])
    sq = (xs * xs).astype(F32)
    assert sq[0] < c < sq[-1] and not (sq == c).any()


@pytest.mark.parametrize("name", ["mesh_face_normals", "mesh_vertex_normals", "mixed"])
def test_every_face_with_area_is_picked_and_no_other(swept, name):
    e, osc, fam, out, _ = swept(name)
    o0 = np.concatenate([out[k] for k in sorted(fam) if k[0] == 0])
    faces = o0[:, es.FACE]
    assert set(faces[~np.isnan(faces)].astype(int)) == {k for k, a in enumerate(es.MESH_AREAS) if a > 0}


def test_every_emitter_of_the_mixed_scene_is_picked(swept):
    e, osc, fam, out, _ = swept("mixed")
    for k in sorted(fam):
        if k[0] == 0:
            assert set(out[k][:, es.INDEX].astype(int)) == {0, 1, 2, 3}, k


@pytest.mark.parametrize("name", es.NAMES)
def test_every_query_passes_the_validation_rule_and_nan_rows_stay_few(swept, name):
    """finite floats and draws in [0, 1) only (dtof_emitter_eval refuses anything else); and, since two NaNs compare equal in test_emitter_sweep_gpu.py, rows with a
    NaN stay below 5 % of family A and below half of every edge family (B puts a third of its reference points ON a point light, where the direction is 0 / 0)"""
    e, osc, fam, out, _ = swept(name)
    for k, q in fam.items():
        assert es.valid(k[0], q), k
        assert len(q) > 0 and q.shape[1] == es.N_IN[k[0]]
        assert np.isnan(out[k][:, :es.N_OUT[k[0]]]).any(axis=1).mean() < (0.05 if k[1] == "A" else 0.5), k
    assert len(fam[(0, "A", -1)]) == es.N_A


def test_catalogue_levels_are_what_the_entry_accepts():
    """the catalogue's own bookkeeping: a scene with an area light is never listed for a level without AREA, a scene with SPEC-only features for none below 4, and
    the level scene_traits() implies is among the eligible ones"""
    for e in es.catalogue():
        assert e.traits_level in e.levels, e.name
        if e.hit_shapes:
            assert not set(e.levels) & {0, 2, 6}, e.name
        if e.env or e.textured or e.kind in ("spot", "directional"):
            assert min(e.levels) >= 4, e.name
