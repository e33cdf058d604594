"""The fused sweep's conditions, shown on the oracle alone (no device): that the rays of tests/fused_sweep.py are what test_fused_sweep_gpu.py needs them to be -- every
decision of the analytic shapes' ray tests is met on both sides, the sphere's two query kinds disagree near tangency, every analytic tie exists, no oracle hit on an
analytic shape is an artefact, the extreme family misses -- and what can be held of dtof_fused_query without a device: the forms each scene meets, and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fused_sweep as fz
from conftest import ROOT

OK, INVALID, HIP = 0, 1, 2


@pytest.fixture(scope="module")
def swept(orc, tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fz.Sweep(name, orc, tmp_path_factory.mktemp(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", fz.NAMES)
def test_families_are_there_and_the_extreme_family_misses(swept, name):
    sw = swept(name)
    hit = sw.want["ids"][:, 0] >= 0
    assert sw.n == len(sw.rays) == len(sw.family) and (2000 <= sw.n <= 6000 if name == "domino_half" else 10000 <= sw.n <= 60000), sw.n
    fams = set(np.unique(sw.family))
    want = {"A", "G", "M", "C", "H"} | ({"S", "Y", "K", "T"} if name.startswith("analytic") else set())
    assert fams == want, fams
    for fam in sorted(fams):
        sel = sw.family == fam
        print("%s, family %s: %d rays, the oracle hits %d, occludes %d" % (name, fam, sel.sum(), hit[sel].sum(), sw.want["occluded"][sel].sum()))
    for fam in ("H", "M"):
        sel = sw.family == fam
        assert sel.sum() > 50 and hit[sel].sum() == 0 and sw.want["occluded"][sel].sum() == 0, (name, fam)
    print("%s, family H: %d of %d candidates are misses of the oracle and were kept" % (name, sw.extreme_rays[1], sw.extreme_rays[0]))
    # C: t == maxt is a miss, a float above it is the hit again
    c = np.flatnonzero(sw.family == "C")
    third = len(c) // 3
    at, above = c[third:2 * third], c[2 * third:]
    assert (sw.want["tuv"][above, 0] == sw.rays[at, 7]).mean() > 0.95 and (sw.want["tuv"][at, 0] != sw.rays[at, 7]).all()
    # G: the moving shapes are hit at one shutter end only by some of the rays whose maxt lies between the two distances
    g = np.flatnonzero(sw.family == "G")
    finite = g[np.isfinite(sw.rays[g, 7])].reshape(-1, 3)      # times 0, T, T / 2 of one ray
    one_end = int((hit[finite[:, 0]] != hit[finite[:, 1]]).sum())
    print("%s, family G: %d of %d finite-maxt rays hit at one shutter end only" % (name, one_end, len(finite)))
    assert one_end > 0
    # every direction is normalised in float32, every origin lies within 1e4 extents (family H aside)
    plain = sw.family != "H"
    d = sw.rays[plain, 3:6].astype(np.float64)
    zero_comp = (sw.family[plain] == "K") & (np.abs(np.linalg.norm(d, axis=1) - 1) > 1e-6)      # (K's in-plane rays have one component set to +-0 afterwards)
    assert (np.abs(np.linalg.norm(d, axis=1) - 1) < 1e-6)[~zero_comp].all() and zero_comp.sum() <= 64
    assert np.abs(sw.rays[plain, 0:3]).max() <= 1e4 * max(sw.extent, 1.0) * 1.01 + 200.0
    # the placements
    sizes = {len(v) for v in sw.short.values()}
    resident = any(f >= 2 for f, _ in sw.forms)
    assert sizes == {1, 63, 64, 65} | ({w * 64 + e for w in fz.WAVES for e in (-1, 0, 1)} if resident else set())
    for rows in sw.short.values():
        assert (sw.want["ids"][rows, 0] >= 0).sum() == 1 and (sw.want["occluded"][rows] == 1).sum() == 1
    assert np.array_equal(np.sort(sw.perm), np.arange(sw.n))


@pytest.mark.parametrize("name", ["analytic_field", "analytic_small"])
def test_every_decision_of_the_analytic_tests_is_met_on_both_sides(swept, name):
    sw = swept(name)
    for label, (ok, dropped) in sorted(sw.bisected.items()):
        print("%s, bisected on the oracle: %-32s %4d thresholds (%d pairs dropped: an end did not behave)" % (name, label, ok, dropped))
        assert ok > 0, label
    want = {"S tangent", "S maxt", "S behind"}
    assert {l.split(",")[0] for l in sw.bisected if l.endswith("occlusion")} == want == {l.split(",")[0] for l in sw.bisected if l.endswith("closest")}
    assert {"Y tangent", "Y end z == 0", "Y end z == 1", "Y inside through the end", "Y maxt", "K rim", "K t == 0", "K maxt"} <= set(sw.bisected)
    dec = fz.decisions(sw)
    for label, (yes, no) in dec.items():
        print("%s, %-56s true for %5d rays, false for %5d" % (name, label, yes, no))
    need = ["S discrim >= 0", "S near_t <= maxt", "S far_t >= 0", "S in_bounds", "S near_t < 0 (the far root answers)", "S plane_t == 0",
            "S plane_t == 0 and no coordinate equals the centre's", "Y A == 0", "Y A == 0: C != 0 (the linear branch, b == 0: -c / 0)", "Y discrim >= 0", "Y near_t <= maxt", "Y far_t >= 0", "Y in_bounds",
            "Y z_near >= 0", "Y z_near <= 1", "Y z_far >= 0", "Y z_far <= 1", "Y near_ok", "Y !near_ok && far_ok", "K ld.z == 0", "K t >= 0", "K t <= maxt",
            "K u * u + v * v <= 1"]
    for label in need:
        assert label in dec and dec[label][0] > 0 and dec[label][1] > 0, (label, dec.get(label))
    wall = dec["Y A == 0: C == 0 (on the wall: 0 / 0)"]      # (its other side is the linear branch, asserted above)
    assert wall[0] > 0, wall
    # the families hit and miss the shape they were built around: the thresholds lie between rays, not beside them
    hit = sw.want["ids"][:, 0] >= 0
    for fam in ("S", "Y", "K"):
        sel = sw.family == fam
        assert 0 < hit[sel].sum() < sel.sum()


@pytest.mark.parametrize("name", ["analytic_field", "analytic_small"])
def test_the_spheres_two_query_kinds_disagree_near_tangency(swept, name):
    sw = swept(name)
    s = sw.family == "S"
    differ = (sw.want["ids"][s, 0] >= 0) != (sw.want["occluded"][s] == 1)
    print("%s: the oracle's closest-hit and occlusion queries disagree on %d of %d rays of family S" % (name, differ.sum(), s.sum()))
    assert differ.sum() > 0


@pytest.mark.parametrize("name", ["analytic_field", "analytic_small"])
def test_every_analytic_tie_class_is_there(swept, name):
    counts = swept(name).tie_classes()
    print("%s, ties at equal float t: %s" % (name, ", ".join("%s %d" % kv for kv in counts.items())))
    assert all(v > 0 for v in counts.values()), counts


@pytest.mark.parametrize("name", ["analytic_field", "analytic_small"])
def test_no_oracle_hit_on_an_analytic_shape_is_an_artefact(swept, name):
    sw = swept(name)
    bad = fz.artefacts(sw)
    on_analytic = sum(sw.prims[sw.by_id[(int(o), int(s))]].kind in (fz.SPHERE, fz.DISK, fz.CYLINDER) for o, s in sw.want["ids"][sw.want["ids"][:, 0] >= 0, 0:2])
    print("%s: %d oracle hits on analytic shapes, %d of them on a shape the float64 ray does not come within the padding of" % (name, on_analytic, len(bad)))
    assert on_analytic > 1000 and len(bad) == 0, [(sw.family[i], sw.rays[i].tolist(), sw.want["ids"][i].tolist()) for i in bad[:5]]


# ---------------------------------------------------------------------------- dtof_fused_query without a device
def test_fused_query_is_declared_and_exported(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    decl = re.search(r"\bint\s+dtof_fused_query\s*\(([^;]*)\)\s*;", hdr)
    assert decl and [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == ["scene", "form", "waves", "any", "n", "rays8", "out3", "ids3"]
    assert hasattr(C.CDLL(mi.lib_path()), "dtof_fused_query")
    assert mi.Scene.FUSED_FORMS == {n: i for i, n in enumerate(fz.FORM_NAMES)}
    abi = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "_abi.py")).read()
    assert '"dtof_fused_query"' in abi
    mk = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "Makefile")).read()
    assert re.search(r"KERNEL_SRCS :=.*\bdtof_fused_query\b", mk)


@pytest.mark.parametrize("name", fz.NAMES)
def test_each_scene_meets_exactly_its_forms(mi, tmp_path, monkeypatch, name):
    """every (form, waves) against the table of fused_sweep.SCENE_FORMS, under the LDS limit of the device the table is written for.  A call of no rays is refused
    (DTOF_ERR_INVALID) or not: a scene that stops qualifying for a form fails here instead of being refused everywhere on the device."""
    monkeypatch.setenv("DTOF_LDS_LIMIT", str(fz.LDS_LIMIT))
    scene = mi.load_file(fz.build(name, tmp_path), resx=16, resy=16)
    i = scene.info()
    print("%s: %d objects, %d shapes, %d nodes, stack depth %d, blob %d bytes" % (name, i["n_objects"], i["n_shapes"], i["n_bvh_nodes"], i["bvh_stack_depth"], i["scene_blob_bytes"]))
    assert (i["scene_blob_bytes"] <= 16 * 1024) == (name in ("analytic_small", "rects_tree"))
    if name == "domino_half":
        assert 1024 < i["n_bvh_nodes"] <= 2048
    if name == "analytic_field":
        assert i["n_shapes"] - 4 - 9 >= 40      # static analytic shapes: all but the group's four and the nine rectangles
    met = set()
    word = np.zeros(4, np.int32)
    for form in range(len(fz.FORM_NAMES)):
        for waves in ((0,) if form < 2 else fz.WAVES):
            for any_hit in (0, 1):
                rc = mi._lib().dtof_fused_query(scene._h, form, waves, any_hit, 0, None, None, word.ctypes.data)
                msg = mi._lib().dtof_last_error().decode()
                assert rc in (OK, HIP) or (rc == INVALID and msg.startswith("dtof_fused_query:")), (form, waves, rc, msg)
                if rc != INVALID:
                    met.add((form, waves))
                else:
                    print("%s, %s at %d waves: %s" % (name, fz.FORM_NAMES[form], waves, msg))
    assert met == set(dict(fz.SCENE_FORMS)[name]), sorted(met)


def test_refusals_come_before_any_device_work(mi, tmp_path, monkeypatch):
    """forms a scene does not meet, a bad form, bad wave counts, too many rays and null arguments are refused with DTOF_ERR_INVALID, a message that begins
    "dtof_fused_query:" and the outputs' canaries untouched -- here, where there is no device to launch on, which also shows that the refusal precedes the launch"""
    monkeypatch.setenv("DTOF_LDS_LIMIT", str(fz.LDS_LIMIT))
    rays = fz.ts.rays8([[0, 1, 3]] * 4, [[0, 0, -1]] * 4, 0.0, np.inf)
    field = mi.load_file(fz.build("analytic_field", tmp_path), resx=16, resy=16)
    small = mi.load_file(fz.build("analytic_small", tmp_path), resx=16, resy=16)
    half = mi.load_file(fz.build("domino_half", tmp_path), resx=16, resy=16)
    boxes = mi.load_file(os.path.join(ROOT, "scenes", "cornell_boxes.xml"), resx=16, resy=16)
    cases = [(field, 1, 0, "rectangle code only"), (field, 4, 8, "half-float planes"), (field, 5, 16, "half-float planes"), (field, 2, 16, "bytes of LDS"),
             (field, 2, 10, "waves must be"), (field, 3, 0, "waves must be"), (field, 2, 64, "waves must be"), (field, -1, 8, "form must be"), (field, 6, 8, "form must be"),
             (small, 2, 8, "no resident layout"), (small, 3, 12, "no resident layout"), (boxes, 2, 8, "no resident layout"),
             (half, 2, 8, "more than 1024 nodes"), (half, 3, 16, "more than 1024 nodes"), (half, 1, 0, "rectangle code only")]
    for sc, form, waves, reason in cases:
        for any_hit in (0, 1):
            rc, out, ids = fz.device_query(mi, sc, form, waves, any_hit, rays)
            msg = mi._lib().dtof_last_error().decode()
            assert rc == INVALID and reason in msg and msg.startswith("dtof_fused_query:"), (form, waves, any_hit, rc, msg)
            assert (ids.view(np.uint32) == fz.CANARY).all() and (out is None or (out == fz.CANARY).all())
    # a smaller LDS budget refuses what fitted
    monkeypatch.setenv("DTOF_LDS_LIMIT", str(64 * 1024))
    rc, out, ids = fz.device_query(mi, field, 2, 8, 0, rays)
    assert rc == INVALID and "bytes of LDS" in mi._lib().dtof_last_error().decode() and (ids.view(np.uint32) == fz.CANARY).all() and (out == fz.CANARY).all()
    monkeypatch.setenv("DTOF_LDS_LIMIT", str(fz.LDS_LIMIT))
    rc, out, ids = fz.device_query(mi, field, 0, 0, 1, rays, n=(1 << 24) + 1)
    assert rc == INVALID and "2^24" in mi._lib().dtof_last_error().decode() and (ids.view(np.uint32) == fz.CANARY).all()
    L = mi._lib()
    word = np.zeros(16, np.int32)
    for args in ((field._h, 0, 0, 0, 4, None, word.ctypes.data, word.ctypes.data), (field._h, 0, 0, 0, 4, rays.ctypes.data, None, word.ctypes.data),
                 (field._h, 0, 0, 1, 4, rays.ctypes.data, None, None), (None, 0, 0, 1, 4, rays.ctypes.data, None, word.ctypes.data)):
        assert L.dtof_fused_query(*args) == INVALID and L.dtof_last_error().decode().startswith("dtof_fused_query: null argument")
    with pytest.raises(mi.DtofError, match="rectangle code only"):
        field.fused_query(rays, "classic_rect")
    with pytest.raises(mi.DtofError, match="waves must be"):
        field.fused_query(rays, "resident", waves=4)
