"""The tree sweep's conditions, shown on the oracle alone (no device): that the rays of tests/tree_sweep.py are what test_tree_sweep_gpu.py needs them to be -- the
boundary families hit, the ties exist, the deep scene is deep, the non-finite family misses -- and what can be held of dtof_tree_query without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tree_sweep as ts
from conftest import ROOT

INVALID = 1


@pytest.fixture(scope="module")
def swept(orc, tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ts.Sweep(name, orc, tmp_path_factory.mktemp(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", ts.NAMES)
def test_boundary_families_hit_and_the_extreme_family_misses(swept, name):
    sw = swept(name)
    hit = sw.want["ids"][:, 0] >= 0
    assert sw.n == len(sw.rays) == len(sw.family) and (sw.n <= 4000 if name == "deep" else 10000 <= sw.n <= 60000), sw.n
    for fam in ("B", "F", "E"):
        sel = sw.family == fam
        print("%s, family %s: %d rays, the oracle hits %d" % (name, fam, sel.sum(), hit[sel].sum()))
        assert sel.sum() > 0 and 2 * hit[sel].sum() >= sel.sum(), (name, fam, int(sel.sum()), int(hit[sel].sum()))
    # B sits ON the rim: of its rays, issued a few floats either side of the last one that hits a mesh, some miss that mesh
    b = sw.family == "B"
    assert 0 < hit[b].sum() < b.sum() or name == "deep"
    h = sw.family == "H"
    assert h.sum() > 50 and hit[h].sum() == 0 and sw.want["occluded"][h].sum() == 0, (name, int(hit[h].sum()))
    assert sw.inf_direction_rays[1] > 0 or name not in ("slab_small", "slab_unit"), sw.inf_direction_rays      # (the flat slabs: every infinite direction is a miss)
    m = sw.family == "M"
    assert hit[m].sum() == 0 and sw.want["occluded"][m].sum() == 0
    # C: t == maxt is a miss, a float above it is the hit again
    c = np.flatnonzero(sw.family == "C")
    third = len(c) // 3
    below, at, above = c[:third], c[third:2 * third], c[2 * third:]
    assert (sw.want["tuv"][above, 0] == sw.rays[at, 7]).mean() > 0.95 and (sw.want["tuv"][at, 0] != sw.rays[at, 7]).all()
    # every family is there, each ray serves both kinds, the short lists hold one hit each
    fams = set(np.unique(sw.family))
    assert {"A", "B", "F", "E", "C", "C2", "H", "M"} <= fams and (("G" in fams) == bool(sw.geo.moving())) and (("T" in fams) == (name == "ties"))
    assert sorted(len(v) for v in sw.short.values())[0] == 1 and {len(v) for v in sw.short.values()} == {1, 63, 64, 65}
    for rows in sw.short.values():
        assert (sw.want["ids"][rows, 0] >= 0).sum() == 1
    assert np.array_equal(np.sort(sw.perm), np.arange(sw.n))


def test_ties_exist_across_objects_shapes_and_faces(swept):
    sw = swept("ties")
    across_objects, across_shapes, across_faces = ts.tie_classes(sw, sw.rays[np.isin(sw.family, ["T", "F"])])
    print("ties: %d across objects, %d across shapes, %d across faces" % (across_objects, across_shapes, across_faces))
    assert across_objects > 0 and across_shapes > 0 and across_faces > 0


def test_instance_rays_hit_at_one_shutter_end_only(swept):
    sw = swept("blobs")
    g = sw.of("G")
    res = sw.osc.tree_n(g)["ids"][:, 0] >= 0
    one_end = sum(bool(res[i]) != bool(res[i + 2]) for i in range(1, len(g), 4))
    print("blobs, family G: %d of %d finite-maxt pairs hit at one shutter end only" % (one_end, len(g) // 4))
    assert one_end > len(g) // 16


def test_deep_scene_exceeds_the_lds_stack(mi, swept):
    sw = swept("deep")
    depth = mi.load_file(sw.path, resx=16, resy=16).info()["bvh_stack_depth"]
    print("deep: bvh_stack_depth %d" % depth)
    assert ts.LDS_STACK8 < depth <= 64
    hdr = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "dtof_kernels.h")).read()
    assert int(re.search(r"kLdsStack8\s*=\s*(\d+)", hdr).group(1)) == ts.LDS_STACK8


def test_oracle_array_entry_is_the_per_ray_entry(orc, swept):
    sw = swept("blobs")
    rows = np.random.default_rng(5).choice(sw.n, 600, replace=False)
    L = orc.lib()
    for i in rows:
        o, d = np.ascontiguousarray(sw.rays[i, 0:3]), np.ascontiguousarray(sw.rays[i, 3:6])
        hit3, ids3 = np.zeros(3, np.float32), np.zeros(3, np.int32)
        fp = C.POINTER(C.c_float)
        L.orc_intersect(C.byref(sw.osc.c), o.ctypes.data_as(fp), d.ctypes.data_as(fp), C.c_float(sw.rays[i, 6]), C.c_float(sw.rays[i, 7]), hit3.ctypes.data_as(fp),
                        ids3.ctypes.data_as(C.POINTER(C.c_int32)))
        assert np.array_equal(hit3.view(np.uint32), sw.want["tuv"][i].view(np.uint32)) and np.array_equal(ids3, sw.want["ids"][i]), i


# ---------------------------------------------------------------------------- dtof_tree_query without a device
def test_tree_query_is_declared_and_exported(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    decl = re.search(r"\bint\s+dtof_tree_query\s*\(([^;]*)\)\s*;", hdr)
    assert decl and [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == ["scene", "form", "any", "n", "rays8", "out3", "ids3"]
    assert hasattr(C.CDLL(mi.lib_path()), "dtof_tree_query")
    assert mi.Scene.TREE_FORMS == {n: i for i, n in enumerate(ts.FORM_NAMES)}


def test_refusals_come_before_any_device_work(mi, tmp_path):
    """forms a scene does not meet, a bad form, too many rays and null arguments are refused with DTOF_ERR_INVALID and the outputs keep their canaries -- here, where
    there is no device to launch on, which also shows that the refusal precedes the launch"""
    rays = ts.rays8([[0, 1, 3]] * 4, [[0, 0, -1]] * 4, 0.0, np.inf)
    boxes = mi.load_file(os.path.join(ROOT, "scenes", "cornell_boxes.xml"), resx=16, resy=16)      # cubes of 12 triangles: no BLAS, no half-float nodes
    mixed = mi.load_file(ts.build("mixed", tmp_path), resx=16, resy=16)
    cases = [(boxes, 1, "no half-float nodes"), (boxes, 2, "no half-float nodes"), (boxes, 3, "no half-float nodes"), (boxes, 4, "no half-float nodes"),
             (mixed, 1, "analytic shape"), (mixed, 2, "analytic shape"), (mixed, 3, "analytic shape"), (mixed, -1, "form must be"), (mixed, 5, "form must be")]
    for sc, form, reason in cases:
        for any_hit in (0, 1):
            rc, out, ids = ts.device_query(mi, sc, form, any_hit, rays)
            msg = mi._lib().dtof_last_error().decode()
            assert rc == INVALID and reason in msg and msg.startswith("dtof_tree_query"), (form, any_hit, rc, msg)
            assert (ids.view(np.uint32) == ts.CANARY).all() and (out is None or (out == ts.CANARY).all())
    big = np.zeros(((1 << 24) + 1, 8), np.float32)
    rc, out, ids = ts.device_query(mi, mixed, 0, 1, big[:4], n=(1 << 24) + 1)
    assert rc == INVALID and "2^24" in mi._lib().dtof_last_error().decode() and (ids.view(np.uint32) == ts.CANARY).all()
    L = mi._lib()
    word = np.zeros(16, np.int32)
    assert L.dtof_tree_query(mixed._h, 0, 0, 4, None, word.ctypes.data, word.ctypes.data) == INVALID
    assert L.dtof_tree_query(mixed._h, 0, 0, 4, rays.ctypes.data, None, word.ctypes.data) == INVALID
    assert L.dtof_tree_query(mixed._h, 0, 1, 4, rays.ctypes.data, None, None) == INVALID
    assert L.dtof_tree_query(None, 0, 1, 4, rays.ctypes.data, None, word.ctypes.data) == INVALID
    with pytest.raises(mi.DtofError, match="analytic shape"):
        mixed.tree_query(rays, "defer_pair")
