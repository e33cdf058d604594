"""The TLAS / BLAS ray query against the brute-force oracle on dense and boundary rays: every scene of tests/tree_sweep.py through every form of dtof_tree_query the scene
meets -- the instantiations of trace_scene / trace_deferred the ray kernels of a frame carry: float nodes, half-float nodes with the overflow stack, the TLAS copy in LDS,
the DEFER pair, half-float nodes with every shape's code -- as closest-hit and as occlusion query, against orc_kat_tree_n (scene_closest / scene_occluded) on the same
rays.  Every output word equal as a bit pattern -- t, u, v, object, shape, primitive, the occlusion flag -- with no tolerance and no ray left out.  The three placements
of a ray agree: in family order, under a fixed permutation, and as the one hit among certain misses in lists of 1, 63, 64 and 65 rays.  test_tree_sweep_cpu.py shows on
the oracle alone that the rays are what this needs; test_box_cull.py holds the slab test itself to its contract on the host."""
import os
import time

import numpy as np
import pytest

import tree_sweep as ts
from conftest import SCENES

pytestmark = pytest.mark.gpu
INVALID, HIP = 1, 2
_ended_abnormally = []      # a call that reported a HIP error: nothing more is launched by this module


@pytest.fixture(scope="module")
def swept(mi, orc, tmp_path_factory):
    """name -> (sweep, device scene, {(form, any): answer for the rays in family order}); the last scene is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            t0 = time.time()
            sw = ts.Sweep(name, orc, tmp_path_factory.mktemp(name))
            print("%s: %d rays, generated and answered by the oracle in %.2f s" % (name, sw.n, time.time() - t0))
            cache[name] = (sw, mi.load_file(sw.path, resx=16, resy=16), {})
        return cache[name]
    return get


def _query(mi, scene, form, any_hit, rays, what):
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    rc, out, ids = ts.device_query(mi, scene, form, any_hit, rays)
    if rc != 0:
        msg = "%s: return code %d, %s" % (what, rc, mi._lib().dtof_last_error().decode("utf-8", "replace"))
        if rc == HIP:
            _ended_abnormally.append(msg)
        pytest.fail(msg)
    never = int((ids.view(np.uint32) == ts.CANARY).sum()) + (0 if any_hit else int((out == ts.CANARY).sum()))
    assert never == 0, "%s: %d output words were never written" % (what, never)
    return out, ids


def _in_order(mi, entry, form, any_hit):
    sw, scene, got = entry
    if (form, any_hit) not in got:
        got[(form, any_hit)] = _query(mi, scene, form, any_hit, sw.rays, "%s, %s, %s, in family order" % (sw.name, ts.FORM_NAMES[form], ts.KINDS[any_hit]))
    return got[(form, any_hit)]


@pytest.mark.parametrize("name,form,kind", ts.CASES, ids=["%s-%s-%s" % (n, ts.FORM_NAMES[f], k) for n, f, k in ts.CASES])
def test_device_tree_query_equals_the_oracle(mi, swept, name, form, kind):
    entry = swept(name)
    sw, scene, _ = entry
    any_hit = ts.KINDS.index(kind)
    what = "%s, %s, %s" % (name, ts.FORM_NAMES[form], kind)
    t0 = time.time()
    got = _in_order(mi, entry, form, any_hit)
    want = ts.want_words(sw, any_hit)
    rows = ts.differing(got, want)
    print("%s: %d rays in family order, %d differ from the oracle" % (what, sw.n, len(rows)))
    assert len(rows) == 0, ts.describe(sw, rows, lambda i: ts.show(got, i), lambda i: ts.show(want, i), what + " (first) against the oracle (second)")
    # the same rays under the fixed permutation: mixed waves
    mixed = _query(mi, scene, form, any_hit, sw.rays[sw.perm], what + ", permuted")
    back = (None if any_hit else np.empty_like(mixed[0]), np.empty_like(mixed[1]))
    back[1][sw.perm] = mixed[1]
    if not any_hit:
        back[0][sw.perm] = mixed[0]
    rows = ts.differing(back, got)
    assert len(rows) == 0, ts.describe(sw, rows, lambda i: ts.show(back, i), lambda i: ts.show(got, i), what + ": permuted (first) against in order (second)")
    # one ray that hits among certain misses, in lists of 1, 63, 64 and 65
    for label, idx in sw.short.items():
        short = _query(mi, scene, form, any_hit, sw.rays[idx], what + ", " + label)
        ref = (None if any_hit else got[0][idx], got[1][idx])
        rows = ts.differing(short, ref)
        assert len(rows) == 0, "%s, %s: rays %s of the list differ from their answers in family order" % (what, label, rows.tolist())
    print("%s: in order, permuted, %d short lists: %.2f s" % (what, len(sw.short), time.time() - t0))


@pytest.mark.parametrize("name", ts.NAMES)
def test_form_0_is_the_ray_query_of_dtof_ray_intersect(mi, swept, name):
    entry = swept(name)
    sw, scene, _ = entry
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    words, ids = _in_order(mi, entry, 0, 0)
    r = scene.ray_intersect(sw.rays[:, 0:3], sw.rays[:, 3:6], sw.rays[:, 6], sw.rays[:, 7])
    assert np.array_equal(np.ascontiguousarray(r["t"], np.float32).view(np.uint32), words[:, 0]) and np.array_equal(np.asarray(r["ids"], np.int32), ids)
    assert np.array_equal(np.asarray(scene.ray_test(sw.rays[:, 0:3], sw.rays[:, 3:6], sw.rays[:, 6], sw.rays[:, 7])).astype(np.int32), _in_order(mi, entry, 0, 1)[1])
    # ... and the Python entry is the same call
    q = scene.tree_query(sw.rays[:3000], "float")
    assert np.array_equal(np.stack([q["t"], q["u"], q["v"]], 1).view(np.uint32), words[:3000]) and np.array_equal(q["ids"], ids[:3000])
    assert np.array_equal(scene.tree_query(sw.rays[:3000], 0, any=True), _in_order(mi, entry, 0, 1)[1][:3000])
    assert len(scene.tree_query(sw.rays[:0])["t"]) == 0


def test_refusals_write_nothing_and_the_next_call_works(mi, tmp_path):
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    rays = ts.rays8([[0, 1, 3]] * 64, [[0, 0, -1]] * 64, 0.0, np.inf)
    boxes = mi.load_file(os.path.join(SCENES, "cornell_boxes.xml"), resx=16, resy=16)
    mixed = mi.load_file(ts.build("mixed", tmp_path), resx=16, resy=16)
    cases = [(boxes, f, "no half-float nodes") for f in (1, 2, 3, 4)] + [(mixed, f, "analytic shape") for f in (1, 2, 3)] + [(mixed, -1, "form must be"), (mixed, 5, "form must be")]
    for sc, form, reason in cases:
        for any_hit in (0, 1):
            rc, out, ids = ts.device_query(mi, sc, form, any_hit, rays)
            msg = mi._lib().dtof_last_error().decode()
            assert rc == INVALID and reason in msg, (form, any_hit, rc, msg)
            assert (ids.view(np.uint32) == ts.CANARY).all() and (out is None or (out == ts.CANARY).all())
    rc, out, ids = ts.device_query(mi, mixed, 0, 0, rays, n=(1 << 24) + 1)
    assert rc == INVALID and "2^24" in mi._lib().dtof_last_error().decode() and (ids.view(np.uint32) == ts.CANARY).all() and (out == ts.CANARY).all()
    first = {}
    for sc, forms in ((boxes, (0,)), (mixed, (0, 4))):      # ... and the same scenes answer in the forms they meet: 64 equal rays, 64 equal answers, the same in every form
        for form in forms:
            out, ids = _query(mi, sc, form, 0, rays, "form %d after the refusals" % form)
            assert (ids == ids[0]).all() and (out == out[0]).all() and (ids[0, 0] >= 0 or sc is mixed), (form, ids[0], out[0])
            ref = first.setdefault(id(sc), (out[0].copy(), ids[0].copy()))
            assert np.array_equal(ref[0], out[0]) and np.array_equal(ref[1], ids[0])
    assert first[id(boxes)][1][0] >= 0 and 3.0 < float(first[id(boxes)][0][0:1].view(np.float32)[0]) <= 4.001      # the tall box, in front of the room's back wall
