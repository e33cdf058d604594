"""The tree walk of the fused shade kernels and the analytic shapes' ray tests against the brute-force oracle on dense and boundary rays: every scene of
tests/fused_sweep.py through every form of dtof_fused_query the scene meets -- the classic launch's walk with the blob staged or in global memory, the rectangle-only
instantiation, the resident stage's SOA planes with 32-bit and with 16-bit references and stack columns, its half-float planes, each resident form at every wave count
that fits -- as closest-hit and as occlusion query, against orc_kat_tree_n (scene_closest / scene_occluded) on the same rays.  Every output word equal as a bit pattern
-- t, u, v, object, shape, primitive, the occlusion flag -- with no tolerance and no ray left out.  The placements of a ray agree: in family order, under a fixed
permutation, and as the one hit among certain misses in lists of 1, 63, 64, 65 rays and of a block less one, a block and a block plus one.  The analytic scenes' rays
also go through dtof_tree_query form 0 (k_ray_query's instantiation), and form 0 of the two entries agrees on every scene.  test_fused_sweep_cpu.py shows on the oracle
alone that the rays are what this needs."""
import time

import numpy as np
import pytest

import fused_sweep as fz
import tree_sweep as ts

pytestmark = pytest.mark.gpu
INVALID, HIP = 1, 2
_ended_abnormally = []      # a call that reported a HIP error: nothing more is launched by this module


@pytest.fixture(scope="module")
def swept(mi, orc, tmp_path_factory):
    """name -> (sweep, device scene, {(entry, form, waves, any): answer for the rays in family order}); the last scene is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            t0 = time.time()
            sw = fz.Sweep(name, orc, tmp_path_factory.mktemp(name))
            print("%s: %d rays, generated and answered by the oracle in %.2f s" % (name, sw.n, time.time() - t0))
            cache[name] = (sw, mi.load_file(sw.path, resx=16, resy=16), {})
        return cache[name]
    return get


def _launch_allowed():
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])


def _query(mi, scene, form, waves, any_hit, rays, what, entry="fused"):
    _launch_allowed()
    rc, out, ids = fz.device_query(mi, scene, form, waves, any_hit, rays) if entry == "fused" else ts.device_query(mi, scene, form, any_hit, rays)
    if rc != 0:
        msg = "%s: return code %d, %s" % (what, rc, mi._lib().dtof_last_error().decode("utf-8", "replace"))
        if rc == HIP:
            _ended_abnormally.append(msg)
        pytest.fail(msg)
    never = int((ids.view(np.uint32) == fz.CANARY).sum()) + (0 if any_hit else int((out == fz.CANARY).sum()))
    assert never == 0, "%s: %d output words were never written" % (what, never)
    return out, ids


def _in_order(mi, cached, form, waves, any_hit, entry="fused"):
    sw, scene, got = cached
    key = (entry, form, waves, any_hit)
    if key not in got:
        got[key] = _query(mi, scene, form, waves, any_hit, sw.rays, "%s, %s %d at %d waves, %s, in family order" % (sw.name, entry, form, waves, fz.KINDS[any_hit]), entry)
    return got[key]


def _equals_the_oracle(sw, got, any_hit, what):
    want = ts.want_words(sw, any_hit)
    rows = ts.differing(got, want)
    print("%s: %d rays in family order, %d differ from the oracle" % (what, sw.n, len(rows)))
    assert len(rows) == 0, ts.describe(sw, rows, lambda i: ts.show(got, i), lambda i: ts.show(want, i), what + " (first) against the oracle (second)")


@pytest.mark.parametrize("name,form,waves,kind", fz.CASES, ids=[fz.case_id(*c) for c in fz.CASES])
def test_device_fused_query_equals_the_oracle(mi, swept, name, form, waves, kind):
    cached = swept(name)
    sw, scene, _ = cached
    any_hit = fz.KINDS.index(kind)
    what = fz.case_id(name, form, waves, kind)
    t0 = time.time()
    got = _in_order(mi, cached, form, waves, any_hit)
    _equals_the_oracle(sw, got, any_hit, what)
    # the same rays under the fixed permutation: mixed waves
    mixed = _query(mi, scene, form, waves, any_hit, sw.rays[sw.perm], what + ", permuted")
    back = (None if any_hit else np.empty_like(mixed[0]), np.empty_like(mixed[1]))
    back[1][sw.perm] = mixed[1]
    if not any_hit:
        back[0][sw.perm] = mixed[0]
    rows = ts.differing(back, got)
    assert len(rows) == 0, ts.describe(sw, rows, lambda i: ts.show(back, i), lambda i: ts.show(got, i), what + ": permuted (first) against in order (second)")
    # one ray that hits among certain misses: lists of 1, 63, 64, 65 and, for a resident form, around its own block size
    lists = {label: idx for label, idx in sw.short.items() if len(idx) <= 65 or (waves and abs(len(idx) - waves * 64) <= 1)}
    assert len(lists) >= (8 if waves else 5)
    for label, idx in lists.items():
        short = _query(mi, scene, form, waves, any_hit, sw.rays[idx], what + ", " + label)
        ref = (None if any_hit else got[0][idx], got[1][idx])
        rows = ts.differing(short, ref)
        assert len(rows) == 0, "%s, %s: rays %s of the list differ from their answers in family order" % (what, label, rows.tolist())
    print("%s: in order, permuted, %d short lists: %.2f s" % (what, len(lists), time.time() - t0))


@pytest.mark.parametrize("name", fz.NAMES)
def test_form_0_is_form_0_of_the_tree_query(mi, swept, name):
    """... and on the analytic scenes, whose families are new to it, dtof_tree_query's form 0 (the instantiation k_ray_query carries) is held to the oracle too"""
    cached = swept(name)
    sw, scene, _ = cached
    for any_hit in (0, 1):
        tree = _in_order(mi, cached, 0, 0, any_hit, "tree")
        if name in fz.TREE_FORM_0:
            _equals_the_oracle(sw, tree, any_hit, "%s, dtof_tree_query form 0, %s" % (name, fz.KINDS[any_hit]))
        fused = _in_order(mi, cached, 0, 0, any_hit)
        rows = ts.differing(fused, tree)
        assert len(rows) == 0, ts.describe(sw, rows, lambda i: ts.show(fused, i), lambda i: ts.show(tree, i), name + ": dtof_fused_query form 0 (first) against dtof_tree_query form 0 (second)")
    # the Python entry is the same call
    words, ids = _in_order(mi, cached, 0, 0, 0)
    q = scene.fused_query(sw.rays[:2000], "classic")
    assert np.array_equal(np.stack([q["t"], q["u"], q["v"]], 1).view(np.uint32), words[:2000]) and np.array_equal(q["ids"], ids[:2000])
    form, waves = sw.forms[-1]
    assert np.array_equal(scene.fused_query(sw.rays[:2000], fz.FORM_NAMES[form], waves=waves or 8, any=True), _in_order(mi, cached, form, waves, 1)[1][:2000])
    assert len(scene.fused_query(sw.rays[:0])["t"]) == 0


def test_refusals_write_nothing_and_the_next_call_works(mi, tmp_path):
    _launch_allowed()
    rays = fz.rays([[0, 3, 0.1]] * 64, [[0, -1, 0]] * 64)      # down onto PoleDisk / ExactBall
    field = mi.load_file(fz.build("analytic_field", tmp_path), resx=16, resy=16)
    small = mi.load_file(fz.build("analytic_small", tmp_path), resx=16, resy=16)
    cases = [(field, 1, 0, "rectangle code only"), (field, 4, 8, "half-float planes"), (field, 2, 16, "bytes of LDS"), (field, 2, 10, "waves must be"), (field, 6, 8, "form must be"),
             (small, 2, 8, "no resident layout"), (small, 3, 16, "no resident layout"), (small, 1, 0, "rectangle code only")]
    for sc, form, waves, reason in cases:
        for any_hit in (0, 1):
            rc, out, ids = fz.device_query(mi, sc, form, waves, any_hit, rays)
            msg = mi._lib().dtof_last_error().decode()
            assert rc == INVALID and reason in msg and msg.startswith("dtof_fused_query:"), (form, waves, any_hit, rc, msg)
            assert (ids.view(np.uint32) == fz.CANARY).all() and (out is None or (out == fz.CANARY).all())
    rc, out, ids = fz.device_query(mi, field, 0, 0, 0, rays, n=(1 << 24) + 1)
    assert rc == INVALID and "2^24" in mi._lib().dtof_last_error().decode() and (ids.view(np.uint32) == fz.CANARY).all() and (out == fz.CANARY).all()
    for sc, forms in ((field, dict(fz.SCENE_FORMS)["analytic_field"]), (small, dict(fz.SCENE_FORMS)["analytic_small"])):      # ... and the same scenes answer in the forms they meet
        first = None
        for form, waves in forms:
            out, ids = _query(mi, sc, form, waves, 0, rays, "form %d at %d waves after the refusals" % (form, waves))
            assert (ids == ids[0]).all() and (out == out[0]).all() and ids[0, 0] >= 0, (form, waves, ids[0], out[0])
            first = first or (out[0].copy(), ids[0].copy())
            assert np.array_equal(first[0], out[0]) and np.array_equal(first[1], ids[0])
    assert first[1][0] == 1 and 1.49 < float(first[0][0:1].view(np.float32)[0]) < 1.51      # analytic_small: the disk on the sphere's pole, from 1.5 above it
