"""trace_flat's three walks against the oracle on dense and boundary rays: every scene of tests/flat_sweep.py through every form of dtof_flat_query the scene meets
(generic, one_wall, shape -- the instantiations of trace_flat the shade kernels of flat scenes carry, behind the stage, memo column and memo fill k_shade puts around
them), as closest-hit and as occlusion query, against orc_kat_flat_n (scene_closest / scene_occluded) on the same rays.  The rule is the project's contract: every
output word equal as a bit pattern -- the hit flag, the object, and t, u, v -- with no tolerance.  The forms a scene meets agree with each other, and so do the three
placements of a ray: in family order, under a fixed permutation, and as the one hit among certain misses in lists of 1, 63, 64 and 65 rays.
test_flat_sweep_cpu.py shows on the oracle alone that these rays sit below, on and above every compare; profiles/flat_sweep_mutations.txt records what the module catches."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import flat_sweep as fs
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu
INVALID, HIP = 1, 2
STATS_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_stats.so")
_ended_abnormally = []      # a call that reported a HIP error: nothing more is launched by this module


@pytest.fixture(scope="module")
def swept(mi, orc):
    """name -> (sweep, device scene, {(form, any): (t u v words or None, ids) of the rays in family order}); the last scene is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            t0 = time.time()
            sw = fs.Sweep(name, orc)
            print("%s: %d rays, generated and answered by the oracle in %.2f s" % (name, sw.n, time.time() - t0))
            cache[name] = (sw, mi.load_string(sw.xml, resx=16, resy=16), {})
        return cache[name]
    return get


def _query(mi, scene, form, any_hit, rays, what):
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    rc, out, ids = fs.device_query(mi, scene, form, any_hit, rays)
    if rc != 0:
        msg = "%s: return code %d, %s" % (what, rc, mi._lib().dtof_last_error().decode("utf-8", "replace"))
        if rc == HIP:
            _ended_abnormally.append(msg)
        pytest.fail(msg)
    never = int((ids.view(np.uint32) == fs.CANARY).sum()) + (0 if any_hit else int((out == fs.CANARY).sum()))
    assert never == 0, "%s: %d output words were never written" % (what, never)
    return out, ids


def _in_order(mi, entry, form, any_hit):
    sw, scene, got = entry
    if (form, any_hit) not in got:
        got[(form, any_hit)] = _query(mi, scene, form, any_hit, sw.rays, "%s, %s, %s, in family order" % (sw.name, fs.FORMS[form], fs.KINDS[any_hit]))
    return got[(form, any_hit)]


def _differing(a, b):
    """rows in which two answers (words or None, ids) differ"""
    bad = a[1] != b[1]
    if a[0] is not None:
        bad |= (a[0] != b[0]).any(axis=1)
    return np.flatnonzero(bad)


def _show(ans, i):
    return "ids %d" % ans[1][i] if ans[0] is None else "obj %d t %r u %r v %r" % ((int(ans[1][i]),) + tuple(float(x) for x in ans[0][i].view(np.float32)))


@pytest.mark.parametrize("name,form,kind", fs.CASES, ids=["%s-%s-%s" % (n, fs.FORMS[f], k) for n, f, k in fs.CASES])
def test_device_ray_query_equals_the_oracle(mi, swept, name, form, kind):
    entry = swept(name)
    sw, scene, _ = entry
    any_hit = fs.KINDS.index(kind)
    what = "%s, %s, %s" % (name, fs.FORMS[form], kind)
    t0 = time.time()
    got = _in_order(mi, entry, form, any_hit)
    want = fs.want_words(sw, any_hit)
    rows = _differing(got, want)
    print("%s: %d rays in family order, %d differ from the oracle" % (what, sw.n, len(rows)))
    assert len(rows) == 0, fs.describe(sw, rows, lambda i: _show(got, i), lambda i: _show(want, i), what + " against the oracle")
    # the same rays under the fixed permutation: mixed waves
    mixed = _query(mi, scene, form, any_hit, sw.rays[sw.perm], what + ", permuted")
    back = (None if any_hit else np.empty_like(mixed[0]), np.empty_like(mixed[1]))
    back[1][sw.perm] = mixed[1]
    if not any_hit:
        back[0][sw.perm] = mixed[0]
    rows = _differing(back, got)
    assert len(rows) == 0, fs.describe(sw, rows, lambda i: _show(back, i), lambda i: _show(got, i), what + ": permuted against in order (second answer)")
    # one ray that hits among certain misses, in lists of 1, 63, 64 and 65
    for label, idx in sw.short.items():
        short = _query(mi, scene, form, any_hit, sw.rays[idx], what + ", " + label)
        ref = (None if any_hit else got[0][idx], got[1][idx])
        rows = _differing(short, ref)
        assert len(rows) == 0, fs.describe(sw, idx[rows], lambda i: _show(short, int(np.flatnonzero(idx == i)[0])), lambda i: _show(got, i), "%s, %s against in order (second answer)" % (what, label))
    # the forms this scene meets agree word for word
    for other in sw.forms:
        if other < form:
            prev = _in_order(mi, entry, other, any_hit)
            rows = _differing(got, prev)
            assert len(rows) == 0, fs.describe(sw, rows, lambda i: _show(got, i), lambda i: _show(prev, i), "%s against the %s form (second answer)" % (what, fs.FORMS[other]))
    print("%s: in order, permuted, %d short lists, %d other forms: %.2f s" % (what, len(sw.short), sum(o < form for o in sw.forms), time.time() - t0))


def test_python_entry_is_the_same_call(mi, swept):
    sw, scene, _ = entry = swept("closed")
    for form in (0, "one_wall", "shape"):
        f = mi.Scene.FLAT_FORMS.get(form, form)
        r = scene.flat_query(sw.rays[:5000], form)
        words, ids = _in_order(mi, entry, f, 0)
        assert np.array_equal(np.stack([r["t"], r["u"], r["v"]], 1).view(np.uint32), words[:5000]) and np.array_equal(r["obj"], ids[:5000])
        assert np.array_equal(scene.flat_query(sw.rays[:5000], form, any=True), _in_order(mi, entry, f, 1)[1][:5000])
    assert len(scene.flat_query(sw.rays[:0])["t"]) == 0


def _refused(mi, scene, form, any_hit, rays, n=None):
    rays = np.ascontiguousarray(rays, np.float32)
    out, ids = np.full((len(rays), 3), fs.CANARY, np.uint32), np.full(len(rays), fs.CANARY, np.uint32)
    rc = mi._lib().dtof_flat_query(scene._h, form, any_hit, len(rays) if n is None else n, rays.ctypes.data, out.ctypes.data, ids.ctypes.data)
    return rc == INVALID and bool((out == fs.CANARY).all() and (ids == fs.CANARY).all()), mi._lib().dtof_last_error().decode()


def test_refusals_write_nothing_and_the_next_call_works(mi, swept):
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    rays = fs.rays8([[0, 1, 3]] * 64, [[0, 0, -1]] * 64, 0.0, np.inf)
    scene = {n: mi.load_string(fs.scene_xml(n), resx=16, resy=16) for n in ("closed", "wall_at_3", "six", "no_instance", "two_instances", "eight", "one")}
    boxes = mi.load_file(os.path.join(SCENES, "cornell_boxes.xml"), resx=16, resy=16)
    cases = [(boxes, 0, "no flat table"), (boxes, 2, "no flat table"), (scene["closed"], -1, "form must be"), (scene["closed"], 3, "form must be"),
             (scene["no_instance"], 1, "exactly one instance"), (scene["no_instance"], 2, "exactly one instance"), (scene["two_instances"], 1, "exactly one instance"),
             (scene["one"], 1, "exactly one instance"), (scene["wall_at_3"], 2, "this table has 5 and 3"), (scene["six"], 2, "this table has 6 and 2"),
             (scene["eight"], 2, "this table has 8 and 2")]
    for sc, form, reason in cases:
        for any_hit in (0, 1):
            ok, msg = _refused(mi, sc, form, any_hit, rays)
            assert ok and reason in msg, (form, any_hit, msg)
    for form in (0, 1, 2):
        ok, msg = _refused(mi, scene["closed"], form, 0, rays, n=(1 << 24) + 1)
        assert ok and "2^24" in msg, (form, msg)
    for name, forms in fs.SCENE_FORMS:      # every scene answers in the forms the sweep lists for it: the back wall (object 2, or 3, or the static wall) or the floor at t ~ 4
        sc = scene.get(name) or mi.load_string(fs.scene_xml(name), resx=16, resy=16)
        for form in forms:
            out, ids = _query(mi, sc, form, 0, rays, "%s, form %d" % (name, form))
            assert (ids == ids[0]).all() and (out == out[0]).all() and (ids[0] >= 0) == (name != "one"), (name, form, ids[:4])


def _count_full_tests():
    """(child process on the stats build) the room with the panel, every form: slots 16 .. 19 of the traversal counters after the occlusion queries of the sweep's
    shadow-ray-like segments, and after a list of certain misses only, as a JSON line"""
    sys.path.insert(0, ROOT)
    import ctypes as C
    import mitsuba3dopplertof_amd as mi
    from oracle import orc
    sw = fs.Sweep("panel", orc)
    scene = mi.load_string(sw.xml, resx=16, resy=16)
    slots = (C.c_ulonglong * 24)()
    out = {}
    for form in sw.forms:
        for label, rays in (("segments", sw.of("S", "A")), ("certain misses", sw.rays[sw.only_misses])):
            assert mi._lib().dtof_debug_traversal_stats_n(slots, 24) == 0      # (reads and resets)
            rc, _, ids = fs.device_query(mi, scene, form, True, rays)
            if rc != 0:
                print("FLAT_SWEEP_STATS_ERROR %d %s" % (rc, mi._lib().dtof_last_error().decode()))
                sys.exit(3)
            assert mi._lib().dtof_debug_traversal_stats_n(slots, 24) == 0
            out["%s/%s" % (fs.FORMS[form], label)] = dict(n=len(rays), occluded=int(ids.sum()), slots=[int(x) for x in slots[16:24]], rays=int(slots[0]))
    print("FLAT_SWEEP_STATS " + json.dumps(out))


def test_stats_build_counts_full_tests_for_the_sweep_and_none_for_certain_misses():
    """on the stats build (libdtof_stats.so) the occlusion queries of `panel` count full tests in slot 19 of dtof_traverse.h (waves in which some lane needed one) and a
    list of certain misses counts none: each of its z-row tests (slot 16, one per lane and rectangle) is settled there (slot 17)"""
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    assert os.path.exists(STATS_LIB), "libdtof_stats.so is not built (make -C mitsuba3dopplertof_amd/csrc stats; build() makes it)"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--count-full-tests"], env=dict(os.environ, DTOF_LIB=STATS_LIB), capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        _ended_abnormally.append("the stats child ended with status %d" % r.returncode)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = json.loads(re.search(r"^FLAT_SWEEP_STATS (.*)$", r.stdout, re.M).group(1))
    print(got)
    assert len(got) == 6
    for key, rec in got.items():
        lane_z, lane_settled, wave_z, wave_full = rec["slots"][:4]
        assert rec["rays"] == rec["n"] and lane_z == 5 * rec["n"] and rec["slots"][4:] == [0, 0, 0, 0], (key, rec)      # five z rows per ray, no closest-hit query
        if key.endswith("certain misses"):
            assert wave_full == 0 and lane_settled == lane_z and rec["occluded"] == 0, (key, rec)
        else:
            assert wave_full > 0 and lane_settled < lane_z and 0 < rec["occluded"] < rec["n"], (key, rec)


if __name__ == "__main__" and sys.argv[1:] == ["--count-full-tests"]:
    _count_full_tests()
