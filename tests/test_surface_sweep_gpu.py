"""The surface-interaction fill against the oracle on reachable and placed hits: every scene of tests/surface_sweep.py through every form of dtof_surface_eval the
scene meets -- the instantiations and argument patterns of compute_surface the kernels of a frame carry: the mesh kernels', the rectangle-only kernels' without a memo,
with the memo object's matrices from registers or from the lane's LDS columns, the one-wall kernels' with their precomputed frames, the mesh kernels' with the memo --
with and without the tangent frame, against orc_kat_surface_n (compute_si, offset_p) on the same hits.  Every one of the 32 words equal as a bit pattern: two NaNs are
equal, -0 and +0 differ, no tolerance, no row left out.  The layouts of a row agree: in family order, under a fixed permutation, and in lists of 1, 63, 64 and 65.
test_surface_sweep_cpu.py shows on the oracle alone that the rows are what this needs.

What the forms promise beyond "the oracle's record":
  want_frame = 0   p, n, sh_n, wi.z, uv and both offset points are the want_frame = 1 answer; sh_s, sh_t, dp_du, dp_dv, wi.x, wi.y are +0
  one_wall         dp_du = dp_dv = +0 with the frame as well (dtof_shading.h: no kernel of that form reads them); the other 26 words are the oracle's"""
import os

import numpy as np
import pytest

import surface_sweep as ss
from conftest import SCENES

pytestmark = pytest.mark.gpu
INVALID, HIP = 1, 2
ONE_WALL = 4
_ended_abnormally = []      # a call that reported a HIP error: nothing more is launched by this module


@pytest.fixture(scope="module")
def swept(mi, orc, tmp_path_factory):
    """name -> (sweep, device scene, the ids as the device takes them, {(form, want_frame): answer in family order}); the last scene is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            sw = ss.Sweep(name, orc, tmp_path_factory.mktemp(name))
            scene = mi.load_file(sw.path, resx=16, resy=16)
            # the table of forms (surface_sweep.SCENE_FORMS) is what the device says of the scene: the one-wall form where a frame plan finds the fact, and only there
            assert (ONE_WALL in sw.forms) == (scene.export(26)[0] == 1.0), (name, sw.forms, scene.export(26).tolist())
            cache[name] = (sw, scene, ss.device_ids(scene, sw.ids), {})
        return cache[name]
    return get


def _eval(mi, scene, form, want_frame, q, ids, what):
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    rc, out = ss.device_eval(mi, scene, form, want_frame, q, ids)
    if rc != 0:
        msg = "%s: return code %d, %s" % (what, rc, mi._lib().dtof_last_error().decode("utf-8", "replace"))
        if rc == HIP:
            _ended_abnormally.append(msg)
        pytest.fail(msg)
    never = int((out == ss.CANARY).sum())
    assert never == 0, "%s: %d output words were never written" % (what, never)
    return out.view(np.float32)


def _call(mi, what, fn, *args, **kw):
    """a call of the binding that is expected to succeed, under the module's rule: not started after a HIP error, and a failure of it ends the launches as one does"""
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    try:
        return fn(*args, **kw)
    except mi.DtofError as e:      # (the binding raises without the return code: an accepted call has no other way to fail than on the device)
        _ended_abnormally.append("%s: %s" % (what, e))
        pytest.fail(_ended_abnormally[0])


def _refused(mi, scene, form, want_frame, q, ids, reason, n=None):
    """a call that must be refused on the host: DTOF_ERR_INVALID with `reason`, the canary in every output word; a HIP error instead ends the launches"""
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    rc, out = ss.device_eval(mi, scene, form, want_frame, q, ids, n=n)
    msg = mi._lib().dtof_last_error().decode("utf-8", "replace")
    if rc == HIP:
        _ended_abnormally.append("a call to be refused (%s): return code %d, %s" % (reason, rc, msg))
        pytest.fail(_ended_abnormally[0])
    assert rc == INVALID and reason in msg, (form, want_frame, rc, msg)
    assert (out == ss.CANARY).all(), (form, reason, "a refused call wrote output words")


def _in_order(mi, entry, form, want_frame):
    sw, scene, dev_ids, got = entry
    if (form, want_frame) not in got:
        got[(form, want_frame)] = _eval(mi, scene, form, want_frame, sw.q, dev_ids, "%s, %s, want_frame %d, in family order" % (sw.name, ss.FORM_NAMES[form], want_frame))
    return got[(form, want_frame)]


def _expected(sw, form, want_frame):
    """the oracle's record in what the form promises of it"""
    want = sw.want.copy()
    if form == ONE_WALL:
        want[:, ss.DP_WORDS] = 0.0
    if not want_frame:
        want[:, ss.FRAME_WORDS] = 0.0
    return want


@pytest.mark.parametrize("name,form,want_frame", ss.CASES, ids=["%s-%s-%s" % (n, ss.FORM_NAMES[f], "frame" if w else "cosine") for n, f, w in ss.CASES])
def test_device_surface_equals_the_oracle(mi, swept, name, form, want_frame):
    entry = swept(name)
    sw, scene, dev_ids, _ = entry
    what = "%s, %s, want_frame %d" % (name, ss.FORM_NAMES[form], want_frame)
    got = _in_order(mi, entry, form, want_frame)
    want = _expected(sw, form, want_frame)
    rows = ss.differing(got, want)
    fam, cnt = np.unique(sw.family, return_counts=True)
    print("%s: %d rows (%s), %d differ from the oracle" % (what, sw.n, ", ".join("%s %d" % fc for fc in zip(fam, cnt)), len(rows)))
    assert len(rows) == 0, ss.describe(sw, rows, got, want, what + " (first) against the oracle (second)")
    if not want_frame:      # ... which is the want_frame = 1 answer of the same form in the words kept, and +0 (the bit pattern) in the others
        full = _in_order(mi, entry, form, 1)
        rows = ss.differing(got, full, ss.KEPT_WORDS)
        assert len(rows) == 0, ss.describe(sw, rows, got, full, what + " (first) against want_frame 1 (second)")
        assert not got.view(np.uint32)[:, ss.FRAME_WORDS].any(), what + ": a frame word that is not +0"
    if form == ONE_WALL:
        assert not got.view(np.uint32)[:, ss.DP_WORDS].any(), what + ": dp_du / dp_dv are not +0"
    # the same rows under the fixed permutation: mixed waves
    mixed = _eval(mi, scene, form, want_frame, sw.q[sw.perm], dev_ids[sw.perm], what + ", permuted")
    back = np.empty_like(mixed)
    back[sw.perm] = mixed
    rows = ss.differing(back, got)
    assert len(rows) == 0, ss.describe(sw, rows, back, got, what + ": permuted (first) against in order (second)")
    # the rows of B and C alone, in lists of 1, 63, 64 and 65: a partial wave, a full one, a second one
    for label, idx in sw.short.items():
        short = _eval(mi, scene, form, want_frame, sw.q[idx], dev_ids[idx], what + ", " + label)
        rows = ss.differing(short, got[idx])
        assert len(rows) == 0, "%s, %s: rows %s of the list differ from their answers in family order" % (what, label, rows.tolist())


@pytest.mark.parametrize("name", ss.NAMES)
def test_every_pair_of_forms_agrees(mi, swept, name):
    entry = swept(name)
    sw = entry[0]
    for want_frame in (1, 0):
        first = _in_order(mi, entry, sw.forms[0], want_frame)
        for form in sw.forms[1:]:
            words = np.setdiff1d(np.arange(32), ss.DP_WORDS) if form == ONE_WALL and want_frame else slice(None)
            rows = ss.differing(_in_order(mi, entry, form, want_frame), first, words)
            assert len(rows) == 0, ss.describe(sw, rows, _in_order(mi, entry, form, want_frame), first, "%s, want_frame %d: %s (first) against %s (second)" % (
                name, want_frame, ss.FORM_NAMES[form], ss.FORM_NAMES[sw.forms[0]]))


@pytest.mark.parametrize("name", ss.NAMES)
def test_form_0_on_the_reachable_family_is_dtof_ray_intersect(mi, swept, name):
    entry = swept(name)
    sw, scene, _, _ = entry
    a = np.flatnonzero(sw.family == "A")
    got = _in_order(mi, entry, 0, 1)[a]
    r = _call(mi, name + ", ray_intersect", scene.ray_intersect, sw.rays_a[:, 0:3], sw.rays_a[:, 3:6], sw.rays_a[:, 6], sw.rays_a[:, 7])
    assert np.array_equal(np.asarray(r["ids"], np.int32), sw.ids[a]), "the device's ray query reports other ids than the oracle's (tests/test_tree_sweep_gpu.py holds it to them)"
    assert np.array_equal(ss.bits(r["t"]), ss.bits(sw.q[a, 7])) and np.array_equal(ss.bits(r["prim_uv"]), ss.bits(sw.q[a, 8:10]))
    mine = np.concatenate([got[:, 0:18], got[:, ss.UV]], axis=1)
    theirs = np.concatenate([r["p"], r["n"], r["sh_n"], r["sh_s"], r["sh_t"], r["wi"], r["uv"]], axis=1)
    bad = np.flatnonzero((ss.bits(mine) != ss.bits(theirs)).any(axis=1))
    assert len(bad) == 0, "%s: %d reachable rows differ from dtof_ray_intersect_uv, first %d" % (name, len(bad), bad[0])
    # ... and the Python entry is the same call
    dev_ids = entry[2]
    what = name + ", Scene.surface_eval"
    assert np.array_equal(ss.bits(_call(mi, what, scene.surface_eval, sw.q[:500], dev_ids[:500], "mesh")), ss.bits(_in_order(mi, entry, 0, 1)[:500]))
    assert np.array_equal(ss.bits(_call(mi, what, scene.surface_eval, sw.q[:500], dev_ids[:500], 0, want_frame=False)), ss.bits(_in_order(mi, entry, 0, 0)[:500]))
    assert _call(mi, what, scene.surface_eval, sw.q[:0], dev_ids[:0]).shape == (0, 32)


def test_refusals_write_nothing_and_the_next_call_works(mi, orc, tmp_path):
    if _ended_abnormally:
        pytest.fail("nothing is launched after a call that reported a HIP error: %s" % _ended_abnormally[0])
    scenes = {n: mi.load_file(ss.build(n, tmp_path), resx=16, resy=16) for n in ("analytic", "mesh", "flat_pair")}
    scenes["cornell_wall"] = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=16, resy=16)
    scenes["cornell_boxes"] = mi.load_file(os.path.join(SCENES, "cornell_boxes.xml"), resx=16, resy=16)      # two instances: no memo object
    q = np.tile(ss.row((0, 1, 3), (0, 0, -1), 0.0, 1.0, 0.25, 0.25), (64, 1))
    ok = np.zeros((64, 3), np.int32)
    cases = ([("analytic", f, ok, "not a rectangle") for f in (1, 2, 3, 4)] + [("mesh", f, ok, "not a rectangle") for f in (1, 2, 3, 4)] +
             [("flat_pair", 4, ok, "one_wall form needs")] + [("cornell_boxes", f, ok, "not a rectangle") for f in (1, 2, 3, 4)] + [("cornell_boxes", 5, ok, "memo object")] +
             [("cornell_wall", -1, ok, "form must be"), ("cornell_wall", 6, ok, "form must be")])
    n_obj = {"cornell_wall": 5, "mesh": 6}
    for name, bad, reason in (("cornell_wall", (5, 0, 0), "object out of range"), ("cornell_wall", (-1, 0, 0), "object out of range"), ("cornell_wall", (2, 1, 0), "shape beyond"),
                              ("cornell_wall", (0, 1, 0), "shape beyond"), ("cornell_wall", (0, -1, 0), "shape beyond"), ("mesh", (0, 0, 8), "primitive beyond"),
                              ("mesh", (0, 0, -1), "primitive beyond"), ("mesh", (n_obj["mesh"], 0, 0), "object out of range")):
        ids = ok.copy(); ids[63] = bad      # the last row of the list alone is out of range
        cases.append((name, 0, ids, reason))
    for name, form, ids, reason in cases:
        for want_frame in (0, 1):
            _refused(mi, scenes[name], form, want_frame, q, ids, reason)
    _refused(mi, scenes["cornell_wall"], 0, 2, q, ok, "want_frame")
    _refused(mi, scenes["cornell_wall"], 0, 1, q, ok, "2^24", n=(1 << 24) + 1)
    # (the issue's "scene without a device blob" has no case: the library's only constructor of a scene builds the blob or fails, so the binding cannot make one)
    # ... and the same scenes answer in the forms they meet: 64 equal hits, 64 equal records, the oracle's
    osc = orc.Scene(os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16))
    want = osc.surface_n(q, ok)[0]
    for form in (0, 1, 2, 3, 4, 5):
        got = _eval(mi, scenes["cornell_wall"], form, 1, q, ok, "form %d after the refusals" % form)
        words = np.setdiff1d(np.arange(32), ss.DP_WORDS) if form == ONE_WALL else slice(None)
        assert len(ss.differing(got, want, words)) == 0, form
