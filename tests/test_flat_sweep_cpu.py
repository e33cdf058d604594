"""The inputs of the flat-table sweep (tests/flat_sweep.py), judged by the oracle alone: that the sweep is not vacuous.  For every scene and rectangle each compare of the
rectangle test -- t >= 0, t <= maxt, |u| <= 1, |v| <= 1, and for the closest hit t < best -- is met from below, ON it and from above by rays for which the rectangle's
other compares pass, so that this compare decides; flat_certain_miss (the HOST compilation of dtof_flat_cull.h) both settles and does not settle rectangles in every
family and never settles one the oracle reports hit; family C holds t == maxt for every rectangle, family F equal-t pairs that go to the lower index, family H no hit.
Then what can be held of dtof_flat_query without a device: the symbol, its refusals, and that it has no CPU fallback.  The device leg is test_flat_sweep_gpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import flat_sweep as fs
from conftest import ROOT, SCENES

CSRC = os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc")
INVALID, HIP = 1, 2
COMPARES = ("t >= 0", "t <= maxt", "|u| <= 1", "|v| <= 1", "t < best")
# the second floor of the two scenes with ties repeats the floor (a lower index) bit for bit: whenever it passes, best already holds its own t -- never t < best
SECOND_FLOOR = {"ties_wall": 3, "ties": 5}


@pytest.fixture(scope="module")
def swept(orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = fs.Sweep(name, orc)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def cull(tmp_path_factory):
    """flat_certain_miss and flat_cull_far compiled for the host with the kernels' floating-point flags (tests/test_flat_cull.py does the same for its checker)"""
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("flat_sweep_cull")
    src, lib = str(d / "cull.cpp"), str(d / "libcull.so")
    open(src, "w").write(fs.CULL_SOURCE)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, src, "-o", lib])
    return C.CDLL(lib)


@pytest.mark.parametrize("name", fs.NAMES)
def test_every_compare_of_every_rectangle_is_met_from_below_on_it_and_from_above(swept, name):
    sw = swept(name)
    counts = fs.compare_classes(sw)
    print("%s: %d rays, %d rectangles; (below, on, above) of each compare where the rectangle's other compares pass" % (name, sw.n, sw.geo.n))
    for r in range(sw.geo.n):
        print("  rectangle %d (object %d): " % (r, sw.want["rect_obj"][r]) + ", ".join("%s %s" % (c, counts[(r, c)]) for c in COMPARES))
    for kind in fs.KINDS:
        for r in range(sw.geo.n):
            for c in COMPARES[:4] if kind == "occlusion" else COMPARES:      # t < best belongs to the closest hit
                below, on, above = counts[(r, c)]
                if c == "t < best" and r == 0:                                # the first rectangle visited meets best = maxt: t > best would not have passed t <= maxt
                    assert below > 0 and on > 0 and above == 0, (name, kind, r, c, counts[(r, c)])
                elif c == "t < best" and SECOND_FLOOR.get(name) == r:
                    assert below == 0 and on > 0 and above > 0, (name, kind, r, c, counts[(r, c)])
                else:
                    assert below > 0 and on > 0 and above > 0, (name, kind, r, c, counts[(r, c)])


@pytest.mark.parametrize("name", fs.NAMES)
def test_the_certain_miss_test_settles_and_does_not_settle_in_every_family_and_never_a_hit(swept, cull, name):
    sw = swept(name)
    ops, maxt = sw.want["ops"], sw.rays[:, 7]
    settled = fs.host_cull(cull, ops[..., fs.ZX], ops[..., fs.ZY], maxt[:, None]).reshape(ops.shape[:2])
    hit = fs.passes(ops, maxt)
    assert not (settled & hit).any(), (name, np.argwhere(settled & hit)[:5])
    # ... nor, stronger, one whose t lies in [0, maxt] (what dtof_flat_cull.h promises)
    with np.errstate(invalid="ignore"):
        in_range = (ops[..., fs.T] >= 0) & (ops[..., fs.T] <= maxt[:, None])
    assert not (settled & in_range).any(), (name, np.argwhere(settled & in_range)[:5])
    letter = np.array([{"S": "D", "HT": "H"}.get(f, f[0]) for f in sw.family])      # the families of the issue: A2 belongs to A, C2 to C, D2 and the segments S to D
    for fam in np.unique(letter):
        rows = (letter == fam) & sw.finite
        if not rows.any():
            continue
        n_settled, n_full = int(settled[rows].sum()), int((~settled[rows]).sum())
        print("%s, family %s: %d rectangle visits settled by the z row, %d go to the full test" % (name, fam, n_settled, n_full))
        if fam == "M":      # the certain misses are certain for every rectangle: the short lists and the stats test of the device leg rely on it
            assert n_full == 0 and n_settled == int(rows.sum()) * sw.geo.n, (name, fam)
        else:
            assert n_settled > 0 and n_full > 0, (name, fam, n_settled, n_full)
    # the rays without a number: never settled (NaN and infinities compare false and go to the full test, where they miss)
    nan = ~sw.finite
    assert nan.any() and not (sw.want["obj"][nan & (sw.family != "HT")] >= 0).any()


@pytest.mark.parametrize("name", fs.NAMES)
def test_family_c_holds_t_equal_to_maxt_for_every_rectangle(swept, name):
    """t == maxt: a hit for the occlusion query, none for the closest hit (hit = t != maxt) -- counted where the rectangle's t, u, v pass and no other rectangle is hit"""
    sw = swept(name)
    c = sw.family == "C"
    ops, maxt = sw.want["ops"][c], sw.rays[c, 7]
    ok = fs.passes(ops, maxt)
    for r in range(sw.geo.n):
        at = ok[:, r] & (ops[:, r, fs.T] == maxt)
        alone = at & (ok.sum(axis=1) == 1)
        print("%s, rectangle %d: %d rays of C with t == maxt, %d of them hit nothing else" % (name, r, int(at.sum()), int(alone.sum())))
        assert at.sum() > 0, (name, r)
        if name not in SECOND_FLOOR or r not in (0, SECOND_FLOOR[name]):      # (the two floors are never hit alone)
            assert alone.sum() > 0, (name, r)
            assert (sw.want["occluded"][c][alone] == 1).all() and (sw.want["obj"][c][alone] == -1).all(), (name, r)


@pytest.mark.parametrize("name", fs.TIE_SCENES)
def test_family_f_holds_equal_t_pairs_and_the_oracle_gives_them_to_the_lower_index(swept, name):
    sw = swept(name)
    ops, maxt = sw.want["ops"], sw.rays[:, 7]
    ok = fs.passes(ops, maxt) & sw.finite[:, None]
    with np.errstate(invalid="ignore"):
        closest = ok & (ops[..., fs.T] < maxt[:, None])      # a candidate of the closest hit: t != maxt
        t = np.where(closest, ops[..., fs.T], np.inf)
    tmin = t.min(axis=1)
    pairs = {}
    for a in range(sw.geo.n):
        for b in range(a + 1, sw.geo.n):
            rows = closest[:, a] & closest[:, b] & (t[:, a] == tmin) & (t[:, b] == tmin)
            if rows.any():
                first = np.argmax(t[rows] == tmin[rows, None], axis=1)      # the lowest rectangle that reports the smallest t
                assert (sw.want["obj"][rows] == sw.want["rect_obj"][first]).all(), (name, a, b)
                assert (sw.want["obj"][rows] <= sw.want["rect_obj"][a]).all()
                pairs[(a, b)] = (int(rows.sum()), int((rows & (sw.family == "F")).sum()))
    print(name, "rays whose two nearest candidates tie, by pair of rectangles (all families, family F):", pairs)
    floor2, wall, pose = SECOND_FLOOR[name], sw.geo.instances[0], sw.geo.n - 1
    assert pairs[(0, floor2)][1] > 0 and pairs[(wall, pose)][1] > 0, pairs


@pytest.mark.parametrize("name", fs.NAMES)
def test_family_h_yields_no_hit_and_the_array_entry_is_the_scalar_entries(orc, swept, name):
    sw = swept(name)
    h = sw.family == "H"
    assert h.sum() > 100 and (sw.want["obj"][h] == -1).all() and (sw.want["occluded"][h] == 0).all() and np.isinf(sw.want["t"][h]).all()
    # the words of a hit are the operands of a rectangle of the object it names, bit for bit -- zeros with their signs: a ray that starts in a rectangle's plane has
    # t = -zx / zy = +-0, and a negation folded into the multiply-add before it turns that sign round (oracle/dtof_oracle.c: neg_rounded)
    hit = np.flatnonzero(sw.want["obj"] >= 0)
    words = np.stack([sw.want["t"], sw.want["u"], sw.want["v"]], 1).view(np.uint32)[hit]
    operands = np.ascontiguousarray(sw.want["ops"][hit][:, :, [fs.T, fs.U, fs.V]]).view(np.uint32)
    same = (operands == words[:, None, :]).all(axis=2) & (sw.want["rect_obj"][None, :] == sw.want["obj"][hit, None])
    assert same.any(axis=1).all(), (name, hit[~same.any(axis=1)][:5])
    zero = sw.want["t"][hit] == 0
    assert (zero & np.signbit(sw.want["t"][hit])).sum() > 0 and (zero & ~np.signbit(sw.want["t"][hit])).sum() > 0      # hits at t = -0 and at t = +0
    # orc_kat_flat_n is orc_intersect / orc_occluded per ray (a thousand rays across all families)
    L = orc.lib()
    hit3, ids3 = (C.c_float * 3)(), (C.c_int32 * 3)()
    for i in np.random.default_rng(5).choice(sw.n, 1000, replace=False):
        r = sw.rays[i]
        o, d = (C.c_float * 3)(*r[0:3].tolist()), (C.c_float * 3)(*r[3:6].tolist())
        found = L.orc_intersect(C.byref(sw.osc.c), o, d, C.c_float(r[6]), C.c_float(r[7]), hit3, ids3)
        occ = L.orc_occluded(C.byref(sw.osc.c), o, d, C.c_float(r[6]), C.c_float(r[7]))
        want = np.array([hit3[0], hit3[1], hit3[2]], np.float32).view(np.uint32).tolist() + [ids3[0], occ]
        got = np.array([sw.want["t"][i], sw.want["u"][i], sw.want["v"][i]], np.float32).view(np.uint32).tolist() + [int(sw.want["obj"][i]), int(sw.want["occluded"][i])]
        assert got == want and found == (ids3[0] >= 0), (name, i, sw.family[i])


@pytest.mark.parametrize("name", fs.NAMES)
def test_the_placements(swept, name):
    sw = swept(name)
    assert sw.n <= 100_000                                                      # in order + permuted + the short lists: below 2 x 10^5 rays per (scene, form, kind)
    assert sorted(sw.perm.tolist()) == list(range(sw.n)) and (sw.perm != np.arange(sw.n)).mean() > 0.99
    mixed = sw.family[sw.perm][: 64 * (sw.n // 64)].reshape(-1, 64)
    assert np.mean([len(set(w)) > 2 for w in mixed]) > 0.95                     # the permutation mixes the families within a wave
    assert {len(v) for v in sw.short.values()} == {1, 63, 64, 65} and len(sw.short) >= 7
    for label, rows in sw.short.items():
        hits = sw.want["occluded"][rows] == 1
        assert hits.sum() == 1 and (sw.family[rows][~hits] == "M").all(), label
    for r in range(sw.geo.n):      # every rectangle has its ray with t == maxt whose exact quotient lies above maxt, alone among certain misses
        if name not in SECOND_FLOOR or r not in (0, SECOND_FLOOR[name]):
            assert any(k.startswith("rectangle %d, t == maxt rounded down" % r) for k in sw.short), (name, r)
            assert any(k.startswith("rectangle %d, t == 0" % r) for k in sw.short), (name, r)
    assert (sw.family[sw.only_misses] == "M").all() and len(sw.only_misses) == 128 and (sw.want["occluded"][sw.only_misses] == 0).all()


# ---------------------------------------------------------------------------- dtof_flat_query without a device
def test_header_declares_and_library_exports_the_entry(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    decl = re.search(r"\bint\s+dtof_flat_query\s*\(([^;]*)\)\s*;", hdr)
    assert decl and re.sub(r"\s+", " ", decl.group(1)) == "dtof_scene *scene, int form, int any, uint32_t n, const float *rays8, float *out3, int32_t *ids"
    for lib in ("libdtof.so", "libdtof_stats.so", "libdtof_pattern.so"):
        path = os.path.join(ROOT, "mitsuba3dopplertof_amd", lib)
        if lib == "libdtof.so" or os.path.exists(path):
            assert hasattr(C.CDLL(path), "dtof_flat_query"), lib
    assert mi.Scene.FLAT_FORMS == {"generic": 0, "one_wall": 1, "shape": 2}


def _refused(mi, scene, form, any_hit, rays, n=None):
    rays = np.ascontiguousarray(rays, np.float32)
    out, ids = np.full((max(len(rays), 1), 3), fs.CANARY, np.uint32), np.full(max(len(rays), 1), fs.CANARY, np.uint32)
    rc = mi._lib().dtof_flat_query(scene._h if scene is not None else None, form, any_hit, len(rays) if n is None else n, rays.ctypes.data, out.ctypes.data, ids.ctypes.data)
    return rc == INVALID and bool((out == fs.CANARY).all() and (ids == fs.CANARY).all()), mi._lib().dtof_last_error().decode()


def test_refusals_name_their_reason_and_write_nothing(mi):
    rays = fs.rays8([[0, 1, 3]] * 4, [[0, 0, -1]] * 4, 0.0, np.inf)
    scene = {n: mi.load_string(fs.scene_xml(n), resx=16, resy=16) for n in ("closed", "wall_at_3", "six", "no_instance", "two_instances", "eight", "one")}
    boxes = mi.load_file(os.path.join(SCENES, "cornell_boxes.xml"), resx=16, resy=16)      # cubes: no flat table
    cases = [("a scene without a flat table", boxes, 0, "no flat table"), ("... in the one_wall form", boxes, 1, "no flat table"),
             ("form -1", scene["closed"], -1, "form must be"), ("form 3", scene["closed"], 3, "form must be"),
             ("one_wall without an instance", scene["no_instance"], 1, "exactly one instance"), ("shape without an instance", scene["no_instance"], 2, "exactly one instance"),
             ("one_wall with two instances", scene["two_instances"], 1, "exactly one instance"), ("one_wall on one plain rectangle", scene["one"], 1, "exactly one instance"),
             ("shape with the wall at 3", scene["wall_at_3"], 2, "5 rectangles with the wall at index 2, this table has 5 and 3"),
             ("shape with six rectangles", scene["six"], 2, "this table has 6 and 2"), ("shape with eight rectangles", scene["eight"], 2, "this table has 8 and 2")]
    for what, sc, form, reason in cases:
        for any_hit in (0, 1):
            ok, msg = _refused(mi, sc, form, any_hit, rays)
            assert ok and reason in msg and msg.startswith("dtof_flat_query"), (what, any_hit, msg)
    for form in (0, 1, 2):
        ok, msg = _refused(mi, scene["closed"], form, 0, rays, n=(1 << 24) + 1)
        assert ok and "2^24" in msg, (form, msg)
    assert _refused(mi, None, 0, 0, rays)[0]
    L = mi._lib()
    ids = np.zeros(4, np.int32)
    assert L.dtof_flat_query(scene["closed"]._h, 0, 0, 4, None, ids.ctypes.data, ids.ctypes.data) == INVALID      # null rays
    assert L.dtof_flat_query(scene["closed"]._h, 0, 0, 4, rays.ctypes.data, None, ids.ctypes.data) == INVALID     # closest hit without out3
    assert L.dtof_flat_query(scene["closed"]._h, 0, 1, 4, rays.ctypes.data, None, None) == INVALID                # no ids
    with pytest.raises(mi.DtofError, match="exactly one instance"):
        scene["no_instance"].flat_query(rays, "one_wall")
    with pytest.raises(mi.DtofError, match="this table has 6 and 2"):
        scene["six"].flat_query(rays, "shape", any=True)


NO_DEVICE_CHILD = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
vp = C.c_void_p
L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
L.dtof_flat_query.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, vp, vp, vp]
h = vp()
names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
assert L.dtof_scene_load_file(sys.argv[2].encode(), names, values, 2, C.byref(h)) == 0
rays = (C.c_float * 16)(0, 1, 3, 0, 0, -1, 0, 10, 0, 1, 3, 0, 0, -1, 0, 10)
out, ids = (C.c_float * 6)(*([7.0] * 6)), (C.c_int32 * 2)(7, 7)
print(*[L.dtof_flat_query(h, form, any_hit, 2, rays, out, ids) for form in (0, 1, 2) for any_hit in (0, 1)], int(all(x == 7.0 for x in out) and all(x == 7 for x in ids)))
"""


def test_the_entry_fails_with_err_hip_without_a_device(mi):
    """no CPU fallback: arguments that pass every check reach the device set-up and fail there -- in a child process that sees no device, whatever this host has"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", NO_DEVICE_CHILD, mi.lib_path(), os.path.join(SCENES, "cornell_wall.xml")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(HIP)] * 6 + ["1"], r.stdout
