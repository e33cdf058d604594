"""trace_flat's pair form (mitsuba3dopplertof_amd/csrc/dtof_traverse.h: PAIR_RAYS; dtof_pair_walk.h): two lanes that hold the same ray -- the two members
of a correlated pair, whose times differ and reach the moving wall alone -- share the four plain rectangles of cornell_wall's table between them, the even lane testing
those below the wall and the odd lane those above it.  The form must answer what the plain walk answers, word for word.

  1. (no GPU) tests/pair_walk_check.cpp: the merge against the ascending strict-< walk, exhaustively over five rectangles whose t come from a set with equal values
     across the halves and with the wall, t == maxt, NaN and misses;
  2. dtof_flat_query_pairs against form 0 of dtof_flat_query (which tests/test_flat_sweep_gpu.py holds to the oracle) on the same rays, bit for bit, closest hit and
     occlusion: every ray of the sweeps of `closed`, `panel` and `ties_wall` (tests/flat_sweep.py) issued as a pair -- its own time and a second one -- plus family G's
     rays with maxt between the wall's two hit distances paired so that ONE lane of the pair hits the wall; in family order, with the pairs permuted, and in lists of
     2, 62, 64 and 66 rays around one pair that hits; the refusals (an odd count, a pair that differs in o, d or maxt, a table of another shape);
  3. films of the headline kernel, which runs the form for every camera ray: 1 x 1 crops of cornell_wall 16 x 16 x 64 whose 64 camera rays the oracle puts all on
     plain rectangles, all on the wall, or on both -- among the last one with a pair whose members hit different objects -- against DTOF_PLAN_FACTS=0, as
     tests/test_pair_samples.py does (film bits, statistics, the mask that ran); the frame against the oracle's film; the crops on the pattern-initialised library;
     the fall-backs, which keep their kernels and bits.  (An occlusion query has no pair form -- DESIGN 8.3 (k): it cost more than it saved -- and
     dtof_flat_query_pairs answers it with the shaped sweep; the query tests run both kinds all the same.)

A crop's samples are not the full frame's (the sampler counts pixels inside the crop window), so a crop's class is read off the oracle's lanes of the CROP scene."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import flat_sweep as fs
import test_pair_samples as ps
from conftest import ROOT, SCENES

INVALID = 1
WALL = 2
PAIR_SCENES = ("closed", "panel", "ties_wall")
G_BLOCK = 400            # flat_sweep.Sweep._wall: m rays per instance at the first time, m at the second, then the two lists with maxt between the hit distances
SEEDS = ps.SEEDS
SPP = ps.SPP
PARAMS = dict(resx=16, resy=16, max_depth=4)


# ---------------------------------------------------------------------------- 1. the merge on the host
def test_merge_equals_the_ascending_walk_on_the_host(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "pair_walk_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", ps.CSRC, os.path.join(ROOT, "tests", "pair_walk_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    r = {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()}
    assert r["cases"] == 2 * 3 * 7 ** 6 and r["mismatches"] == 0
    for k in ("none", "lower_wins", "wall_wins", "upper_wins", "ties_across", "ties_wall", "lanes_differ", "at_maxt"):      # every kind of case occurs
        assert r[k] > 0, (k, r)


# ---------------------------------------------------------------------------- 2. the query
def _pair_query(mi, scene, any_hit, rays, n=None):
    """dtof_flat_query_pairs into buffers pre-filled with the sweep's canary -> (return code, (n, 3) words or None, ids)"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    out, ids = np.full((len(rays), 3), fs.CANARY, np.uint32), np.full(len(rays), fs.CANARY, np.uint32)
    rc = mi._lib().dtof_flat_query_pairs(scene._h, 1 if any_hit else 0, len(rays) if n is None else n, rays.ctypes.data, None if any_hit else out.ctypes.data, ids.ctypes.data)
    return rc, (None if any_hit else out), ids.view(np.int32)


def _answers(mi, scene, any_hit, rays, what):
    """(pair form, form 0) of the same rays, each (words or None, ids); both calls must succeed and write every word"""
    got = []
    for label, (rc, out, ids) in (("pairs", _pair_query(mi, scene, any_hit, rays)), ("form 0", fs.device_query(mi, scene, 0, any_hit, rays))):
        assert rc == 0, "%s, %s: return code %d, %s" % (what, label, rc, mi._lib().dtof_last_error().decode("utf-8", "replace"))
        never = int((ids.view(np.uint32) == fs.CANARY).sum()) + (0 if any_hit else int((out == fs.CANARY).sum()))
        assert never == 0, "%s, %s: %d output words were never written" % (what, label, never)
        got.append((out, ids))
    return got


def _differing(a, b):
    bad = a[1] != b[1]
    if a[0] is not None:
        bad |= (a[0] != b[0]).any(axis=1)
    return np.flatnonzero(bad)


def _report(rays, rows, a, b, what):
    lines = ["%s: %d of %d rays differ" % (what, len(rows), len(rays))]
    for i in rows[:6]:
        show = lambda ans: "ids %d" % ans[1][i] if ans[0] is None else "obj %d t u v %s" % (int(ans[1][i]), ans[0][i].view(np.float32).tolist())
        lines.append("  ray %d (lane %d of its wave): %s\n    pair form %s   form 0 %s" % (i, i % 64, rays[i].tolist(), show(a), show(b)))
    return "\n".join(lines)


@pytest.fixture(scope="module")
def paired(mi, orc):
    """name -> (sweep, device scene, (2 n, 8) rays in pairs, first row of the family G pairs with maxt between the wall's two hit distances); the last scene is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            sw = fs.Sweep(name, orc)
            second = fs._times(np.random.default_rng([fs.SEED, 77, fs.NAMES.index(name)]), sw.n).astype(np.float32)
            rays = np.repeat(sw.rays, 2, axis=0)
            rays[1::2, 6] = second
            # family G behind its two blocks of G_BLOCK rays: k rays at the first time and the same k at the second, both with maxt between the two hit distances
            g = sw.of("G")
            assert len(sw.geo.instances) == 1 and len(g) > 2 * G_BLOCK and (len(g) - 2 * G_BLOCK) % 2 == 0
            k = (len(g) - 2 * G_BLOCK) // 2
            between = np.empty((2 * k, 8), np.float32)
            between[0::2], between[1::2] = g[2 * G_BLOCK:2 * G_BLOCK + k], g[2 * G_BLOCK + k:]
            rays = np.ascontiguousarray(np.concatenate([rays, between]))
            same = (rays[0::2, :6].view(np.uint32) == rays[1::2, :6].view(np.uint32)).all() and (rays[0::2, 7].view(np.uint32) == rays[1::2, 7].view(np.uint32)).all()
            assert same and (rays[0::2, 6] != rays[1::2, 6]).mean() > 0.5
            cache[name] = (sw, mi.load_string(sw.xml, resx=16, resy=16), rays, 2 * sw.n)
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [(n, k) for n in PAIR_SCENES for k in fs.KINDS], ids=["%s-%s" % (n, k) for n in PAIR_SCENES for k in fs.KINDS])
def test_pair_form_answers_what_the_generic_walk_answers(mi, paired, name, kind):
    sw, scene, rays, g_at = paired(name)
    any_hit = fs.KINDS.index(kind)
    what = "%s, %s" % (name, kind)
    # in family order: homogeneous waves
    got, ref = _answers(mi, scene, any_hit, rays, what + ", in family order")
    rows = _differing(got, ref)
    print("%s: %d rays in %d pairs, %d differ from form 0" % (what, len(rays), len(rays) // 2, len(rows)))
    assert len(rows) == 0, _report(rays, rows, got, ref, what + ", in family order")
    # the rays are what the case is about: family G's pairs with maxt between the two distances have ONE member on the wall, family F ties rectangles of both halves
    ids = ref[1]
    split = (ids[g_at::2] == (1 if any_hit else WALL)) != (ids[g_at + 1::2] == (1 if any_hit else WALL))
    print("%s: %d of %d family G pairs have one member %s" % (what, int(split.sum()), len(split), "occluded" if any_hit else "on the wall"))
    assert split.sum() > 10
    if not any_hit:
        assert (ids[:g_at:2] != ids[1:g_at:2]).sum() > 10      # ... and pairs of the sweep proper differ too: a second time moves the wall
        if name == "ties_wall":
            ops = sw.want["ops"][sw.family == "F"]
            ok = fs.passes(ops, sw.rays[sw.family == "F", 7])
            tie = lambda a, b: ok[:, a] & ok[:, b] & (ops[:, a, fs.T] == ops[:, b, fs.T])
            across = tie(0, 3) | tie(0, 4) | tie(1, 3) | tie(1, 4)
            with_wall = tie(0, WALL) | tie(1, WALL) | tie(3, WALL) | tie(4, WALL)
            print("ties_wall: %d rays of family F pass a rectangle of each half at one t, %d the wall and a plain rectangle" % (int(across.sum()), int(with_wall.sum())))
            assert list(sw.want["rect_obj"]) == [0, 1, 2, 3, 4] and across.sum() > 10 and with_wall.sum() > 10
    # the pairs under a fixed permutation: mixed waves
    perm = np.random.default_rng([fs.SEED, 98]).permutation(len(rays) // 2)
    idx = np.stack([2 * perm, 2 * perm + 1], 1).ravel()
    mixed, mixed_ref = _answers(mi, scene, any_hit, rays[idx], what + ", pairs permuted")
    rows = _differing(mixed, mixed_ref)
    assert len(rows) == 0, _report(rays[idx], rows, mixed, mixed_ref, what + ", pairs permuted")
    rows = _differing(mixed, (None if any_hit else ref[0][idx], ref[1][idx]))
    assert len(rows) == 0, _report(rays[idx], rows, mixed, ref, what + ": permuted against in order")
    # lists of 2, 62, 64 and 66 rays: pairs of certain misses around ONE pair that hits, one such pair per object
    miss = 2 * np.flatnonzero(sw.family == "M")
    hits = np.flatnonzero((sw.family == "A") & (sw.want["obj"] >= 0) & (sw.want["occluded"] == 1))
    n_lists = 0
    for o in np.unique(sw.want["obj"][hits]):
        h = 2 * int(hits[sw.want["obj"][hits] == o][0])
        for n, at in ((2, 0), (62, 16), (62, 60), (64, 0), (64, 62), (64, 30), (66, 64), (66, 6)):
            first = miss[(np.arange(n // 2) + 7 * int(o)) % len(miss)].copy()
            first[at // 2] = h
            rows_ = np.stack([first, first + 1], 1).ravel()
            short, short_ref = _answers(mi, scene, any_hit, rays[rows_], "%s, %d rays, the pair that hits object %d in lanes %d and %d" % (what, n, o, at, at + 1))
            bad = _differing(short, short_ref)
            assert len(bad) == 0, _report(rays[rows_], bad, short, short_ref, "%s, %d rays, the hit in lane %d" % (what, n, at))
            assert (short[1][at] == 1 if any_hit else short[1][at] == o) and len(_differing(short, (None if any_hit else ref[0][rows_], ref[1][rows_]))) == 0
            n_lists += 1
    assert n_lists >= 8 * 3
    print("%s: in order, permuted and %d short lists agree with form 0" % (what, n_lists))


@pytest.mark.gpu
def test_python_entry_and_refusals(mi, paired):
    sw, scene, rays, _ = paired("closed")
    lib = mi._lib()
    r = scene.flat_query_pairs(rays[:4096])
    rc, words, ids = _pair_query(mi, scene, 0, rays[:4096])
    assert rc == 0 and np.array_equal(np.stack([r["t"], r["u"], r["v"]], 1).view(np.uint32), words) and np.array_equal(r["obj"], ids)
    assert np.array_equal(scene.flat_query_pairs(rays[:4096], any=True), _pair_query(mi, scene, 1, rays[:4096])[2])
    assert len(scene.flat_query_pairs(rays[:0])["t"]) == 0

    def refused(sc, any_hit, rr, reason, n=None):
        rc, out, ids_ = _pair_query(mi, sc, any_hit, rr, n)
        msg = lib.dtof_last_error().decode()
        assert rc == INVALID and (ids_.view(np.uint32) == fs.CANARY).all() and (out is None or (out == fs.CANARY).all()) and reason in msg, (rc, msg, reason)

    good = np.ascontiguousarray(rays[:64])
    for any_hit in (0, 1):
        refused(scene, any_hit, good, "odd number", n=63)
        refused(scene, any_hit, good[:1], "odd number")
        for col in (0, 2, 3, 5, 7):      # o, d and maxt each: one word of one member differs
            bad = good.copy()
            bad[41, col] = np.nextafter(bad[41, col], np.float32(7.0), dtype=np.float32) if np.isfinite(bad[41, col]) else np.float32(1.0)
            assert bad[41, col].view(np.uint32) != good[41, col].view(np.uint32)
            refused(scene, any_hit, bad, "rays 40 and 41 differ")
        for name in ("wall_at_3", "six"):
            refused(mi.load_string(fs.scene_xml(name), resx=16, resy=16), any_hit, good, "5 rectangles")
        refused(mi.load_file(os.path.join(SCENES, "cornell_boxes.xml"), resx=16, resy=16), any_hit, good, "no flat table")
        with pytest.raises(mi.DtofError):
            scene.flat_query_pairs(good[:3], any=bool(any_hit))
        # ... and the next call works
        (out, ids), (out0, ids0) = _answers(mi, scene, any_hit, good, "after the refusals")
        assert np.array_equal(ids, ids0) and (any_hit or np.array_equal(out, out0))


# ---------------------------------------------------------------------------- 3. films
STATIC, ALL_WALL, MIXED = 0, 1, 2
CLASS_NAMES = ("static", "wall", "mixed")


def _classify(osc, seed, n_pixels):
    """per pixel of the oracle scene: (class, number of pairs whose members hit different objects), from the oracle's camera rays (render_lanes) and their closest
    hits (flat_n); the two members of every pair must hold one ray"""
    lanes = osc.render_lanes(osc.params(), seed, SPP, 0, n_pixels * SPP, threads=ps.NCPU)
    rays = np.concatenate([lanes["ray_o"], lanes["ray_d"], lanes["time"][:, None], np.full((len(lanes), 1), np.inf, np.float32)], 1).astype(np.float32)
    assert np.array_equal(rays[0::2, :6].view(np.uint32), rays[1::2, :6].view(np.uint32)) and (rays[0::2, 6] != rays[1::2, 6]).all()
    obj = osc.flat_n(rays, False)["obj"].reshape(n_pixels, SPP)
    wall = obj == WALL
    cls = np.where(wall.all(axis=1), ALL_WALL, np.where((~wall).all(axis=1), STATIC, MIXED))
    return cls, (obj[:, 0::2] != obj[:, 1::2]).sum(axis=1)


@pytest.fixture(scope="module")
def wall():
    """variants of scenes/cornell_wall.xml (test_pair_samples._variant) written next to it and removed afterwards"""
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(rfilter="tent", crop=None, integrator_props="", second_light=False):
        key = (rfilter, crop, integrator_props, second_light)
        if key not in made:
            made[key] = os.path.join(SCENES, "_pair_walk_%d_%d.xml" % (os.getpid(), len(made)))
            open(made[key], "w").write(ps._variant(base, rfilter, crop, integrator_props, second_light))
        return made[key]
    yield get
    for p in made.values():
        os.remove(p)


@pytest.fixture(scope="module")
def crops(orc, wall):
    """{seed: {case: [(crop, seed of its frames), ...]}}: the frame's pixels classified by the oracle, then, of each class, two crops whose OWN 64 camera rays are of
    that class.  "split": the crop of a mixed pixel of the frame that holds a pair whose members hit different objects, at the seed -- and the same crop at the
    first other seed at which the CROP's rays hold such a pair (the 64 sample offsets of a one-pixel crop are the same in every crop of a seed, and at seeds 4 and 11
    none of the 256 crops puts one of them between the wall's two edges; the frame's own split pairs are what the frame test renders)"""
    chosen = {}
    for seed in SEEDS:
        cls, differ = _classify(orc.Scene(os.path.join(SCENES, "cornell_wall.xml"), PARAMS), seed, 256)
        counts = np.bincount(cls, minlength=3)
        print("seed %d: %d pixels all on plain rectangles, %d all on the wall, %d on both; %d pairs with members on different objects" % ((seed,) + tuple(counts) + (int(differ.sum()),)))
        assert (counts > 0).all() and counts.sum() == 256, counts
        assert ((cls == MIXED) & (differ > 0)).any(), "no mixed pixel holds a pair with differing hit objects"
        chosen[seed] = {"static": [], "wall": [], "mixed": [], "split": []}
        order = np.random.default_rng([seed, 5]).permutation(256)
        for want in (STATIC, ALL_WALL, MIXED):
            for p in order[cls[order] == want]:
                crop = (int(p % 16), int(p // 16))
                if _classify(orc.Scene(wall("tent", crop), PARAMS), seed, 1)[0][0] == want:
                    chosen[seed][CLASS_NAMES[want]].append((crop, seed))
                if len(chosen[seed][CLASS_NAMES[want]]) == 2:
                    break
        p = order[(cls[order] == MIXED) & (differ[order] > 0)][0]
        crop = (int(p % 16), int(p // 16))
        osc = orc.Scene(wall("tent", crop), PARAMS)
        splits = lambda s: (lambda c, d: c[0] == MIXED and d[0] > 0)(*_classify(osc, s, 1))
        chosen[seed]["split"] = [(crop, seed)] + [(crop, s) for s in range(64) if s not in SEEDS and splits(s)][:1]
        print("seed %d: crops %s" % (seed, chosen[seed]))
        assert all(len(chosen[seed][k]) == 2 for k in chosen[seed]), chosen[seed]
    return chosen


def test_the_oracle_finds_crops_of_every_class(crops):
    """(no GPU) the three classes are not empty, a mixed pixel with a pair of differing hit objects exists, and crops of each kind exist for both seeds"""
    assert set(crops) == set(SEEDS)


CROP_CASES = [(f, k) for f in ("tent", "tent075") for k in ("static", "wall", "mixed", "split")]


@pytest.mark.gpu
@pytest.mark.parametrize("rfilter,case", CROP_CASES, ids=["%s_%s" % c for c in CROP_CASES])
def test_pair_walk_film_of_a_one_pixel_crop_is_the_generic_fused_film(mi, wall, crops, monkeypatch, rfilter, case):
    for k, v in ps.HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for frame_seed in SEEDS:
        for crop, seed in crops[frame_seed][case]:
            sc = mi.load_file(wall(rfilter, crop), **PARAMS)
            assert sc.size == (1, 1) and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop
            what = (case, rfilter, crop, seed)
            off, on, st = ps._on_and_off(sc, monkeypatch, seed, SPP, what, ps.PAIR_MASK)      # (every statistic of ps.STATS equal, the mask that ran)
            assert sc.last_plan_kernel == 0x52fffff and sc.last_plan_mask == ps.SHAPE_MASK and sc.last_plan_shape == (5, 2), what
            assert np.array_equal(ps.bits(on), ps.bits(off)), (what, on, off)
            print("%s: film bits and statistics equal (n_bounces %d, shadow rays %d)" % (what, st["n_bounces"], st["n_shadow_rays"]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_pair_walk_frame_matches_the_oracle_film(mi, orc, monkeypatch, seed):
    """cornell_wall 16 x 16 x 64 into a device film: one launch of the headline kernel; colour and weight within IMG_TOL of the oracle's film"""
    for k, v in dict(ps.HEADLINE_SHAPE, **{ps.SWITCH: "1"}).items():
        monkeypatch.setenv(k, v)
    path = os.path.join(SCENES, "cornell_wall.xml")
    sc, osc = mi.load_file(path, **PARAMS), orc.Scene(path, PARAMS)
    got, st, kernel = ps._film_frame(sc, seed, SPP)
    assert kernel == ps.PAIR_MASK and st["n_plan_facts_launches"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1 and st["n_paths"] == 256 * SPP, (st, hex(kernel))
    ref = osc.render(osc.params(), seed=seed, spp=SPP, raw=True, threads=ps.NCPU)[0]
    for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
        err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
        print("seed %d, %s: %.3g of the largest value (bound %g)" % (seed, name, err, ps.IMG_TOL))
        assert err <= ps.IMG_TOL, (name, err)


FALLBACKS = [c for c in ps.FALLBACKS if c[0] in ("max_depth_2", "max_depth_3", "max_depth_5", "two_point_lights", "antithetic")]


@pytest.mark.gpu
@pytest.mark.parametrize("fallback", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_a_frame_without_the_fact_keeps_its_kernel_and_bits(mi, wall, crops, monkeypatch, fallback):
    name, params, props, second_light, kernel = fallback
    for k, v in ps.HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    seed = SEEDS[0]
    for rfilter, crop in (("tent", crops[seed]["static"][0][0]), ("tent075", crops[seed]["split"][0][0])):
        sc = mi.load_file(wall(rfilter, crop, props, second_light), resx=16, resy=16, **params)
        off, on, _ = ps._on_and_off(sc, monkeypatch, seed, SPP, (name, rfilter, crop), kernel)
        assert not sc.last_plan_pair_samples and sc.last_plan_kernel == kernel, (name, rfilter, crop)
        assert np.array_equal(ps.bits(on), ps.bits(off)), (name, rfilter, crop, on, off)


@pytest.mark.gpu
def test_crop_cases_on_the_pattern_initialised_build():
    """the crops in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(ps.PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "one_pixel_crop"],
                       env=dict(os.environ, DTOF_LIB=ps.PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
