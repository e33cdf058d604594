"""The z rows of the four plain rectangles on the matrix cores (mitsuba3dopplertof_amd/csrc/dtof_zrow_mfma.h; trace_flat: ZROW): under the table shape
of the headline frame -- five rectangles, the wall at index 2 -- a vertex's shadow and continuation queries take the local z of their ray in rectangles 0, 1, 3, 4 from
six v_mfma_f32_4x4x1 issued by every lane of the wave in front of the query, instead of four LDS rows and 24 multiply-adds.  The premise is that a 4x4x1 f32 MFMA chain
is the fmaf chain of flat_zrow in every bit; nothing here takes that on trust.

  1. (no GPU) dtof_flat_query_zrow exists in the header, the library and the binding's table, and refuses what it is not compiled for before a device is touched;
  2. the eight MFMA words of every ray of the sweeps of `closed`, `panel` and `ties_wall` (tests/flat_sweep.py: families A to M, X, HT) against the oracle's ZX / ZY
     operands of rectangles 0, 1, 3, 4, bit for bit -- signed zeros, the denormal directions of E, the 1e30 / 1e38 lengths of D2; a NaN where the oracle has one;
  3. dtof_flat_query_zrow against form 0 of dtof_flat_query (which tests/test_flat_sweep_gpu.py holds to the oracle), ids and all three words, both query kinds: in
     family order, under the sweep's fixed permutation, and in the short lists of 1, 63, 64 and 65 rays -- partial waves, whose lanes behind the end of the list take
     part in the MFMAs and store nothing;
  4. films of the headline kernel, which runs the form at every vertex: 1 x 1 crops of cornell_wall 16 x 16 x 64 at max_depth 4 the oracle puts all on plain
     rectangles, all on the wall and on both (tests/test_pair_walk.py chooses them) against DTOF_PLAN_FACTS=0 -- film bits, statistics, the mask that ran; the
     16 x 16 frames at seeds 4 and 11 (paths leave through the open front and their lanes sit out later iterations) with the statistics of DTOF_PLAN_FACTS=0 and
     within IMG_TOL of its film and of the oracle's -- a frame's film is not reproducible to the bit by ANY kernel, the generic one included (float atomics of
     several waves per cell), so its bits cannot be held; `wall_at_3` and `six` keep their kernels and films; the crops, the frames and one query on the
     pattern-initialised library."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import flat_sweep as fs
import test_flat_shape as fsh
import test_pair_samples as ps
from conftest import ROOT, SCENES
from test_pair_walk import crops, wall  # noqa: F401  (fixtures: the oracle's choice of crops, the scene variants they are rendered from)

INVALID = 1
ZROW_SCENES = ("closed", "panel", "ties_wall")
PLAIN = (0, 1, 3, 4)          # the rectangle of each of the four slots
FAMILIES = {"A", "A2", "B", "C", "C2", "D", "D2", "S", "E", "G", "H", "HT", "X", "M"}
SEEDS = (4, 11)
SPP = 64
PARAMS = dict(resx=16, resy=16, max_depth=4)


def _zrow_query(mi, scene, any_hit, rays, n=None, zrows=True):
    """dtof_flat_query_zrow into buffers pre-filled with the sweep's canary -> (return code, (n, 3) words or None, ids, (n, 8) z-row words or None)"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    out, ids, z = np.full((len(rays), 3), fs.CANARY, np.uint32), np.full(len(rays), fs.CANARY, np.uint32), np.full((len(rays), 8), fs.CANARY, np.uint32)
    rc = mi._lib().dtof_flat_query_zrow(scene._h, 1 if any_hit else 0, len(rays) if n is None else n, rays.ctypes.data, None if any_hit else out.ctypes.data, ids.ctypes.data,
                                        z.ctypes.data if zrows else None)
    return rc, (None if any_hit else out), ids.view(np.int32), (z if zrows else None)


# ---------------------------------------------------------------------------- 1. without a GPU
def test_entry_is_declared_and_refuses_other_tables_on_the_host(mi):
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    decl = re.search(r"\bint\s+dtof_flat_query_zrow\s*\(([^;]*)\)\s*;", hdr)
    assert decl and [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")] == ["scene", "any", "n", "rays8", "out3", "ids", "zrow8"]
    assert hasattr(C.CDLL(mi.lib_path()), "dtof_flat_query_zrow")
    lib = mi._lib()
    rays = np.zeros((4, 8), np.float32)
    rays[:, 5], rays[:, 7] = 1.0, 10.0
    for name, reason in (("wall_at_3", "5 rectangles"), ("six", "5 rectangles"), ("no_instance", "5 rectangles")):
        sc = mi.load_string(fs.scene_xml(name), resx=16, resy=16)
        for any_hit in (0, 1):
            rc, out, ids, z = _zrow_query(mi, sc, any_hit, rays)
            msg = lib.dtof_last_error().decode()
            assert rc == INVALID and reason in msg and msg.startswith("dtof_flat_query_zrow"), (name, rc, msg)
            assert (ids.view(np.uint32) == fs.CANARY).all() and (z == fs.CANARY).all() and (out is None or (out == fs.CANARY).all()), name
        with pytest.raises(mi.DtofError):
            sc.flat_query_zrow(rays)
    closed = mi.load_string(fs.scene_xml("closed"), resx=16, resy=16)
    ids = np.zeros(4, np.int32)
    assert lib.dtof_flat_query_zrow(closed._h, 0, 4, None, ids.ctypes.data, ids.ctypes.data, None) == INVALID        # null rays
    assert lib.dtof_flat_query_zrow(closed._h, 0, 4, rays.ctypes.data, None, ids.ctypes.data, None) == INVALID        # closest hit without out3
    assert lib.dtof_flat_query_zrow(closed._h, 1, 4, rays.ctypes.data, None, None, None) == INVALID                   # no ids
    assert lib.dtof_flat_query_zrow(closed._h, 0, (1 << 24) + 1, rays.ctypes.data, ids.ctypes.data, ids.ctypes.data, None) == INVALID


# ---------------------------------------------------------------------------- 2. and 3. the z rows and the query
@pytest.fixture(scope="module")
def swept(mi, orc):
    """name -> (sweep, device scene); the last scene is kept"""
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            sw = fs.Sweep(name, orc)
            assert list(sw.want["rect_obj"]) == [0, 1, 2, 3, 4] and FAMILIES <= set(sw.family), sorted(set(sw.family))
            cache[name] = (sw, mi.load_string(sw.xml, resx=16, resy=16))
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ZROW_SCENES)
def test_mfma_z_rows_are_the_fmaf_chains_bit_for_bit(mi, swept, name):
    """THE test of the premise: a chain of three 4x4x1 f32 MFMAs is fmaf(z2, c, fmaf(z1, b, fmaf(z0, a, z3))), and with C = -0.0 its first link is the product z0 * a"""
    sw, scene = swept(name)
    rc, _, ids, z = _zrow_query(mi, scene, 0, sw.rays)
    assert rc == 0, mi._lib().dtof_last_error().decode("utf-8", "replace")
    assert int((z == fs.CANARY).sum()) == 0
    ops = sw.want["ops"]
    want = np.concatenate([ops[:, PLAIN, fs.ZX], ops[:, PLAIN, fs.ZY]], axis=1).astype(np.float32)
    got = z.view(np.float32)
    nan = np.isnan(want)
    differ = np.where(nan, ~np.isnan(got), z != want.view(np.uint32))
    rows = np.flatnonzero(differ.any(axis=1))
    finite = np.isfinite(sw.rays[:, :6]).all(axis=1)
    tiny = (np.abs(want) < np.finfo(np.float32).tiny) & (want != 0)
    print("%s: %d rays, %d of their 8 z-row words differ from the oracle's operands (%d on finite rays); %d words are NaN, %d +-0 (%d of them -0), %d denormal, %d beyond 1e30"
          % (name, sw.n, int(differ.sum()), int(differ[finite].sum()), int(nan.sum()), int((want == 0).sum()), int(((want == 0) & np.signbit(want)).sum()), int(tiny.sum()),
             int((np.abs(want[~nan]) > 1e30).sum())))
    for i in rows[:6]:
        print("  ray %d, family %s: %s\n    device %s\n    oracle %s" % (i, sw.family[i], sw.rays[i].tolist(), ["%08x" % w for w in z[i]], ["%08x" % w for w in want[i].view(np.uint32)]))
    # the sweep holds what the case is about
    assert nan.sum() > 0 and ((want == 0) & np.signbit(want)).sum() > 0 and ((want == 0) & ~np.signbit(want)).sum() > 0 and tiny.sum() > 0
    assert len(rows) == 0, "%s: %d rays differ, by family %s" % (name, len(rows), dict(zip(*np.unique(sw.family[rows], return_counts=True))))
    # ... and the Python entry hands out the same words
    r, zz = scene.flat_query_zrow(sw.rays[:4096], zrows=True)
    assert np.array_equal(zz.view(np.uint32), z[:4096]) and np.array_equal(r["obj"], ids[:4096])
    assert np.array_equal(scene.flat_query_zrow(sw.rays[:4096], any=True), _zrow_query(mi, scene, 1, sw.rays[:4096], zrows=False)[2])
    assert len(scene.flat_query_zrow(sw.rays[:0])["t"]) == 0


def _answers(mi, scene, any_hit, rays, what):
    """(zrow form, form 0) of the same rays, each (words or None, ids); both calls must succeed and write every word"""
    got = []
    for label, (rc, out, ids) in (("zrow", _zrow_query(mi, scene, any_hit, rays, zrows=False)[:3]), ("form 0", fs.device_query(mi, scene, 0, any_hit, rays))):
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


def _report(sw, rows, idx, a, b, what):
    lines = ["%s: %d rays differ" % (what, len(rows))]
    for i in rows[:6]:
        show = lambda ans: "ids %d" % ans[1][i] if ans[0] is None else "obj %d t u v %s" % (int(ans[1][i]), ans[0][i].view(np.float32).tolist())
        lines.append("  ray %d (lane %d of its wave), family %s: %s\n    zrow form %s   form 0 %s" % (i, i % 64, sw.family[idx[i]], sw.rays[idx[i]].tolist(), show(a), show(b)))
    return "\n".join(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [(n, k) for n in ZROW_SCENES for k in fs.KINDS], ids=["%s-%s" % (n, k) for n in ZROW_SCENES for k in fs.KINDS])
def test_zrow_form_answers_what_the_generic_walk_answers(mi, swept, name, kind):
    sw, scene = swept(name)
    any_hit = fs.KINDS.index(kind)
    what = "%s, %s" % (name, kind)
    order = np.arange(sw.n)
    got, ref = _answers(mi, scene, any_hit, sw.rays, what + ", in family order")
    rows = _differing(got, ref)
    print("%s: %d rays, %d differ from form 0 in family order" % (what, sw.n, len(rows)))
    assert len(rows) == 0, _report(sw, rows, order, got, ref, what + ", in family order")
    hit = ref[1] == 1 if any_hit else ref[1] >= 0
    # (ties_wall's second floor, object 3, loses every tie to the first: four objects are hit there, five elsewhere)
    assert 0.05 < hit.mean() < 0.95 and (any_hit or {-1, 2} < set(np.unique(ref[1])) and len(np.unique(ref[1])) >= 5), (what, float(hit.mean()), np.unique(ref[1]))
    # the fixed permutation: mixed waves
    mixed, mixed_ref = _answers(mi, scene, any_hit, sw.rays[sw.perm], what + ", permuted")
    rows = _differing(mixed, mixed_ref)
    assert len(rows) == 0, _report(sw, rows, sw.perm, mixed, mixed_ref, what + ", permuted")
    rows = _differing(mixed, (None if any_hit else ref[0][sw.perm], ref[1][sw.perm]))
    assert len(rows) == 0, _report(sw, rows, sw.perm, mixed, ref, what + ": permuted against in order")
    # the short lists of 1, 63, 64 and 65 rays: the last wave is partial, its lanes behind the list run the MFMAs on zeros
    sizes = set()
    for label, idx in sw.short.items():
        short, short_ref = _answers(mi, scene, any_hit, sw.rays[idx], "%s, %s" % (what, label))
        bad = _differing(short, short_ref)
        assert len(bad) == 0, _report(sw, bad, idx, short, short_ref, "%s, %s" % (what, label))
        assert len(_differing(short, (None if any_hit else ref[0][idx], ref[1][idx]))) == 0, (what, label)
        sizes.add(len(idx))
    assert sizes >= {1, 63, 64, 65}
    # ... and with the z rows asked for, a partial wave writes the rows of its own rays only
    idx = next(i for i in sw.short.values() if len(i) == 65)
    rc, _, _, z = _zrow_query(mi, scene, any_hit, np.concatenate([sw.rays[idx], sw.rays[idx[:7]]]), n=65)
    assert rc == 0 and (z[:65] != fs.CANARY).all() and (z[65:] == fs.CANARY).all()
    print("%s: in order, permuted and %d short lists agree with form 0" % (what, len(sw.short)))


# ---------------------------------------------------------------------------- 4. films
CROP_CASES = [(f, k) for f in ("tent", "tent075") for k in ("static", "wall", "mixed")]


@pytest.mark.gpu
@pytest.mark.parametrize("rfilter,case", CROP_CASES, ids=["%s_%s" % c for c in CROP_CASES])
def test_zrow_film_of_a_one_pixel_crop_is_the_generic_fused_film(mi, wall, crops, monkeypatch, rfilter, case):  # noqa: F811
    for k, v in ps.HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for frame_seed in SEEDS:
        for crop, seed in crops[frame_seed][case]:
            sc = mi.load_file(wall(rfilter, crop), **PARAMS)
            assert sc.size == (1, 1) and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop
            what = (case, rfilter, crop, seed)
            off, on, st = ps._on_and_off(sc, monkeypatch, seed, SPP, what, ps.PAIR_MASK)      # (every statistic of ps.STATS equal, the mask that ran)
            assert sc.last_plan_kernel == ps.PAIR_MASK and sc.last_plan_shape == (5, 2), what
            assert np.array_equal(ps.bits(on), ps.bits(off)), (what, on, off)
            print("%s: film bits and statistics equal (n_bounces %d, shadow rays %d)" % (what, st["n_bounces"], st["n_shadow_rays"]))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_zrow_frame_is_the_generic_fused_film_and_matches_the_oracle(mi, orc, monkeypatch, seed):
    """cornell_wall 16 x 16 x 64 at max_depth 4 into a device film: one launch of the headline kernel with the statistics of the generic fused kernel's frame, and
    colour and weight within IMG_TOL of that frame's film and of the oracle's.  Paths leave the room through its open front: fewer lanes enter iteration 1 and 2
    than paths start.
    The frame's film cannot be held to bits: a film cell of a frame takes one float atomic from each of up to nine waves, in the order they arrive, and two frames of
    the SAME kernel differ (the generic kernel against itself at seed 4: 222 of the 1 024 words).  The lanes are bit-exact and only the order of the film sums
    differs, which is what IMG_TOL bounds everywhere in the suite; the bits are held on the one-pixel crops above, whose cells take one wave's atomics."""
    for k, v in ps.HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    path = os.path.join(SCENES, "cornell_wall.xml")
    sc, osc = mi.load_file(path, **PARAMS), orc.Scene(path, PARAMS)
    monkeypatch.setenv(ps.SWITCH, "0")
    off, st_off, k_off = ps._film_frame(sc, seed, SPP)
    monkeypatch.setenv(ps.SWITCH, "1")
    on, st, k_on = ps._film_frame(sc, seed, SPP)
    assert k_off == 0 and st_off["n_plan_facts_launches"] == 0 and k_on == ps.PAIR_MASK and st["n_plan_facts_launches"] == 1 and sc.last_plan_shape == (5, 2), (hex(k_off), hex(k_on))
    for k in ps.STATS:
        assert st[k] == st_off[k], (seed, k, st[k], st_off[k])
    assert st["n_launches_shade"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_paths"] == 256 * SPP, st
    assert st["n_paths"] < st["n_bounces"] < 3 * st["n_paths"], st      # some lanes sit out later iterations
    assert np.isfinite(off).all() and np.abs(off[..., :3]).max() > 0 and (off[..., 3] > 0).all()
    ref = osc.render(osc.params(), seed=seed, spp=SPP, raw=True, threads=ps.NCPU)[0]
    for other, against in ((np.asarray(off, np.float64), "the generic fused kernel's film"), (ref, "the oracle's film")):
        for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
            err = float(np.abs(np.asarray(on[..., ch], np.float64) - other[..., ch]).max() / max(np.abs(other[..., ch]).max(), 1e-30))
            print("seed %d, %s against %s: %.3g of the largest value (bound %g); %d words differ" % (seed, name, against, err, ps.IMG_TOL, int((ps.bits(on) != ps.bits(off)).sum())))
            assert err <= ps.IMG_TOL, (against, name, err)


@pytest.fixture(scope="module")
def rooms():
    """test_flat_shape's scene variants (another set of rectangles), written next to cornell_wall.xml and removed afterwards"""
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(rfilter, crop, room):
        if (rfilter, crop, room) not in made:
            made[(rfilter, crop, room)] = os.path.join(SCENES, "_zrow_mfma_%d_%d.xml" % (os.getpid(), len(made)))
            open(made[(rfilter, crop, room)], "w").write(fsh._variant(base, rfilter, crop, room))
        return made[(rfilter, crop, room)]
    yield get
    for p in made.values():
        os.remove(p)


@pytest.mark.gpu
@pytest.mark.parametrize("room", ["six", "wall_at_3"])
def test_a_table_of_another_shape_keeps_its_kernel_and_film(mi, rooms, monkeypatch, room):
    for k, v in ps.HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for rfilter, crop in (("tent", (5, 9)), ("tent075", (0, 0))):      # (one-pixel crops: their films are reproducible to the bit)
        sc = mi.load_file(rooms(rfilter, crop, room), **PARAMS)
        monkeypatch.setenv(ps.SWITCH, "0")
        off, st_off, k_off = ps._film_frame(sc, 6, SPP)
        monkeypatch.setenv(ps.SWITCH, "1")
        on, st_on, k_on = ps._film_frame(sc, 6, SPP)
        what = (room, rfilter, crop, hex(k_on))
        assert k_off == 0 and sc.last_plan_shape is None, what
        assert not (k_on & 1 << ps.FACT_BIT["kFactFlatShape"]) and k_on not in (ps.SHAPE_MASK, ps.PAIR_MASK), what
        assert np.isfinite(off).all() and np.abs(off[..., :3]).max() > 0 and np.array_equal(ps.bits(on), ps.bits(off)), what
        for k in ps.STATS:
            assert st_on[k] == st_off[k], (what, k)


@pytest.mark.gpu
def test_films_and_one_query_on_the_pattern_initialised_build():
    """the crops, the frames and one sweep's query in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(ps.PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "one_pixel_crop or zrow_frame or (generic_walk and closed)"],
                       env=dict(os.environ, DTOF_LIB=ps.PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
