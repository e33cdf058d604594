"""The scene facts of the headline first-bounce kernels (k_shade's FACTS mask, dtof_kernels.h: kFactFlat, kFactOneWall, kFactFusedSplat) and the shading
frames that come with them, against the generic kernels, which DTOF_PLAN_FACTS=0 restores.

Under the facts every ray query is trace_flat without its instance loop, compute_surface takes the memo branch and reads its shading frames instead of normalising them
(the plain rectangles' from the DFlatFrame table of the blob, the moving wall's from two values computed once per path), and C2's kernel splats with the tent known at
compile time.  Each replaces a launch-uniform decision by a constant or an expression by its own value computed earlier, in the same order: no lane's arithmetic differs.

  1. reproducible films (box filter, the splat kernels): the kernel compiled with kHeadlineFacts gives the bits of the generic one -- cornell_wall 16 x 16 x 64 stratified,
     and 8 x 8 x 256 antithetic_mirror (C3's form), max_depth 1 .. 4; the same cases on the pattern-initialised build;
  2. the fused kernel (kHeadlineFacts | kFactFusedSplat) against the generic kernel's fused film on 1 x 1 crops -- one wave per film pixel, so every film word is one
     atomic add onto zero and the film is reproducible -- under a tent of radius 1 and 0.75, at a frame corner and inside; a 16 x 16 fused frame against the oracle;
  3. each fact broken alone takes a less specific kernel (the counters say which form ran) and the film keeps its bits;
  4. (no GPU) the DFlatFrame table equals the frame restated in numpy float32, in the order of compute_surface, bit for bit.

Frames are launched in the headline's shape (DTOF_CHUNK_SEGS=0: one block per 512-lane segment), as tests/test_plan_facts.py explains."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT, SCENES

IMG_TOL = 5e-5            # tests/test_device_film.py: relative to max|ref|; the lanes are bit-exact, only the float32 order of the film sums differs
NCPU = min(os.cpu_count() or 1, 16)
SWITCH = "DTOF_PLAN_FACTS"
HEADLINE_SHAPE = dict(DTOF_CHUNK_SEGS="0")
PATTERN_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_pattern.so")
STATS = ("n_paths", "n_bounces", "n_shadow_rays", "n_bounces_inline", "n_launches_trace", "n_launches_shade", "n_launches_shadow", "n_launches_first", "n_fused_splat_launches")

WALL_BLOCK = re.compile(r'\t<shape type="rectangle" id="BackWall">.*?</shape>\n', re.S)
PANEL = ('<transform time="0"><scale value="0.3" /><translate x="0.3" y="0.6" z="0.2" /></transform>'
         '<transform time="0.0015"><scale value="0.3" /><translate x="0.3" y="0.6" z="0.21" /></transform>')
TILTED = ('<shape type="rectangle" id="Tilted"><transform name="to_world"><scale x="0.3" y="0.7" z="1" /><rotate x="0.3" y="1" z="0.2" angle="37" />'
          '<translate x="0.2" y="0.9" z="0.1" /></transform><ref id="ShortBoxBSDF" /></shape>')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _variant(xml, rfilter="tent", crop=None, shape=None):
    """cornell_wall.xml with another reconstruction filter, a crop window, or another set of moving objects"""
    assert xml.count('<rfilter type="tent" />') == 1
    xml = xml.replace('<rfilter type="tent" />', {"tent": '<rfilter type="tent" />', "box": '<rfilter type="box" />', "gaussian": '<rfilter type="gaussian" />',
                                                  "tent075": '<rfilter type="tent"><float name="radius" value="0.75" /></rfilter>'}[rfilter])
    if crop is not None:
        assert xml.count('<string name="file_format"') == 1
        xml = xml.replace('<string name="file_format"', '<integer name="crop_offset_x" value="%d" /><integer name="crop_offset_y" value="%d" />'
                          '<integer name="crop_width" value="1" /><integer name="crop_height" value="1" /><string name="file_format"' % crop)
    wall = WALL_BLOCK.search(xml)
    assert wall is not None
    matrix = re.search(r'<matrix value="[^"]*" />', wall.group(0)).group(0)
    if shape == "two_instances":      # a second moving rectangle: no memo object
        xml = xml.replace("\t<emitter", '\t<shape type="rectangle" id="Panel"><animation name="to_world">%s</animation><ref id="ShortBoxBSDF" /></shape>\n\t<emitter' % PANEL, 1)
    elif shape == "two_rectangles":   # the one instance holds the wall and a panel: a general instance of the flat table
        group = ('\t<shape type="shapegroup" id="G"><shape type="rectangle"><transform name="to_world">%s</transform><ref id="BackWallBSDF" /></shape>'
                 '<shape type="rectangle"><transform name="to_world"><scale value="0.3" /><translate x="0.3" y="0.6" z="0.2" /></transform><ref id="ShortBoxBSDF" /></shape></shape>\n'
                 '\t<shape type="instance"><ref id="G" /><animation name="to_world"><transform time="0"><translate x="0" y="0" z="0" /></transform>'
                 '<transform time="0.0015"><translate x="0" y="0" z="0.015" /></transform></animation></shape>\n' % matrix)
        xml = xml.replace(wall.group(0), group)
    elif shape == "no_instance":      # the wall stands still: a plain rectangle
        xml = xml.replace(wall.group(0), '\t<shape type="rectangle" id="BackWall"><transform name="to_world">%s</transform><ref id="BackWallBSDF" /></shape>\n' % matrix)
    elif shape == "tilted":           # one more plain rectangle, rotated about a skew axis and scaled differently along its two sides
        xml = xml.replace("\t<emitter", "\t" + TILTED + "\n\t<emitter", 1)
    else:
        assert shape is None
    return xml


@pytest.fixture(scope="module")
def wall():
    """variants of scenes/cornell_wall.xml written next to it and removed afterwards"""
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(rfilter="tent", crop=None, shape=None):
        key = (rfilter, crop, shape)
        if key not in made:
            made[key] = os.path.join(SCENES, "_flat_facts_%d_%s_%s_%s.xml" % (os.getpid(), rfilter, "x".join(map(str, crop)) if crop else "full", shape))
            open(made[key], "w").write(_variant(base, rfilter, crop, shape))
        return made[key]
    yield get
    for p in made.values():
        os.remove(p)


def _film_frame(sc, seed, spp):
    """one frame into a zeroed device film -> (film as numpy, stats)"""
    import torch
    W, H = sc.size
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    st = sc.render_rows(film.data_ptr(), seed, spp, 0, H)
    return film.cpu().numpy(), st


def _on_and_off(sc, monkeypatch, seed, spp, what, lit=True):
    """the frame with the switch off (twice: the film must be reproducible) and on -> (film off, film on, stats off, stats on); lit = False: a frame whose paths gather
    nothing and that launches no bounce kernel (max_depth = 1)"""
    monkeypatch.setenv(SWITCH, "0")
    off_a, st_off = _film_frame(sc, seed, spp)
    off_b, _ = _film_frame(sc, seed, spp)
    assert np.isfinite(off_a).all() and (np.abs(off_a[..., :3]).max() > 0) == lit and (off_a[..., 3] > 0).all(), what
    assert np.array_equal(bits(off_a), bits(off_b)), (what, "the film chosen as reproducible is not", int((bits(off_a) != bits(off_b)).sum()))
    assert st_off["n_plan_facts_launches"] == 0 and st_off["n_launches_first"] == (1 if lit else 0), (what, st_off)
    monkeypatch.setenv(SWITCH, "1")
    on, st_on = _film_frame(sc, seed, spp)
    for k in STATS:
        assert st_on[k] == st_off[k], (what, k, st_on[k], st_off[k])
    return off_a, on, st_off, st_on


# ---------------------------------------------------------------------------- without a GPU
def _fma(a, b, c):
    """fmaf on float32 values: the exact a * b + c, rounded once to the nearest float32 (ties to even)"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))   # (keeps the sign of a zero; exact)
    r = np.float32(float(exact))
    cands = sorted({r, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))}, key=float)
    best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(np.float32(x).view(np.uint32)) & 1))
    return np.float32(best)


def _dot(a, b):
    return _fma(a[2], b[2], _fma(a[1], b[1], np.float32(a[0] * b[0])))


def _frame(n, dp_du):
    """initialize_sh_frame as compute_surface (dtof_shading.h) evaluates it for a plain rectangle, sh_n = n: s = normalize(fma(n, -dot(n, dp_du), dp_du)), t = cross(n, s);
    normalize(v) = v * sqrt(1 / dot(v, v)).  Multiplication, division and square root of numpy float32 are the IEEE operations."""
    n, dp_du = np.asarray(n, np.float32), np.asarray(dp_du, np.float32)
    k = np.float32(-_dot(n, dp_du))
    v = np.array([_fma(n[i], k, dp_du[i]) for i in range(3)], np.float32)
    r = np.sqrt(np.float32(1.0) / _dot(v, v))
    s = (v * r).astype(np.float32)
    t = np.array([_fma(n[1], s[2], -np.float32(n[2] * s[1])), _fma(n[2], s[0], -np.float32(n[0] * s[2])), _fma(n[0], s[1], -np.float32(n[1] * s[0]))], np.float32)
    return s, t


def test_host_frames_are_the_frames_compute_surface_builds(mi, wall):
    """DFlatFrame of every plain rectangle of cornell_wall and of a rotated, non-uniformly scaled one: all six words decided by the restatement, so all six compared as
    bit patterns; the moving wall's record is zero (its frame depends on the ray time).  No rectangle here has dp_du == 0: that fallback (coordinate_system) is not restated."""
    sc = mi.load_file(wall(shape="tilted"))
    rec = sc.export(25).reshape(-1, 13)
    assert rec.shape[0] == 6 and sorted(rec[:, 0]) == [0, 0, 0, 0, 0, 2]
    for r in rec:
        mark, n, dp_du, s, t = r[0], r[1:4], r[4:7], r[7:10], r[10:13]
        if mark != 0:
            assert not bits(r[7:13]).any()
            continue
        assert np.abs(dp_du).max() > 0
        rs, rt = _frame(n, dp_du)
        assert np.array_equal(bits(s), bits(rs)) and np.array_equal(bits(t), bits(rt)), (n, dp_du, s, rs, t, rt)
        assert abs(float(np.dot(s, s)) - 1) < 1e-6 and abs(float(np.dot(s, n))) < 1e-6 and abs(float(np.dot(t, n))) < 1e-6
    tilted = rec[5]
    assert np.count_nonzero(np.abs(tilted[7:10]) > 1e-3) == 3, "the added rectangle's tangent has no zero component"
    assert mi.load_file(os.path.join(SCENES, "cornell_boxes.xml")).export(25).size == 0   # a scene without the flat table exports nothing


def test_the_masks():
    """kHeadlineFacts carries Flat and OneWall on top of the ten facts of the frame plan; which instantiation ran is what the GPU cases below read from the counters"""
    hdr = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "dtof_kernels.h")).read()
    bit = {m.group(1): int(m.group(2)) for m in re.finditer(r"(kFact\w+)\s*=\s*1u << (\d+)", hdr)}
    assert (bit["kFactFlat"], bit["kFactOneWall"], bit["kFactFusedSplat"]) == (10, 11, 12)
    assert int(re.search(r"#define DTOF_HEADLINE_FACTS (0x[0-9a-f]+)", hdr).group(1), 16) == 0xfff


# ---------------------------------------------------------------------------- 1. reproducible films
REPRODUCIBLE = [("stratified_depth%d" % d, dict(resx=16, resy=16, max_depth=d), 64) for d in (1, 2, 3, 4)]
REPRODUCIBLE += [("mirror_256_depth%d" % d, dict(resx=8, resy=8, max_depth=d, time_sampling_method="antithetic_mirror"), 256) for d in (1, 2, 3, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,params,spp", REPRODUCIBLE, ids=[c[0] for c in REPRODUCIBLE])
def test_reproducible_film_is_the_same_bits_with_and_without_the_scene_facts(mi, wall, monkeypatch, name, params, spp):
    for k, v in dict(HEADLINE_SHAPE, DTOF_FUSE_SPLAT="0").items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(wall("box"), **params)
    # (max_depth = 1: no vertex of a path is shaded -- a scene lit by a point light gathers nothing there, so no bounce kernel is launched at all and the film is its weights)
    lit = params["max_depth"] > 1
    off, on, _, st_on = _on_and_off(sc, monkeypatch, 3, spp, name, lit=lit)
    assert st_on["n_plan_facts_launches"] == (1 if lit else 0) and st_on["n_fused_splat_launches"] == 0, st_on      # the kernel of kHeadlineFacts ran
    assert np.array_equal(bits(on), bits(off)), (name, int((bits(on) != bits(off)).sum()), float(np.abs(on - off).max()))


# ---------------------------------------------------------------------------- 2. the fused kernel
CROPS = [("r1_corner_0_0", "tent", (0, 0)), ("r1_corner_15_15", "tent", (15, 15)), ("r1_inside_5_9", "tent", (5, 9)), ("r1_edge_15_3", "tent", (15, 3)),
         ("r075_corner_0_15", "tent075", (0, 15)), ("r075_inside_8_2", "tent075", (8, 2)), ("r075_inside_11_12", "tent075", (11, 12))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,rfilter,crop", CROPS, ids=[c[0] for c in CROPS])
def test_fused_kernel_film_of_a_one_pixel_crop_is_the_generic_fused_film(mi, wall, monkeypatch, name, rfilter, crop):
    """a 1 x 1 crop of the 16 x 16 frame at 64 spp is ONE wave: the film's four words each receive one atomic add of the wave's reduction (the taps outside the crop are
    dropped), so the fused film is reproducible, and the kernel with every fact must give the generic fused kernel's bits"""
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(wall(rfilter, crop), resx=16, resy=16)
    assert sc.size == (1, 1) and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop
    off, on, st_off, st_on = _on_and_off(sc, monkeypatch, 4, 64, name)
    assert st_off["n_fused_splat_launches"] == 1 and st_on["n_fused_splat_launches"] == 1 and st_on["n_plan_facts_launches"] == 1 and st_on["n_paths"] == 64, (st_off, st_on)
    assert np.array_equal(bits(on), bits(off)), (name, on, off)


@pytest.mark.gpu
def test_fused_kernel_frame_matches_the_oracle_film(mi, orc, monkeypatch):
    """cornell_wall 16 x 16 x 64 with the tent filter into a device film: one launch of the fused kernel; colour and weight within IMG_TOL of the oracle's film, the bound
    tests/test_plan_facts.py and tests/test_device_film.py hold the fused splat to"""
    for k, v in dict(HEADLINE_SHAPE, **{SWITCH: "1"}).items():
        monkeypatch.setenv(k, v)
    path, params, spp = os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16), 64
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    got, st = _film_frame(sc, 5, spp)
    assert st["n_plan_facts_launches"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1 and st["n_paths"] == 16 * 16 * spp, st
    ref = osc.render(osc.params(), seed=5, spp=spp, raw=True, threads=NCPU)[0]
    for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
        err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
        print("fused kernel, %s: %.3g of the largest value (bound %g)" % (name, err, IMG_TOL))
        assert err <= IMG_TOL, (name, err)


# ---------------------------------------------------------------------------- 3. each fact broken alone
# (id, filter, scene variant, spp, environment, specialised launches expected with the switch on, fused splat launches expected)
BROKEN = [
    ("two_instances", "box", "two_instances", 64, {}, 0, 0),
    ("instance_of_two_rectangles", "box", "two_rectangles", 64, {}, 0, 0),
    ("no_instance", "box", "no_instance", 64, {}, 0, 0),
    ("flat_off", "box", None, 64, dict(DTOF_FLAT="0"), 0, 0),
    ("instance_memo_off", "box", None, 64, dict(DTOF_INSTANCE_MEMO="0"), 0, 0),
    ("spp_32", "box", None, 32, {}, 0, 0),
    # no fused splat: the kernel of kHeadlineFacts, which leaves the film to the splat kernels, instead of C2's
    ("gaussian_filter", "gaussian", None, 64, {}, 1, 0),
    ("spp_32_tent", "tent", None, 32, {}, 0, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BROKEN, ids=[c[0] for c in BROKEN])
def test_a_scene_that_breaks_one_fact_takes_a_less_specific_kernel(mi, wall, monkeypatch, case):
    name, rfilter, shape, spp, env, n_special, n_fused = case
    for k, v in dict(dict(HEADLINE_SHAPE, DTOF_FUSE_SPLAT="0") if rfilter == "box" else HEADLINE_SHAPE, **env).items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(wall(rfilter, None, shape), resx=16, resy=16)
    before = sc.plan_facts_launches
    monkeypatch.setenv(SWITCH, "0")
    off_a, st_off = _film_frame(sc, 6, spp)
    off_b, _ = _film_frame(sc, 6, spp)
    assert sc.plan_facts_launches == before and st_off["n_plan_facts_launches"] == 0, (name, st_off)
    monkeypatch.setenv(SWITCH, "1")
    on, st_on = _film_frame(sc, 6, spp)
    assert st_on["n_plan_facts_launches"] == n_special and sc.plan_facts_launches == before + n_special and st_on["n_launches_first"] == 1, (name, st_on)
    assert st_on["n_fused_splat_launches"] == n_fused == st_off["n_fused_splat_launches"], (name, st_on)
    for k in STATS:
        assert st_on[k] == st_off[k], (name, k, st_on[k], st_off[k])
    assert np.isfinite(on).all() and np.abs(on[..., :3]).max() > 0, name
    if rfilter == "box":
        assert np.array_equal(bits(off_a), bits(off_b)), (name, "the film chosen as reproducible is not")
    if np.array_equal(bits(off_a), bits(off_b)):       # a reproducible film: the same bits with the switch in either position
        assert np.array_equal(bits(on), bits(off_a)), (name, int((bits(on) != bits(off_a)).sum()))
    else:                                              # the splat kernel's atomics land in no fixed order: the same lanes, summed in another order
        for ch in (slice(0, 3), 3):
            assert float(np.abs(on[..., ch] - off_a[..., ch]).max() / np.abs(off_a[..., ch]).max()) <= IMG_TOL, (name, ch)


# ---------------------------------------------------------------------------- the pattern-initialised build
@pytest.mark.gpu
def test_core_cases_on_the_pattern_initialised_build():
    """the reproducible films and the fused kernel's crops in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "reproducible or one_pixel_crop"],
                       env=dict(os.environ, DTOF_LIB=PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
