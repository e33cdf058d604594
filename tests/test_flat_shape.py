"""The shape fact of C2's first-bounce kernel (k_shade's FACTS mask, dtof_kernels.h: kFactFlatShape with the table's object count and the wall's index as two fields;
DESIGN 8.3 (i)) against the generic kernels, which DTOF_PLAN_FACTS=0 restores.

Under the shape trace_flat walks cornell_wall's table of five rectangles, the wall at index 2, in straight-line code: an occlusion query is one sweep over the five z rows
and certain-miss tests and ONE branch, behind which a tail runs the full tests of the rectangles some lane still needs; a closest-hit query is the five visits written out
in ascending order.  Every z row, certain-miss test and rectangle test keeps its operations in their order, so the films must keep their bits.

  1. the kernel of kHeadlineShapeFacts (kHeadlineC2Facts and the shape) against the generic fused kernel on 1 x 1 crops of cornell_wall 16 x 16 x 64 -- ONE wave per film, so every film
     word is one atomic add onto zero and the film is reproducible (tests/test_flat_facts.py) -- in a corner, on an edge and in the middle, under a tent of radius 1 and
     0.75, max_depth 2, 3 and 4, two seeds; dtof_scene_last_plan_facts carries the shape bit;
  2. the tail: a room of the same shape in which the left wall is a free-standing panel in front of the back wall, so that shadow rays of second path vertices (the light
     sits at the camera: no first vertex is shadowed) cross its plane and some hit it.  Same bits as the generic kernel, and on the stats build
     (make -C mitsuba3dopplertof_amd/csrc stats, part of build()) the occlusion queries of those crops count full tests (slot 19 of dtof_traverse.h, counted in the tail
     only) while the closed room counts none;
  3. a room with a sixth rectangle, and one with the wall at index 3, take the kernel without the shape (mask 0x3ffff) and keep the bits of the switch-off film;
  4. a 16 x 16 x 64 frame through the new kernel against the oracle's film;
  5. the crops of 1 and 2 on the pattern-initialised library, in a child process;
  6. (no GPU) the fields a frame plan fills: 5 and 2 for cornell_wall, 6 / 2 and 5 / 3 for the rooms of 3, none for cornell_boxes.

Frames are launched in the headline's shape (DTOF_CHUNK_SEGS=0: one block per 512-lane segment), as tests/test_plan_facts.py explains."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

IMG_TOL = 5e-5            # tests/test_sampling_facts.py, tests/test_device_film.py: relative to max|ref|; the lanes are bit-exact, only the float32 order of the film sums differs
NCPU = min(os.cpu_count() or 1, 16)
SWITCH = "DTOF_PLAN_FACTS"
HEADLINE_SHAPE = dict(DTOF_CHUNK_SEGS="0")
CSRC = os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc")
PATTERN_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_pattern.so")
STATS_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_stats.so")
STATS = ("n_paths", "n_bounces", "n_shadow_rays", "n_bounces_inline", "n_launches_trace", "n_launches_shade", "n_launches_shadow", "n_launches_first", "n_fused_splat_launches")
SHAPE_BLOCK = r'\t<shape type="rectangle" id="%s">.*?</shape>\n'
# a rectangle of side 0.6 that faces the camera, in front of the back wall (z = -1) and above the floor: what lies behind it sees no light
PANEL = ('\t<shape type="rectangle" id="LeftWall">\n\t\t<transform name="to_world"><scale value="0.3" /><translate x="0.3" y="0.6" z="0.2" /></transform>\n'
         '\t\t<ref id="LeftWallBSDF" />\n\t</shape>\n')
SIXTH = ('\t<shape type="rectangle" id="Tilted"><transform name="to_world"><scale x="0.3" y="0.7" z="1" /><rotate x="0.3" y="1" z="0.2" angle="37" />'
         '<translate x="0.2" y="0.9" z="0.1" /></transform><ref id="ShortBoxBSDF" /></shape>\n')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _masks():
    """(the mask of the shaped kernel, kHeadlineC2Facts = the same without the shape fields, the shape fields of cornell_wall, all fields) as dtof_kernels.h defines them"""
    hdr = open(os.path.join(CSRC, "dtof_kernels.h")).read()
    bit = {m.group(1): int(m.group(2)) for m in re.finditer(r"(kFact\w+)\s*=\s*1u << (\d+)", hdr)}
    count_shift, wall_shift = (int(re.search(r"%s = (\d+)" % k, hdr).group(1)) for k in ("kFlatShapeCountShift", "kFlatShapeWallShift"))
    count, wall = (int(re.search(r"#define DTOF_HEADLINE_SHAPE_%s (\d+)" % k, hdr).group(1)) for k in ("COUNT", "WALL"))
    headline = int(re.search(r"#define DTOF_HEADLINE_FACTS (0x[0-9a-f]+)", hdr).group(1), 16) | 1 << bit["kFactFusedSplat"]
    c2 = headline | int(re.search(r"#define DTOF_HEADLINE_C2 (0x[0-9a-f]+)", hdr).group(1), 16)
    shape = 1 << bit["kFactFlatShape"] | count << count_shift | wall << wall_shift
    return c2 | shape, c2, shape, 1 << bit["kFactFlatShape"] | 0xf << count_shift | 0x7 << wall_shift, bit


SHAPE_MASK, ROUTE_MASK, SHAPE_5_2, SHAPE_FIELDS, FACT_BIT = _masks()


def _variant(xml, rfilter, crop, room):
    """cornell_wall.xml with another tent radius, a 1 x 1 crop window and another set of rectangles"""
    assert xml.count('<rfilter type="tent" />') == 1 and xml.count('<string name="file_format"') == 1
    xml = xml.replace('<rfilter type="tent" />', {"tent": '<rfilter type="tent" />', "tent075": '<rfilter type="tent"><float name="radius" value="0.75" /></rfilter>'}[rfilter])
    if crop is not None:
        xml = xml.replace('<string name="file_format"', '<integer name="crop_offset_x" value="%d" /><integer name="crop_offset_y" value="%d" />'
                          '<integer name="crop_width" value="1" /><integer name="crop_height" value="1" /><string name="file_format"' % crop)
    block = {k: re.search(SHAPE_BLOCK % k, xml, re.S) for k in ("BackWall", "RightWall", "LeftWall")}
    assert all(b is not None for b in block.values())
    if room == "panel":          # five rectangles, the instance at index 2; the left wall is a panel inside the room
        xml = xml.replace(block["LeftWall"].group(0), PANEL)
    elif room == "six":          # one more plain rectangle behind the five
        xml = xml.replace("\t<emitter", SIXTH + "\t<emitter", 1)
    elif room == "wall_at_3":    # the moving wall behind the right wall: five rectangles, the instance at index 3
        xml = xml.replace(block["BackWall"].group(0), "").replace(block["RightWall"].group(0), block["RightWall"].group(0) + block["BackWall"].group(0))
    else:
        assert room == "closed"
    return xml


@pytest.fixture(scope="module")
def wall():
    """variants of scenes/cornell_wall.xml written next to it and removed afterwards"""
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(rfilter="tent", crop=None, room="closed"):
        key = (rfilter, crop, room)
        if key not in made:
            made[key] = os.path.join(SCENES, "_flat_shape_%d_%d.xml" % (os.getpid(), len(made)))
            open(made[key], "w").write(_variant(base, rfilter, crop, room))
        return made[key]
    yield get
    for p in made.values():
        os.remove(p)


def _film_frame(sc, seed, spp):
    """one frame into a zeroed device film -> (film as numpy, stats, mask of the specialised first-bounce kernel it launched)"""
    import torch
    W, H = sc.size
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    st = sc.render_rows(film.data_ptr(), seed, spp, 0, H)
    return film.cpu().numpy(), st, sc.last_plan_mask


def _on_and_off(sc, monkeypatch, seed, spp, what, mask_on):
    """the frame with the switch off (twice: the film must be reproducible) and on; the switch-on frame must have launched the kernel of `mask_on` -> (film off, film on)"""
    monkeypatch.setenv(SWITCH, "0")
    off_a, st_off, m_off = _film_frame(sc, seed, spp)
    off_b, _, _ = _film_frame(sc, seed, spp)
    assert np.isfinite(off_a).all() and np.abs(off_a[..., :3]).max() > 0 and (off_a[..., 3] > 0).all(), what
    assert np.array_equal(bits(off_a), bits(off_b)), (what, "the film chosen as reproducible is not", int((bits(off_a) != bits(off_b)).sum()))
    assert st_off["n_plan_facts_launches"] == 0 and m_off == 0 and st_off["n_launches_first"] == 1 and st_off["n_fused_splat_launches"] == 1, (what, st_off, hex(m_off))
    monkeypatch.setenv(SWITCH, "1")
    on, st_on, m_on = _film_frame(sc, seed, spp)
    assert st_on["n_plan_facts_launches"] == 1 and m_on == mask_on, (what, st_on, hex(m_on), hex(mask_on))
    for k in STATS:
        assert st_on[k] == st_off[k], (what, k, st_on[k], st_off[k])
    return off_a, on


# ---------------------------------------------------------------------------- 6. without a GPU
def test_the_masks():
    """the shape sits behind one presence bit above the route facts; C2's mask is the route kernel's and the fields 5 and 2"""
    assert FACT_BIT["kFactFlatShape"] == 18 and FACT_BIT["kFactIdShift24"] == 17
    assert ROUTE_MASK == 0x3ffff and SHAPE_MASK == ROUTE_MASK | SHAPE_5_2 and SHAPE_5_2 == 1 << 18 | 5 << 19 | 2 << 23 and SHAPE_5_2 & ~SHAPE_FIELDS == 0


PLANS = [("closed", [1, 1, 5, 2]), ("panel", [1, 1, 5, 2]), ("six", [1, 1, 6, 2]), ("wall_at_3", [1, 1, 5, 3])]


def test_the_frame_plan_reads_the_shape_off_the_scene(mi, wall):
    """what FramePlan::launch_facts gets from plan_frame (dtof_scene_export kind 26: one wall, a shape, its object count, the wall's index)"""
    for room, want in PLANS:
        got = mi.load_file(wall("tent", None, room), resx=16, resy=16).export(26)
        assert got.tolist() == want, (room, got)
    assert mi.load_file(os.path.join(SCENES, "cornell_wall.xml")).export(26).tolist() == [1, 1, 5, 2]
    assert mi.load_file(os.path.join(SCENES, "cornell_boxes.xml")).export(26).tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------- 1. one-pixel crops of the closed room, 2. of the room with the panel
CROPS = [("corner_0_0", (0, 0)), ("edge_15_3", (15, 3)), ("inside_5_9", (5, 9))]
CROP_CASES = [("%s_%s" % (f, n), f, c) for f in ("tent", "tent075") for n, c in CROPS]
# pixels that show the back wall beside the panel, the floor in front of it and the panel itself (it covers x 8 .. 11, y 9 .. 11 of the 16 x 16 frame): bounces from
# there land in the panel's shadow, and every shadow ray that starts behind its plane crosses it
PANEL_CROPS = [("beside_6_10", (6, 10)), ("floor_9_14", (9, 14)), ("panel_9_10", (9, 10))]
PANEL_CASES = [("%s_%s" % (f, n), f, c) for f, (n, c) in zip(("tent", "tent075", "tent"), PANEL_CROPS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,rfilter,crop", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_shaped_kernel_film_of_a_one_pixel_crop_is_the_generic_fused_film(mi, wall, monkeypatch, name, rfilter, crop):
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for max_depth in (2, 3, 4):
        sc = mi.load_file(wall(rfilter, crop), resx=16, resy=16, max_depth=max_depth)
        assert sc.size == (1, 1) and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop
        for seed in (4, 11):
            what = (name, max_depth, seed)
            off, on = _on_and_off(sc, monkeypatch, seed, 64, what, SHAPE_MASK)
            # dtof_scene_last_plan_facts carries the shape bit and the fields; Scene.last_plan_facts is the one-bit facts of it, Scene.last_plan_shape the fields
            assert sc.last_plan_mask & 1 << FACT_BIT["kFactFlatShape"] and sc.last_plan_facts == ROUTE_MASK and sc.last_plan_shape == (5, 2), what
            assert np.array_equal(bits(on), bits(off)), (what, on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name,rfilter,crop", PANEL_CASES, ids=[c[0] for c in PANEL_CASES])
def test_shaped_kernel_film_of_a_crop_with_occluded_shadow_rays_is_the_generic_fused_film(mi, wall, monkeypatch, name, rfilter, crop):
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for max_depth in (3, 4):
        sc = mi.load_file(wall(rfilter, crop, "panel"), resx=16, resy=16, max_depth=max_depth)
        assert sc.size == (1, 1)
        for seed in (4, 11):
            what = (name, max_depth, seed)
            off, on = _on_and_off(sc, monkeypatch, seed, 64, what, SHAPE_MASK)
            assert np.array_equal(bits(on), bits(off)), (what, on, off)


def _count_full_occlusion_tests():
    """(child process on the stats build) per room and crop: slots 16 .. 19 of the traversal counters after one frame of the shaped kernel, as a JSON line"""
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import mitsuba3dopplertof_amd as mi
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()
    out, made = {}, []
    try:
        for room, crops in (("panel", PANEL_CROPS), ("closed", PANEL_CROPS + CROPS)):
            for name, crop in crops:
                made.append(os.path.join(SCENES, "_flat_shape_stats_%d_%d.xml" % (os.getpid(), len(made))))
                open(made[-1], "w").write(_variant(base, "tent", crop, room))
                sc = mi.load_file(made[-1], resx=16, resy=16, max_depth=4)
                slots = (C.c_ulonglong * 24)()
                mi._lib().dtof_debug_traversal_stats_n(slots, 24)   # (reads and resets)
                film = torch.zeros((1, 1, 4), dtype=torch.float32, device="cuda")
                sc.render_rows(film.data_ptr(), 4, 64, 0, 1)
                torch.cuda.synchronize()
                mi._lib().dtof_debug_traversal_stats_n(slots, 24)
                out["%s/%s" % (room, name)] = dict(mask=sc.last_plan_mask, slots=[int(x) for x in slots[16:24]])
    finally:
        for p in made:
            os.remove(p)
    print("FLAT_SHAPE_STATS " + json.dumps(out))


@pytest.mark.gpu
def test_the_tail_runs_where_shadow_rays_cross_the_panel_and_nowhere_in_the_closed_room():
    """the stats build counts a full occlusion test (slot 19) only in the tail of the shaped occlusion query: some on every crop of the room with the panel, none in the closed
    room, whose z rows settle every visit (slot 17 = slot 16); every shadow ray's five z rows are counted once (slot 18 = 5 per query of a wave)"""
    assert os.path.exists(STATS_LIB), "libdtof_stats.so is not built (make -C mitsuba3dopplertof_amd/csrc stats; build() makes it)"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--count-full-occlusion-tests"], env=dict(os.environ, DTOF_LIB=STATS_LIB, DTOF_PLAN_FACTS="1", **HEADLINE_SHAPE),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = json.loads(re.search(r"^FLAT_SHAPE_STATS (.*)$", r.stdout, re.M).group(1))
    print(got)
    assert len(got) == 2 * len(PANEL_CROPS) + len(CROPS)
    for key, rec in got.items():
        lane_tests, lane_settled, wave_z, wave_full = rec["slots"][:4]
        assert rec["mask"] == SHAPE_MASK, (key, hex(rec["mask"]))
        assert lane_tests > 0 and wave_z > 0 and wave_z % 5 == 0 and lane_tests % 5 == 0, (key, rec)
        if key.startswith("panel/"):
            assert wave_full > 0 and lane_settled < lane_tests, (key, rec)
        else:
            assert wave_full == 0 and lane_settled == lane_tests, (key, rec)


# ---------------------------------------------------------------------------- 3. other shapes
@pytest.mark.gpu
@pytest.mark.parametrize("room", ["six", "wall_at_3"])
def test_a_table_of_another_shape_takes_the_kernel_without_the_shape(mi, wall, monkeypatch, room):
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for rfilter, crop in (("tent", (5, 9)), ("tent075", (0, 0))):
        sc = mi.load_file(wall(rfilter, crop, room), resx=16, resy=16)
        off, on = _on_and_off(sc, monkeypatch, 6, 64, (room, rfilter, crop), ROUTE_MASK)
        assert sc.last_plan_shape is None and sc.last_plan_facts == ROUTE_MASK, (room, rfilter, crop)
        assert np.array_equal(bits(on), bits(off)), (room, rfilter, crop, on, off)


# ---------------------------------------------------------------------------- 4. a frame against the oracle
@pytest.mark.gpu
def test_shaped_kernel_frame_matches_the_oracle_film(mi, orc, monkeypatch):
    """cornell_wall 16 x 16 x 64 with the tent filter into a device film: one launch of the kernel of kHeadlineShapeFacts; colour and weight within IMG_TOL of the oracle's film"""
    for k, v in dict(HEADLINE_SHAPE, **{SWITCH: "1"}).items():
        monkeypatch.setenv(k, v)
    path, params, spp = os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16), 64
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    got, st, mask = _film_frame(sc, 5, spp)
    assert mask == SHAPE_MASK and st["n_plan_facts_launches"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1 and st["n_paths"] == 16 * 16 * spp, (st, hex(mask))
    ref = osc.render(osc.params(), seed=5, spp=spp, raw=True, threads=NCPU)[0]
    for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
        err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
        print("shaped kernel, %s: %.3g of the largest value (bound %g)" % (name, err, IMG_TOL))
        assert err <= IMG_TOL, (name, err)


# ---------------------------------------------------------------------------- 5. the pattern-initialised build
@pytest.mark.gpu
def test_crop_cases_on_the_pattern_initialised_build():
    """the crops of 1 and 2 in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "film_of_a"],
                       env=dict(os.environ, DTOF_LIB=PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]


if __name__ == "__main__" and sys.argv[1:] == ["--count-full-occlusion-tests"]:
    _count_full_occlusion_tests()
