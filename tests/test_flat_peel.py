"""trace_flat's rectangle loop in the kernels compiled with kFactOneWall (dtof_traverse.h, DTOF_FLAT_PEEL): the flat table is visited as the rectangles
below the wall, the wall with its own ray, the rectangles above it -- instead of one loop that copies each object's ray into place -- and must give the films of the
generic kernel (DTOF_PLAN_FACTS=0), whose single loop is untouched, bit for bit.

  1. the wall as the first, the middle (stock) and the last object of the table (an empty lower segment, neither, an empty upper segment): cornell_wall 16 x 16 x 64
     stratified, max_depth 1 .. 4, and 8 x 8 x 256 antithetic_mirror (C3's form, the 0xfff kernel);
  2. tables of two objects (the wall at index 0 and at index 1) and of eight, the limit of the flat path, with the wall at index 7;
  3. exact ties: one static rectangle twice in the table with an identical to_world and different reflectances -- one copy on each side of the wall, and both below
     it.  Their t are the same bits, so the lower index wins (ascending order, strict <); the film with the two reflectances exchanged differs, so a wrong winner shows;
  4. the fused kernel (0x1fff) on 1 x 1 crops at a corner and inside, tent radius 1, the wall first and last: every film word is one atomic add onto zero;
  5. the cases of 1 and 3 on the pattern-initialised build, in a child process.

Every comparison is bit equality of reproducible films (box filter, or fused 1 x 1 crops), with equal statistics; n_plan_facts_launches says that the specialised
kernel ran.  Frames are launched in the headline's shape (DTOF_CHUNK_SEGS=0), as tests/test_plan_facts.py explains.  Scene variants are written next to
scenes/cornell_wall.xml and removed afterwards, as tests/test_flat_facts.py does."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

SWITCH = "DTOF_PLAN_FACTS"
HEADLINE_SHAPE = dict(DTOF_CHUNK_SEGS="0")
PATTERN_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_pattern.so")
STATS = ("n_paths", "n_bounces", "n_shadow_rays", "n_bounces_inline", "n_launches_trace", "n_launches_shade", "n_launches_shadow", "n_launches_first", "n_fused_splat_launches")

SHAPE_BLOCK = re.compile(r'\t<shape type="rectangle" id="(\w+)">.*?</shape>\n', re.S)
STOCK = ("Floor", "Ceiling", "BackWall", "RightWall", "LeftWall")
WALL = "BackWall"


def _static(name, to_world, bsdf):
    return '\t<shape type="rectangle" id="%s"><transform name="to_world">%s</transform><ref id="%s" /></shape>\n' % (name, to_world, bsdf)


TILTED_XF = '<scale x="0.3" y="0.7" z="1" /><rotate x="0.3" y="1" z="0.2" angle="37" /><translate x="0.2" y="0.9" z="0.1" />'   # tests/test_flat_facts.py's
DUP_XF = '<scale x="0.45" y="0.35" z="1" /><rotate x="1" y="0.4" z="0.1" angle="-28" /><translate x="-0.15" y="0.8" z="0.35" />'
EXTRA = {
    "Tilted": _static("Tilted", TILTED_XF, "ShortBoxBSDF"),
    "PanelA": _static("PanelA", '<scale value="0.25" /><rotate y="1" angle="30" /><translate x="-0.45" y="0.5" z="-0.2" />', "ShortBoxBSDF"),
    "PanelB": _static("PanelB", '<scale x="0.2" y="0.5" z="1" /><rotate x="1" angle="60" /><translate x="0.5" y="1.4" z="0.3" />', "TallBoxBSDF"),
    # the same rectangle twice: identical to_world, the red and the green wall's reflectance
    "DupRed": _static("DupRed", DUP_XF, "LeftWallBSDF"),
    "DupGreen": _static("DupGreen", DUP_XF, "RightWallBSDF"),
}
LAYOUTS = {
    "wall_first": (WALL, "Floor", "Ceiling", "RightWall", "LeftWall"),
    "wall_middle": STOCK,
    "wall_last": ("Floor", "Ceiling", "RightWall", "LeftWall", WALL),
    "two_wall_0": (WALL, "Floor"),
    "two_wall_1": ("Floor", WALL),
    "eight_wall_7": ("Floor", "Ceiling", "RightWall", "LeftWall", "Tilted", "PanelA", "PanelB", WALL),
    # ties across the wall, and both copies below it; *_swapped: the two reflectances exchanged
    "tie_across": ("Floor", "DupRed", WALL, "DupGreen", "RightWall", "LeftWall", "Ceiling"),
    "tie_across_swapped": ("Floor", "DupGreen", WALL, "DupRed", "RightWall", "LeftWall", "Ceiling"),
    "tie_below": ("DupRed", "DupGreen", "Floor", "Ceiling", WALL, "RightWall", "LeftWall"),
    "tie_below_swapped": ("DupGreen", "DupRed", "Floor", "Ceiling", WALL, "RightWall", "LeftWall"),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _variant(xml, layout, rfilter="box", crop=None):
    """cornell_wall.xml with its shapes replaced by those of `layout`, in that order (the order of the flat table), another reconstruction filter, a crop window"""
    assert xml.count('<rfilter type="tent" />') == 1
    xml = xml.replace('<rfilter type="tent" />', '<rfilter type="%s" />' % rfilter)
    if crop is not None:
        assert xml.count('<string name="file_format"') == 1
        xml = xml.replace('<string name="file_format"', '<integer name="crop_offset_x" value="%d" /><integer name="crop_offset_y" value="%d" />'
                          '<integer name="crop_width" value="1" /><integer name="crop_height" value="1" /><string name="file_format"' % crop)
    blocks = dict(EXTRA, **{m.group(1): m.group(0) for m in SHAPE_BLOCK.finditer(xml)})
    assert all(k in blocks for k in STOCK) and "<animation" in blocks[WALL]
    xml = SHAPE_BLOCK.sub("", xml)
    assert "<shape" not in xml and xml.count("\t<emitter") == 1
    return xml.replace("\t<emitter", "".join(blocks[k] for k in LAYOUTS[layout]) + "\t<emitter")


@pytest.fixture(scope="module")
def scene_file():
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(layout, rfilter="box", crop=None):
        key = (layout, rfilter, crop)
        if key not in made:
            made[key] = os.path.join(SCENES, "_flat_peel_%d_%s_%s_%s.xml" % (os.getpid(), layout, rfilter, "x".join(map(str, crop)) if crop else "full"))
            open(made[key], "w").write(_variant(base, layout, rfilter, crop))
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
    """the frame with the switch off (twice: the film must be reproducible) and on -> (film off, film on, stats on)"""
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
    return off_a, on, st_on


def _wall_index(sc):
    """the moving wall's index in the flat table (DFlatFrame export: mark 2) and the table's size"""
    marks = sc.export(25).reshape(-1, 13)[:, 0]
    assert sorted(marks)[-1] == 2 and np.count_nonzero(marks) == 1, marks
    return int(np.flatnonzero(marks)[0]), len(marks)


def _same_bits_with_the_facts(mi, scene_file, monkeypatch, layout, params, spp, seed=3):
    for k, v in dict(HEADLINE_SHAPE, DTOF_FUSE_SPLAT="0").items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(scene_file(layout), **params)
    assert _wall_index(sc) == (LAYOUTS[layout].index(WALL), len(LAYOUTS[layout])), layout
    lit = params.get("max_depth", 4) > 1   # (max_depth = 1: a scene lit by a point light gathers nothing, no bounce kernel is launched and the film is its weights)
    off, on, st_on = _on_and_off(sc, monkeypatch, seed, spp, (layout, params), lit=lit)
    assert st_on["n_plan_facts_launches"] == (1 if lit else 0) and st_on["n_fused_splat_launches"] == 0, st_on      # the kernel of kHeadlineFacts ran
    assert np.array_equal(bits(on), bits(off)), (layout, params, int((bits(on) != bits(off)).sum()), float(np.abs(on - off).max()))
    return off


# ---------------------------------------------------------------------------- without a GPU
def test_layouts_put_the_wall_where_they_say(mi, scene_file):
    """the flat table follows the order of the shapes in the file; the two tie scenes hold the same rectangle twice, bit for bit"""
    for layout, names in LAYOUTS.items():
        sc = mi.load_file(scene_file(layout), resx=8, resy=8)
        assert _wall_index(sc) == (names.index(WALL), len(names)), layout
        if layout.startswith("tie"):
            rec = sc.export(25).reshape(-1, 13)
            a, b = sorted((names.index("DupRed"), names.index("DupGreen")))
            assert np.array_equal(bits(rec[a]), bits(rec[b])) and a < names.index(WALL) and (b > names.index(WALL)) == ("across" in layout), layout


# ---------------------------------------------------------------------------- 1. the wall's position
FORMS = [("stratified_depth%d" % d, dict(resx=16, resy=16, max_depth=d), 64) for d in (1, 2, 3, 4)]
FORMS += [("mirror_256_depth%d" % d, dict(resx=8, resy=8, max_depth=d, time_sampling_method="antithetic_mirror"), 256) for d in (1, 2, 3, 4)]
POSITIONS = [(layout,) + f for layout in ("wall_first", "wall_middle", "wall_last") for f in FORMS]


@pytest.mark.gpu
@pytest.mark.parametrize("layout,name,params,spp", POSITIONS, ids=["%s-%s" % c[:2] for c in POSITIONS])
def test_wall_position_film_is_the_generic_kernels(mi, scene_file, monkeypatch, layout, name, params, spp):
    _same_bits_with_the_facts(mi, scene_file, monkeypatch, layout, params, spp)


# ---------------------------------------------------------------------------- 2. the table's size
SIZES = [(layout,) + f for layout in ("two_wall_0", "two_wall_1", "eight_wall_7") for f in (FORMS[3], FORMS[1], FORMS[7])]


@pytest.mark.gpu
@pytest.mark.parametrize("layout,name,params,spp", SIZES, ids=["%s-%s" % c[:2] for c in SIZES])
def test_table_of_two_and_of_eight_objects(mi, scene_file, monkeypatch, layout, name, params, spp):
    _same_bits_with_the_facts(mi, scene_file, monkeypatch, layout, params, spp)


# ---------------------------------------------------------------------------- 3. exact ties
TIES = [(layout,) + f for layout in ("tie_across", "tie_below") for f in (FORMS[3], FORMS[1], FORMS[7])]


@pytest.mark.gpu
@pytest.mark.parametrize("layout,name,params,spp", TIES, ids=["%s-%s" % c[:2] for c in TIES])
def test_equal_t_goes_to_the_lower_index(mi, scene_file, monkeypatch, layout, name, params, spp):
    film = _same_bits_with_the_facts(mi, scene_file, monkeypatch, layout, params, spp)
    swapped = _same_bits_with_the_facts(mi, scene_file, monkeypatch, layout + "_swapped", params, spp)
    # the copies are seen (the other winner is another film), so the equality above did decide between them
    assert not np.array_equal(bits(film[..., :3]), bits(swapped[..., :3])), layout
    assert np.array_equal(bits(film[..., 3]), bits(swapped[..., 3])), layout       # (the weights do not depend on a reflectance)


# ---------------------------------------------------------------------------- 4. the fused kernel
CROPS = [(layout, crop) for layout in ("wall_first", "wall_last") for crop in ((0, 0), (15, 15), (5, 9))]


@pytest.mark.gpu
@pytest.mark.parametrize("layout,crop", CROPS, ids=["%s-%d_%d" % ((c[0],) + c[1]) for c in CROPS])
def test_fused_kernel_film_of_a_one_pixel_crop(mi, scene_file, monkeypatch, layout, crop):
    """a 1 x 1 crop of the 16 x 16 frame at 64 spp is ONE wave: each of the film's four words receives one atomic add of the wave's reduction, so the fused film is
    reproducible and the kernel with every fact (0x1fff) must give the generic fused kernel's bits"""
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(scene_file(layout, "tent", crop), resx=16, resy=16)
    assert sc.size == (1, 1) and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop
    off, on, st_on = _on_and_off(sc, monkeypatch, 4, 64, (layout, crop))
    assert st_on["n_fused_splat_launches"] == 1 and st_on["n_plan_facts_launches"] == 1 and st_on["n_paths"] == 64, st_on
    assert np.array_equal(bits(on), bits(off)), (layout, crop, on, off)


# ---------------------------------------------------------------------------- 5. the pattern-initialised build
@pytest.mark.gpu
def test_positions_and_ties_on_the_pattern_initialised_build():
    """cases 1 and 3 in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "wall_position or equal_t"],
                       env=dict(os.environ, DTOF_LIB=PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
