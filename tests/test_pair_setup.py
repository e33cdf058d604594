"""The chunk-pair setup of C2's first-bounce kernel (DTOF_PAIR_SETUP, dtof_kernels.h; dtof_pair_setup.h): what the two lanes of a correlated pair share of
lane generation -- the path stream's seeding, its two jitter draws, the sample position, the camera ray -- is evaluated once per pair, at every even chunk of a segment
for the pairs of that chunk (even lanes) and of the chunk after it (odd lanes), carried in registers over the two chunks and fetched by both lanes of a pair.  The values
are the same functions of the same integers, evaluated in another lane, so every lane and every film must keep its bits.

  1. lanes: form 1 of dtof_pair_setup_lanes (the chunk-pair form, the device functions k_shade calls) against form 0 (generate_lane per lane) in all 16 words, and its
     first nine words against Scene.sample_lanes and the oracle's render_lanes -- over ranges with a lone tail chunk, a pair of chunks, a pair plus a tail, a whole
     segment, a second segment that is a lone tail, the 512 + 7 chunks of a 5 x 3 frame, and a 3 x 3 crop whose chunk pair (2, 3) straddles a row; the
     refusals;
  2. films, bit for bit: crops of 2 x 1 and 1 x 2 pixels -- two chunks of one segment, the second set up by the odd lanes of the first -- against DTOF_PLAN_FACTS=0.
     The oracle picks crops in which every sample's floored position is its own pixel: each film cell then takes exactly one atomic from each of the two waves, and
     two float additions onto zero commute.  Among them an all-static pixel beside an all-wall one in both orders, and a crop with a mixed pixel
     (test_pair_walk._classify);
  3. films within IMG_TOL of the oracle's: the 3 x 3 crop, the 5 x 3 frame, the 16 x 16 frame; statistics equal to the switch-off frame's;
  4. 2. and 3. on the pattern-initialised library, in a child process.

16 x 16 or smaller, 64 spp, seeds 4 and 11, frames in the headline's shape (DTOF_CHUNK_SEGS=0: one block per 512-lane segment, as tests/test_plan_facts.py explains).
The one-pixel crops of tests/test_pair_samples.py and tests/test_pair_walk.py run the tail chunk of the same kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_pair_samples as ps
import test_pair_walk as pw
from conftest import SCENES

SEEDS = ps.SEEDS
SPP = ps.SPP
PARAMS = dict(resx=16, resy=16, max_depth=4)
SMALL = dict(resx=5, resy=3, max_depth=4)
CROP3 = (6, 1, 3, 3)       # x, y, width, height: rows 1 .. 3 at columns 6 .. 8 of the 16 x 16 film -- wall and ceiling
LANE_WORDS = (("sample_pos", slice(0, 2)), ("time", slice(2, 3)), ("ray_o", slice(3, 6)), ("ray_d", slice(6, 9)))


def _variant(xml, rfilter, crop):
    """cornell_wall.xml with another tent radius and a crop window (x, y, width, height)"""
    assert xml.count('<rfilter type="tent" />') == 1 and xml.count('<string name="file_format"') == 1
    xml = xml.replace('<rfilter type="tent" />', {"tent": '<rfilter type="tent" />', "tent075": '<rfilter type="tent"><float name="radius" value="0.75" /></rfilter>'}[rfilter])
    if crop is not None:
        xml = xml.replace('<string name="file_format"', '<integer name="crop_offset_x" value="%d" /><integer name="crop_offset_y" value="%d" />'
                          '<integer name="crop_width" value="%d" /><integer name="crop_height" value="%d" /><string name="file_format"' % crop)
    return xml


@pytest.fixture(scope="module")
def wall():
    """variants of scenes/cornell_wall.xml written next to it and removed afterwards"""
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(rfilter="tent", crop=None):
        key = (rfilter, crop)
        if key not in made:
            made[key] = os.path.join(SCENES, "_pair_setup_%d_%d.xml" % (os.getpid(), len(made)))
            open(made[key], "w").write(_variant(base, rfilter, crop))
        return made[key]
    yield get
    for p in made.values():
        os.remove(p)


# ---------------------------------------------------------------------------- 1. lanes
def _scene_of(wall, which):
    return (wall("tent", CROP3), PARAMS) if which == "crop3" else (os.path.join(SCENES, "cornell_wall.xml"), SMALL)


LANE_RANGES = [("lone_tail", "frame5x3", 0, 64), ("one_pair", "frame5x3", 0, 128), ("pair_and_tail", "frame5x3", 0, 192), ("segment", "frame5x3", 0, 512),
               ("segment_and_lone_tail", "frame5x3", 0, 576), ("frame_5x3", "frame5x3", 0, 960), ("crop_3x3", "crop3", 0, 576)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,which,begin,n", LANE_RANGES, ids=[c[0] for c in LANE_RANGES])
def test_chunk_pair_lanes_are_the_per_lane_lanes_and_the_oracles(mi, orc, wall, name, which, begin, n):
    path, params = _scene_of(wall, which)
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    W, H = sc.size
    assert (W, H) == ((3, 3) if which == "crop3" else (5, 3)) and begin + n <= W * H * SPP
    for seed in SEEDS:
        per_lane, pairs = sc.pair_setup_lanes(seed, SPP, begin, n, form=0), sc.pair_setup_lanes(seed, SPP, begin, n, form=1)
        assert per_lane.shape == pairs.shape == (n, 16) and per_lane.dtype == pairs.dtype == np.uint32
        differ = (per_lane != pairs).any(axis=1)
        assert not differ.any(), (name, seed, "lanes that differ between the forms", np.flatnonzero(differ)[:8], per_lane[differ][:2], pairs[differ][:2])
        assert not pairs[:, 13:].any(), (name, seed)
        # the two lanes of a pair: one position, one ray, one path stream -- and times of their own
        assert np.array_equal(pairs[0::2, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]], pairs[1::2, [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]]) and (pairs[0::2, 2] != pairs[1::2, 2]).all(), (name, seed)
        g, o = sc.sample_lanes(seed, SPP, begin, n), osc.render_lanes(osc.params(), seed, SPP, begin, n, threads=ps.NCPU)
        for f, cols in LANE_WORDS:
            mine = pairs[:, cols].reshape(n, -1)
            for other, whose in ((g, "sample_lanes"), (o, "the oracle")):
                theirs = ps.bits(other[f]).reshape(n, -1)
                assert np.array_equal(mine, theirs), (name, seed, f, whose, int((mine != theirs).any(axis=1).sum()))
        print("%s seed %d: %d lanes, 16 words equal between the forms, 9 equal to sample_lanes and the oracle" % (name, seed, n))


@pytest.mark.gpu
def test_a_chunk_pair_of_the_crop_straddles_a_row(mi, wall):
    """the premise of the 3 x 3 case: pixel 2 is the last of row 0 and pixel 3 the first of row 1, so chunk pair (2, 3) is set up from two pixels that are not neighbours
    in a row.  (Of the segment's other pairs, (0, 1), (4, 5) and (6, 7) each lie in one row; chunk 8 is the second segment's lone tail.)"""
    sc = mi.load_file(wall("tent", CROP3), **PARAMS)
    pos = sc.pair_setup_lanes(SEEDS[0], SPP, 0, 576)[:, :2].copy().view(np.float32).reshape(9, SPP, 2)
    px = np.floor(pos).astype(int)
    assert (px[2] == (CROP3[0] + 2, CROP3[1])).all() and (px[3] == (CROP3[0], CROP3[1] + 1)).all(), (px[2][0], px[3][0])


@pytest.mark.gpu
def test_refusals(mi, wall):
    """what the entry's kernels are not compiled for is refused before anything is launched, and the output stays untouched"""
    path = os.path.join(SCENES, "cornell_wall.xml")
    sc = mi.load_file(path, **SMALL)
    L = mi._lib()
    out = np.full((128, 16), 0xabababab, np.uint32)
    call = lambda s, form, spp, begin, n: L.dtof_pair_setup_lanes(s._h, form, 4, spp, begin, n, out.ctypes.data)
    assert call(sc, 1, SPP, 0, 128) == 0 and (out != 0xabababab).any()
    out[:] = 0xabababab
    cases = [("a lane_begin that is no multiple of 64", sc, 1, SPP, 32, 64), ("an n that is no multiple of 64", sc, 1, SPP, 0, 96), ("n above 2^24", sc, 1, SPP, 0, (1 << 24) + 64),
             ("a range beyond the wavefront", sc, 1, SPP, 960, 64), ("a form that does not exist", sc, 2, SPP, 0, 64), ("32 samples per pixel", sc, 1, 32, 0, 64),
             ("96 samples per pixel", sc, 1, 96, 0, 64),
             ("antithetic time sampling", mi.load_file(path, time_sampling_method="antithetic", **SMALL), 1, SPP, 0, 64),
             ("antithetic time sampling, per lane", mi.load_file(path, time_sampling_method="antithetic", **SMALL), 0, SPP, 0, 64)]
    for what, s, form, spp, begin, n in cases:
        assert call(s, form, spp, begin, n) == pw.INVALID, what
        assert (out == 0xabababab).all(), what
    with pytest.raises(mi.DtofError):
        sc.pair_setup_lanes(4, SPP, 32, 64)
    assert L.dtof_pair_setup_lanes(None, 1, 4, SPP, 0, 64, out.ctypes.data) == pw.INVALID and L.dtof_pair_setup_lanes(sc._h, 1, 4, SPP, 0, 64, None) == pw.INVALID


# ---------------------------------------------------------------------------- 2. films, bit for bit
SHAPES = {"2x1": (2, 1), "1x2": (1, 2)}
CASES = ("static_wall", "wall_static", "mixed")


def _own_pixel(osc, seed, crop):
    """does every sample of the crop scene lie, floored, in its own pixel?"""
    x, y, w, h = crop
    pos = osc.render_lanes(osc.params(), seed, SPP, 0, w * h * SPP, threads=ps.NCPU)["sample_pos"].reshape(w * h, SPP, 2)
    want = np.array([(x + p % w, y + p // w) for p in range(w * h)])[:, None, :]
    return bool((np.floor(pos).astype(int) == want).all())


RESOLUTIONS = (16, 15, 14, 13, 12, 11, 10, 9, 8)


@pytest.fixture(scope="module")
def crops(orc, wall):
    """{(seed, shape, case): (film size, crop)}: the frame's pixels classified by the oracle; every window of the frame whose two pixels are not both static or both on
    the wall there is then classified from the lanes of its own CROP scene (a crop's samples are not the frame's), and for every shape and case the first window is
    taken whose crop is of the case and whose samples all lie in their own pixels.  The 64 sample offsets of a crop are the same in every crop of a seed, and at
    16 x 16 they put a sample across some of the wall's edges from every pixel beside them: the square films from 16 x 16 down are searched in turn until every case
    has its crop."""
    want = {"static_wall": lambda a, b: (a, b) == (pw.STATIC, pw.ALL_WALL), "wall_static": lambda a, b: (a, b) == (pw.ALL_WALL, pw.STATIC), "mixed": lambda a, b: pw.MIXED in (a, b)}
    chosen = {}
    for seed in SEEDS:
        for res in RESOLUTIONS:
            params = dict(PARAMS, resx=res, resy=res)
            cls = pw._classify(orc.Scene(os.path.join(SCENES, "cornell_wall.xml"), params), seed, res * res)[0].reshape(res, res)
            for shape, (w, h) in SHAPES.items():
                for p in np.random.default_rng([seed, w, 7]).permutation(res * res):
                    if all((seed, shape, case) in chosen for case in CASES):
                        break
                    x, y = int(p % res), int(p // res)
                    if x + w > res or y + h > res or (cls[y, x] == cls[y + h - 1, x + w - 1] and cls[y, x] != pw.MIXED):
                        continue
                    crop = (x, y, w, h)
                    osc = orc.Scene(wall("tent", crop), params)
                    own = pw._classify(osc, seed, 2)[0]
                    for case in CASES:
                        if (seed, shape, case) not in chosen and want[case](own[0], own[1]) and _own_pixel(osc, seed, crop):
                            chosen[(seed, shape, case)] = (res, crop)
            if all((seed, shape, case) in chosen for shape in SHAPES for case in CASES):
                break
        print("seed %d: %s" % (seed, {k[1:]: v for k, v in chosen.items() if k[0] == seed}))
    return chosen


def test_the_oracle_finds_two_pixel_crops_of_every_case(crops):
    """(no GPU) for both shapes: a static pixel before a wall pixel and a wall pixel before a static one, each at one of the seeds at least, and a crop with a mixed pixel
    at both.  (Not every order exists at every seed: a crop's 64 sample offsets per pixel are fixed by the seed, and at seed 4 no film from 8 x 8 to 16 x 16 has a
    window of 1 x 2 whose upper pixel stays clear of the wall while the lower lies on it whole; likewise 2 x 1, wall before static, at seed 11.)"""
    for sh in SHAPES:
        assert all((s, sh, "mixed") in crops for s in SEEDS), sorted(crops)
        for c in ("static_wall", "wall_static"):
            assert any((s, sh, c) in crops for s in SEEDS), (sh, c, sorted(crops))
    assert len(crops) >= 10, sorted(crops)


FILM_CASES = [(f, sh, c) for f in ("tent", "tent075") for sh in SHAPES for c in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("rfilter,shape,case", FILM_CASES, ids=["%s_%s_%s" % c for c in FILM_CASES])
def test_pair_setup_film_of_a_two_pixel_crop_is_the_generic_fused_film(mi, wall, crops, monkeypatch, rfilter, shape, case):
    for k, v in ps.HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for seed in SEEDS:
        if (seed, shape, case) not in crops:   # (test_the_oracle_finds_two_pixel_crops_of_every_case: the case exists at the other seed)
            continue
        res, crop = crops[(seed, shape, case)]
        sc = mi.load_file(wall(rfilter, crop), **dict(PARAMS, resx=res, resy=res))
        assert sc.size == SHAPES[shape] and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop[:2]
        what = (rfilter, shape, case, res, crop, seed)
        off, on, st = ps._on_and_off(sc, monkeypatch, seed, SPP, what, ps.PAIR_MASK)      # (every statistic of ps.STATS equal, the mask that ran)
        assert sc.last_plan_kernel == 0x52fffff and sc.last_plan_pair_samples and sc.last_plan_mask == ps.SHAPE_MASK, what
        assert np.array_equal(ps.bits(on), ps.bits(off)), (what, on, off)
        print("%s: film bits and statistics equal (n_bounces %d, shadow rays %d)" % (what, st["n_bounces"], st["n_shadow_rays"]))


# ---------------------------------------------------------------------------- 3. films within tolerance
FRAMES = [("crop_3x3", "crop3", PARAMS, 9), ("frame_5x3", None, SMALL, 15), ("frame_16x16", None, PARAMS, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,which,params,n_pixels", FRAMES, ids=[c[0] for c in FRAMES])
def test_pair_setup_frame_matches_the_oracle_film(mi, orc, wall, monkeypatch, name, which, params, n_pixels):
    """one launch of the headline kernel over several segments' chunk pairs: colour and weight within IMG_TOL of the oracle's film, statistics those of the switch-off frame"""
    for k, v in ps.HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    path = wall("tent", CROP3) if which == "crop3" else os.path.join(SCENES, "cornell_wall.xml")
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    for seed in SEEDS:
        monkeypatch.setenv(ps.SWITCH, "0")
        _, st_off, k_off = ps._film_frame(sc, seed, SPP)
        monkeypatch.setenv(ps.SWITCH, "1")
        got, st, kernel = ps._film_frame(sc, seed, SPP)
        assert k_off == 0 and kernel == ps.PAIR_MASK and st["n_plan_facts_launches"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1, (name, seed, st, hex(kernel))
        assert st["n_paths"] == n_pixels * SPP, (name, seed, st)
        for k in ps.STATS:
            assert st[k] == st_off[k], (name, seed, k, st[k], st_off[k])
        ref = osc.render(osc.params(), seed=seed, spp=SPP, raw=True, threads=ps.NCPU)[0]
        for ch, what in ((slice(0, 3), "rgb"), (3, "W")):
            err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
            print("%s seed %d, %s: %.3g of the largest value (bound %g)" % (name, seed, what, err, ps.IMG_TOL))
            assert err <= ps.IMG_TOL, (name, seed, what, err)


# ---------------------------------------------------------------------------- 4. the pattern-initialised build
@pytest.mark.gpu
def test_crop_and_frame_cases_on_the_pattern_initialised_build():
    """the crops and the frames in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(ps.PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "two_pixel_crop or matches_the_oracle_film"],
                       env=dict(os.environ, DTOF_LIB=ps.PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
