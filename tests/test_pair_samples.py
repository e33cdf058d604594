"""The pair samples of C2's first-bounce kernel (k_shade's FACTS mask, dtof_kernels.h: kFactPairSamples) against the generic kernels, which
DTOF_PLAN_FACTS=0 restores.

Under the fact the two lanes of a correlated pair -- one path stream, every draw of the bounce loop from it -- evaluate the BSDF direction of ONE sampling iteration each
(the even lane iteration 0's, the odd lane iteration 1's: pcg_jump to the two states that are read, pcg_output_f32, cosine_hemisphere) and exchange them; the loop draws
nothing.  The states are the same integers and the warp the same function of them, so no lane's arithmetic differs and the films must keep their bits.

  1. the kernel of kHeadlinePairFacts against the generic fused kernel on 1 x 1 crops of cornell_wall 16 x 16 x 64 at max_depth 4 -- ONE wave per film, so every film
     word is one atomic add onto zero and the film is reproducible (tests/test_flat_facts.py) -- under a tent of radius 1 and 0.75, at two corners, an edge and two
     interior pixels, two seeds: film bits, the statistics and the mask that ran.  Where the oracle says that paths of the crop end early (a lane that met at most one
     surface entered at most two of the three iterations, so pairs with one dead member occur), n_bounces < 3 n_paths is asserted of the GPU's count too;
  2. the fall-backs: max_depth 2, 3 (no or one sampling iteration) and 5 (three), a roulette that is reached, a second point light, antithetic time sampling -- the
     film keeps the bits of the switch-off film and the kernel that ran is the one such a frame took before the fact existed;
  3. a 16 x 16 x 64 frame through the new kernel against the oracle's film;
  4. the crops of 1 on the pattern-initialised library, in a child process;
  5. (no GPU) tests/pair_samples_check.cpp: pcg_jump<N> against N single steps, and the states and floats the kernel reads against a plain walk of six draws per
     iteration; the oracle's choice of the crops with early ends.

Scene.last_plan_kernel is what dtof_scene_last_plan_facts reports, every bit of it; Scene.last_plan_mask (the plan's constants: the facts and the shape fields, what the
tests of the older masks compare) is the same value without the pair bit, so a frame of the new kernel reads kHeadlineShapeFacts there.

Frames are launched in the headline's shape (DTOF_CHUNK_SEGS=0: one block per 512-lane segment), as tests/test_plan_facts.py explains."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

IMG_TOL = 5e-5            # tests/test_flat_facts.py, tests/test_device_film.py: relative to max|ref|; the lanes are bit-exact, only the float32 order of the film sums differs
NCPU = min(os.cpu_count() or 1, 16)
SWITCH = "DTOF_PLAN_FACTS"
HEADLINE_SHAPE = dict(DTOF_CHUNK_SEGS="0")
CSRC = os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc")
PATTERN_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_pattern.so")
STATS = ("n_paths", "n_bounces", "n_shadow_rays", "n_bounces_inline", "n_inline_iterations", "n_launches_trace", "n_launches_shade", "n_launches_shadow", "n_launches_first",
         "n_fused_splat_launches")
INTEGRATOR = '\t<integrator type="dopplertofpath">\n'
SECOND_LIGHT = '\t<emitter type="point"><point name="position" x="0.4" y="1.6" z="0.3" /><rgb name="intensity" value="3" /></emitter>\n'
SPP = 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _masks():
    """(kHeadlineFusedFacts, kHeadlineShapeFacts, kHeadlinePairFacts, {fact name: bit}) as dtof_kernels.h defines them"""
    hdr = open(os.path.join(CSRC, "dtof_kernels.h")).read()
    bit = {m.group(1): int(m.group(2)) for m in re.finditer(r"(kFact\w+)\s*=\s*1u << (\d+)", hdr)}
    count_shift, wall_shift = (int(re.search(r"%s = (\d+)" % k, hdr).group(1)) for k in ("kFlatShapeCountShift", "kFlatShapeWallShift"))
    count, wall = (int(re.search(r"#define DTOF_HEADLINE_SHAPE_%s (\d+)" % k, hdr).group(1)) for k in ("COUNT", "WALL"))
    fused = int(re.search(r"#define DTOF_HEADLINE_FACTS (0x[0-9a-f]+)", hdr).group(1), 16) | 1 << bit["kFactFusedSplat"]
    shape = fused | int(re.search(r"#define DTOF_HEADLINE_C2 (0x[0-9a-f]+)", hdr).group(1), 16) | 1 << bit["kFactFlatShape"] | count << count_shift | wall << wall_shift
    return fused, shape, shape | 1 << bit["kFactPairSamples"], bit


FUSED_MASK, SHAPE_MASK, PAIR_MASK, FACT_BIT = _masks()


def _variant(xml, rfilter, crop, integrator_props="", second_light=False):
    """cornell_wall.xml with another tent radius, a 1 x 1 crop window, further properties of the integrator, a second point light"""
    assert xml.count('<rfilter type="tent" />') == 1 and xml.count('<string name="file_format"') == 1 and xml.count(INTEGRATOR) == 1 and xml.count("\t<emitter") == 1
    xml = xml.replace('<rfilter type="tent" />', {"tent": '<rfilter type="tent" />', "tent075": '<rfilter type="tent"><float name="radius" value="0.75" /></rfilter>'}[rfilter])
    if crop is not None:
        xml = xml.replace('<string name="file_format"', '<integer name="crop_offset_x" value="%d" /><integer name="crop_offset_y" value="%d" />'
                          '<integer name="crop_width" value="1" /><integer name="crop_height" value="1" /><string name="file_format"' % crop)
    if second_light:
        xml = xml.replace("\t<emitter", SECOND_LIGHT + "\t<emitter", 1)
    return xml.replace(INTEGRATOR, INTEGRATOR + integrator_props)


@pytest.fixture(scope="module")
def wall():
    """variants of scenes/cornell_wall.xml written next to it and removed afterwards"""
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(rfilter="tent", crop=None, integrator_props="", second_light=False):
        key = (rfilter, crop, integrator_props, second_light)
        if key not in made:
            made[key] = os.path.join(SCENES, "_pair_samples_%d_%d.xml" % (os.getpid(), len(made)))
            open(made[key], "w").write(_variant(base, rfilter, crop, integrator_props, second_light))
        return made[key]
    yield get
    for p in made.values():
        os.remove(p)


def _film_frame(sc, seed, spp):
    """one frame into a zeroed device film -> (film as numpy, stats, FACTS of the specialised first-bounce kernel it launched)"""
    import torch
    W, H = sc.size
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    st = sc.render_rows(film.data_ptr(), seed, spp, 0, H)
    return film.cpu().numpy(), st, sc.last_plan_kernel


def _on_and_off(sc, monkeypatch, seed, spp, what, kernel_on):
    """the frame with the switch off (twice: the film must be reproducible) and on; the switch-on frame must have launched the kernel of `kernel_on` (0: a generic one)
    -> (film off, film on, stats on)"""
    monkeypatch.setenv(SWITCH, "0")
    off_a, st_off, m_off = _film_frame(sc, seed, spp)
    off_b, _, _ = _film_frame(sc, seed, spp)
    assert np.isfinite(off_a).all() and np.abs(off_a[..., :3]).max() > 0 and (off_a[..., 3] > 0).all(), what
    assert np.array_equal(bits(off_a), bits(off_b)), (what, "the film chosen as reproducible is not", int((bits(off_a) != bits(off_b)).sum()))
    assert st_off["n_plan_facts_launches"] == 0 and m_off == 0 and st_off["n_launches_first"] == 1 and st_off["n_fused_splat_launches"] == 1, (what, st_off, hex(m_off))
    monkeypatch.setenv(SWITCH, "1")
    on, st_on, m_on = _film_frame(sc, seed, spp)
    assert st_on["n_plan_facts_launches"] == (1 if kernel_on else 0) and m_on == kernel_on, (what, st_on, hex(m_on), hex(kernel_on))
    for k in STATS:
        assert st_on[k] == st_off[k], (what, k, st_on[k], st_off[k])
    return off_a, on, st_on


def _bounce_bounds(osc, seed, spp):
    """(lower, upper) bound of the first-bounce kernel's n_bounces for the lanes of the oracle scene `osc` at max_depth 4, from the number of surfaces each lane met
    (`depth`): a lane enters iteration 0, and iteration i > 0 if it left a surface at i - 1 -- whether or not its ray then meets another.  A lane that met d surfaces
    entered d or d + 1 of the three iterations, at least one and at most three."""
    W, H = osc.size
    depth = osc.render_lanes(osc.params(), seed, spp, 0, W * H * spp, threads=NCPU)["depth"].astype(np.int64)
    return int(np.clip(depth, 1, 3).sum()), int(np.minimum(depth + 1, 3).sum())


# ---------------------------------------------------------------------------- without a GPU
def test_the_masks():
    """the pair fact sits above the shape fields; the new mask is kHeadlineShapeFacts and that bit"""
    assert FACT_BIT["kFactPairSamples"] == 26 and FACT_BIT["kFactFlatShape"] == 18
    assert SHAPE_MASK == 0x12fffff and PAIR_MASK == 0x52fffff and FUSED_MASK == 0x1fff


def test_stream_jumps_on_the_host(tmp_path):
    """pcg_jump<N> against N single steps, and the offsets k_shade reads against a plain six-draws-per-iteration walk (tests/pair_samples_check.cpp)"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"   # dtof_math.h includes the HIP headers (csrc/Makefile's HIPCC)
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc")
    exe = str(tmp_path / "pair_samples_check")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                           os.path.join(ROOT, "tests", "pair_samples_check.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    print(out.stdout)
    r = {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()}
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    assert r["jump_pairs"] == 10 ** 6 and r["jump_edge_cases"] == 12 and r["jump_checked"] == 12 * (10 ** 6 + 12) and r["streams"] == 10 ** 6
    for k in ("jump_mismatches", "jump6_mismatches", "bad_state", "bad_draw", "bad_loop_state", "bad_loop_draw"):
        assert r[k] == 0, (k, r[k])


CROPS = [("corner_0_0", (0, 0)), ("corner_15_15", (15, 15)), ("edge_15_3", (15, 3)), ("inside_5_9", (5, 9)), ("inside_11_12", (11, 12))]
CROP_CASES = [("%s_%s" % (f, n), f, c) for f in ("tent", "tent075") for n, c in CROPS]
SEEDS = (4, 11)


def test_the_oracle_finds_crops_whose_paths_end_early(orc, wall):
    """among the crops of 1 there is, for each seed, one where some lane meets at most one surface: its path ends before the third iteration while its pair's other
    member may go on (every crop is checked on the GPU against the same bound)"""
    for seed in SEEDS:
        early = []
        for name, crop in CROPS:
            lo, hi = _bounce_bounds(orc.Scene(wall("tent", crop), dict(resx=16, resy=16, max_depth=4)), seed, SPP)
            assert SPP <= lo <= hi <= 3 * SPP
            early.append(hi < 3 * SPP)
        print("seed %d: crops with early ends: %s" % (seed, [n for (n, _), e in zip(CROPS, early) if e]))
        assert any(early), seed


# ---------------------------------------------------------------------------- 1. one-pixel crops
@pytest.mark.gpu
@pytest.mark.parametrize("name,rfilter,crop", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_pair_kernel_film_of_a_one_pixel_crop_is_the_generic_fused_film(mi, orc, wall, monkeypatch, name, rfilter, crop):
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    path, params = wall(rfilter, crop), dict(resx=16, resy=16, max_depth=4)
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    assert sc.size == (1, 1) and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop
    for seed in SEEDS:
        what = (name, seed)
        off, on, st = _on_and_off(sc, monkeypatch, seed, SPP, what, PAIR_MASK)
        assert sc.last_plan_pair_samples and sc.last_plan_mask == SHAPE_MASK and sc.last_plan_shape == (5, 2), what
        assert np.array_equal(bits(on), bits(off)), (what, on, off)
        lo, hi = _bounce_bounds(osc, seed, SPP)
        print("%s seed %d: n_bounces %d of %d paths, oracle bounds [%d, %d], shadow rays %d" % (name, seed, st["n_bounces"], st["n_paths"], lo, hi, st["n_shadow_rays"]))
        assert st["n_paths"] == SPP and st["n_inline_iterations"] == 3 and lo <= st["n_bounces"] <= hi, (what, st, lo, hi)
        if hi < 3 * SPP:   # the oracle: paths of this crop end early
            assert st["n_bounces"] < 3 * st["n_paths"], (what, st)


# ---------------------------------------------------------------------------- 2. the fall-backs
PROP = '\t\t<integer name="%s" value="%d" />\n'
FALLBACKS = [
    # name, -D parameters, integrator properties, second light, FACTS of the kernel such a frame takes
    ("max_depth_2", dict(max_depth=2), "", False, SHAPE_MASK),          # one iteration: the terminal one
    ("max_depth_3", dict(max_depth=3), "", False, SHAPE_MASK),          # one sampling iteration
    ("max_depth_5", dict(max_depth=5), "", False, SHAPE_MASK),          # three sampling iterations
    ("roulette_at_2", dict(max_depth=4), PROP % ("rr_depth", 2), False, 0),   # kFactNoRoulette is a fact of every headline mask: the generic kernel
    ("two_point_lights", dict(max_depth=4), "", True, 0),               # so is kFactOneEmitter: e1 picks the light
    ("antithetic", dict(max_depth=4, time_sampling_method="antithetic"), "", False, FUSED_MASK),   # no stratified pairs: the kernel without the route facts
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FALLBACKS, ids=[c[0] for c in FALLBACKS])
def test_a_frame_without_the_fact_takes_the_kernel_it_took_before(mi, wall, monkeypatch, case):
    name, params, props, second_light, kernel = case
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for rfilter, crop in (("tent", (5, 9)), ("tent075", (0, 0))):
        sc = mi.load_file(wall(rfilter, crop, props, second_light), resx=16, resy=16, **params)
        off, on, _ = _on_and_off(sc, monkeypatch, 6, SPP, (name, rfilter, crop), kernel)
        assert not sc.last_plan_pair_samples, (name, rfilter, crop)
        assert np.array_equal(bits(on), bits(off)), (name, rfilter, crop, on, off)


# ---------------------------------------------------------------------------- 3. a frame against the oracle
@pytest.mark.gpu
def test_pair_kernel_frame_matches_the_oracle_film(mi, orc, monkeypatch):
    """cornell_wall 16 x 16 x 64 with the tent filter into a device film: one launch of the kernel of kHeadlinePairFacts; colour and weight within IMG_TOL of the oracle's film"""
    for k, v in dict(HEADLINE_SHAPE, **{SWITCH: "1"}).items():
        monkeypatch.setenv(k, v)
    path, params = os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16, max_depth=4)
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    got, st, kernel = _film_frame(sc, 5, SPP)
    assert kernel == PAIR_MASK and st["n_plan_facts_launches"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1 and st["n_paths"] == 16 * 16 * SPP, (st, hex(kernel))
    ref = osc.render(osc.params(), seed=5, spp=SPP, raw=True, threads=NCPU)[0]
    for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
        err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
        print("pair kernel, %s: %.3g of the largest value (bound %g)" % (name, err, IMG_TOL))
        assert err <= IMG_TOL, (name, err)


# ---------------------------------------------------------------------------- 4. the pattern-initialised build
@pytest.mark.gpu
def test_crop_cases_on_the_pattern_initialised_build():
    """the crops of 1 in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "one_pixel_crop"],
                       env=dict(os.environ, DTOF_LIB=PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
