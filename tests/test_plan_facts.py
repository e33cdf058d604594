"""The headline first-bounce kernel compiled with the frame plan's constants (k_shade's FACTS mask, dtof_kernels.h: kFact*) against the generic kernel, which
DTOF_PLAN_FACTS=0 restores.

A fact replaces a launch-uniform read -- rp.n_passes, rp.integrator, dbg, qin, rp.rr_depth, rp.chunk_blocks, ... -- by a constant; the host (FramePlan::launch_facts) sets the
fact only where the launch satisfies it, and the specialised kernel runs only when every fact of its mask is set.  No arithmetic that reaches a lane differs, so:

  * same bits: cornell_wall with a box filter and DTOF_FUSE_SPLAT=0 -- every film value is ONE atomic add of a fixed-order 64-sample reduction onto zero, so the film is
    reproducible bit for bit (shown by rendering it twice with the switch off) and must be the same bits with the switch on -- over max_depth, the time-sampling
    strategies, homodyne / heterodyne, the wave functions, and a frame whose lane count is not a multiple of 512;
  * the fused splat of the C2 shape against the oracle's film, within the tolerance tests/test_device_film.py holds;
  * every fact, broken alone, takes the generic kernel (the counters say which form ran), with the same bits where the film is reproducible and the oracle's lanes otherwise;
  * the resident Domino kernel of one film at 16 waves (C4) carries a mask of its own: the same bits, and the generic kernels for 12 waves, four films, one iteration;
  * the core cases against the pattern-initialised build, as tests/test_pattern_build.py runs the other kernels.

The frames here are small.  By default a frame of up to DTOF_CHUNK_SEGS segments whose whole path runs inline is launched as one block per 64-lane chunk, which is not the
headline launch (one block per segment) and breaks a fact by itself -- one of the fall-back cases; every other case sets DTOF_CHUNK_SEGS=0 to get the headline's launch shape."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES

IMG_TOL = 5e-5            # tests/test_device_film.py: relative to max|ref|; the lanes are bit-exact, only the float32 order of the film sums differs
NCPU = min(os.cpu_count() or 1, 16)
SWITCH = "DTOF_PLAN_FACTS"
STATS = ("n_paths", "n_bounces", "n_shadow_rays", "n_bounces_inline", "n_launches_trace", "n_launches_shade", "n_launches_shadow", "n_launches_first")
VARIANTS = [(1.0, 0.0), (1.0, 0.25), (0.0, 0.5), (2.0, 0.75)]
HEADLINE_SHAPE = dict(DTOF_CHUNK_SEGS="0")
PATTERN_LIB = os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof_pattern.so")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- without a GPU
def test_the_switch_is_read_by_the_frame_plan_and_listed_in_the_design_table():
    src = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "dtof_render.hip")).read()
    plan = src[src.index("FramePlan plan_frame("):src.index("void render_rows(")]
    assert 'on("%s")' % SWITCH in plan                      # per call, like the other development switches
    assert src.count('"%s"' % SWITCH) == 1                  # ... and nowhere else
    for name in ("dtof_kernels.hip", "dtof_shade.h", "dtof_shade_plain.hip", "dtof_kernels.h"):
        assert SWITCH not in open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", name)).read().replace("DTOF_PLAN_FACTS=0", ""), name   # (comments may name the switch-off form)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^\|\s*`%s`" % SWITCH, design, re.M), "DESIGN 5.35 lists every development switch of the frame path"


def test_the_counter_is_appended_to_the_statistics_block_and_mirrored():
    """existing offsets hold: the new field is the last one of dtof_render_stats and of its ctypes mirror"""
    import ctypes as C
    import mitsuba3dopplertof_amd as mi
    hdr = open(os.path.join(ROOT, "include", "dtof.h")).read()
    block = hdr[hdr.index("typedef struct {\n    uint64_t n_paths;"):hdr.index("} dtof_render_stats;")]
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", block, flags=re.S))
    assert fields[-2:] == ["n_fused_splat_launches", "n_plan_facts_launches"]
    assert [f[0] for f in mi._Stats._fields_] == fields
    assert mi._Stats.n_plan_facts_launches.offset == mi._Stats.n_fused_splat_launches.offset + 4 and C.sizeof(mi._Stats) % 8 == 0


def test_generic_instantiations_carry_no_fact():
    """FACTS defaults to 0 and only the headline instantiation names a mask"""
    csrc = os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc")
    assert "uint32_t FACTS = 0>" in open(os.path.join(csrc, "dtof_shade.h")).read()
    for name in os.listdir(csrc):
        if name.startswith("dtof_shade_") and name.endswith(".hip"):
            assert ("kHeadlineFacts" in open(os.path.join(csrc, name)).read()) == (name == "dtof_shade_plain.hip"), name


# ---------------------------------------------------------------------------- scenes
@pytest.fixture(scope="module")
def wall():
    """variants of scenes/cornell_wall.xml (or another generated scene) written next to it and removed afterwards: box filter (reproducible films), rr_depth, a second point light"""
    made = {}

    def get(box=True, rr_depth=None, two_lights=False, scene="cornell_wall.xml"):
        key = (box, rr_depth, two_lights, scene)
        if key not in made:
            xml = open(os.path.join(SCENES, scene)).read()
            if box:
                assert xml.count('<rfilter type="tent" />') == 1
                xml = xml.replace('<rfilter type="tent" />', '<rfilter type="box" />')
            if rr_depth is not None:
                line = '<integer name="max_depth" value="$max_depth" />'
                assert xml.count(line) == 1
                xml = xml.replace(line, line + '<integer name="rr_depth" value="%d" />' % rr_depth)
            if two_lights:
                xml = xml.replace("</scene>", '<emitter type="point"><point name="position" x="0.5" y="1.6" z="0.2" /><rgb name="intensity" value="3, 2, 1" /></emitter></scene>')
            made[key] = os.path.join(SCENES, "_plan_facts_%d_%s_rr%s_%s_%s" % (os.getpid(), "box" if box else "tent", rr_depth, "two" if two_lights else "one", scene))   # (the pattern-build child writes its own)
            open(made[key], "w").write(xml)
        return made[key]
    yield get
    for p in made.values():
        os.remove(p)


def _film_frame(sc, seed, spp, planes=1, **kw):
    """one frame into a zeroed device film -> (film as numpy, stats)"""
    import torch
    W, H = sc.size
    film = torch.zeros((planes, H, W, 4) if planes > 1 else (H, W, 4), dtype=torch.float32, device="cuda")
    stripes = kw.pop("stripes", None)
    st = sc.render_stripes(film.data_ptr(), seed, spp, *stripes, **kw) if stripes else sc.render_rows(film.data_ptr(), seed, spp, 0, H, **kw)
    return film.cpu().numpy(), st


def _same_stats(on, off, what):
    for k in STATS:
        assert on[k] == off[k], (what, k, on[k], off[k])


# ---------------------------------------------------------------------------- same bits
BASE = dict(resx=16, resy=8)
SAME_BITS = [("depth%d" % d, dict(BASE, max_depth=d)) for d in (2, 3, 4)]
SAME_BITS += [("time_" + m, dict(BASE, time_sampling_method=m)) for m in ("stratified", "antithetic", "antithetic_mirror", "uniform")]
SAME_BITS += [("hetero_%g" % f, dict(BASE, hetero_frequency=f)) for f in (0.0, 1.0)]
SAME_BITS += [("wave_" + w, dict(BASE, wave_function_type=w)) for w in ("sinusoidal", "rectangular", "trapezoidal")]
SAME_BITS += [("ragged_12x5", dict(resx=12, resy=5)), ("ragged_12x5_mirror_rect", dict(resx=12, resy=5, time_sampling_method="antithetic_mirror", wave_function_type="rectangular"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,params", SAME_BITS, ids=[c[0] for c in SAME_BITS])
def test_reproducible_film_is_the_same_bits_with_and_without_the_plan_facts(mi, wall, monkeypatch, name, params):
    for k, v in dict(HEADLINE_SHAPE, DTOF_FUSE_SPLAT="0").items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(wall(), **params)
    spp, seed = 64, 3
    monkeypatch.setenv(SWITCH, "0")
    off_a, st_off = _film_frame(sc, seed, spp)
    off_b, _ = _film_frame(sc, seed, spp)
    assert np.isfinite(off_a).all() and np.abs(off_a[..., :3]).max() > 0 and (off_a[..., 3] > 0).all(), name
    assert np.array_equal(bits(off_a), bits(off_b)), (name, "the film chosen as reproducible is not", int((bits(off_a) != bits(off_b)).sum()))
    assert st_off["n_plan_facts_launches"] == 0 and st_off["n_launches_first"] == 1 and st_off["n_fused_splat_launches"] == 0, st_off
    monkeypatch.setenv(SWITCH, "1")
    on, st_on = _film_frame(sc, seed, spp)
    assert st_on["n_plan_facts_launches"] == 1 and st_on["n_launches_first"] == 1, st_on      # the specialised form ran
    assert np.array_equal(bits(on), bits(off_a)), (name, int((bits(on) != bits(off_a)).sum()), float(np.abs(on - off_a).max()))
    _same_stats(st_on, st_off, name)
    if name.startswith("ragged"):
        assert st_on["n_paths"] % 512 != 0


# ---------------------------------------------------------------------------- the resident Domino kernel (C4: one film, 16 waves per block)
RESIDENT = [("d64", dict(resx=48, resy=32), 64, {}, None, True), ("d128_rect", dict(resx=40, resy=24, wave_function_type="rectangular"), 128, {}, None, True),
            ("ragged_d64", dict(resx=13, resy=7), 64, {}, None, True),
            # ... and what it does not cover: 12 waves per block, four films, a launch of one iteration
            ("waves_12", dict(resx=48, resy=32), 64, dict(DTOF_RESIDENT="12"), None, False), ("four_variants", dict(resx=48, resy=32), 64, {}, VARIANTS, False),
            ("inline_iters_1", dict(resx=48, resy=32), 64, dict(DTOF_INLINE_ITERS="1"), None, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", RESIDENT, ids=[c[0] for c in RESIDENT])
def test_resident_kernel_film_is_the_same_bits_with_and_without_the_plan_facts(mi, wall, monkeypatch, case):
    """domino.xml through the resident first-bounce kernel, box filter, the splat kernel: reproducible films, the same bits with the switch in either position; the
    specialised instantiation (k_shade<..., RESW = 16, kResidentFacts>) runs for one film at 16 waves when every fact holds, the generic ones otherwise"""
    name, params, spp, env, variants, specialised = case
    for k, v in dict(dict(HEADLINE_SHAPE, DTOF_FUSE_SPLAT="0", DTOF_PIPELINE="fused"), **env).items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(wall(scene="domino.xml"), **params)
    kw = dict(planes=4, variants=variants) if variants else {}
    monkeypatch.setenv(SWITCH, "0")
    off_a, st_off = _film_frame(sc, 3, spp, **dict(kw))
    off_b, _ = _film_frame(sc, 3, spp, **dict(kw))
    assert np.isfinite(off_a).all() and np.abs(off_a[..., :3]).max() > 0, name
    assert np.array_equal(bits(off_a), bits(off_b)), (name, "the film chosen as reproducible is not", int((bits(off_a) != bits(off_b)).sum()))
    monkeypatch.setenv(SWITCH, "1")
    on, st_on = _film_frame(sc, 3, spp, **dict(kw))
    assert st_off["n_plan_facts_launches"] == 0 and st_on["n_plan_facts_launches"] == (1 if specialised else 0) and st_on["n_launches_first"] == 1, (name, st_on)
    assert np.array_equal(bits(on), bits(off_a)), (name, int((bits(on) != bits(off_a)).sum()))
    _same_stats(st_on, st_off, name)


# ---------------------------------------------------------------------------- the fused splat
@pytest.mark.gpu
def test_fused_splat_frame_of_the_c2_shape_matches_the_oracle_film(mi, orc, monkeypatch):
    """cornell_wall at 64 samples per pixel with the tent filter into a device film, the switch on: ONE launch of the specialised kernel runs the whole path and splats its
    lanes itself.  Colour and weight channels each within IMG_TOL of their largest value against the oracle's film."""
    for k, v in dict(HEADLINE_SHAPE, **{SWITCH: "1"}).items():
        monkeypatch.setenv(k, v)
    path, params, spp = os.path.join(SCENES, "cornell_wall.xml"), dict(resx=40, resy=32), 64
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    got, st = _film_frame(sc, 5, spp)
    assert st["n_plan_facts_launches"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1 and st["n_paths"] == 40 * 32 * spp, st
    ref = osc.render(osc.params(), seed=5, spp=spp, raw=True, threads=NCPU)[0]
    for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
        err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
        print("fused splat, %s: %.3g of the largest value (bound %g)" % (name, err, IMG_TOL))
        assert err <= IMG_TOL, (name, err)


# ---------------------------------------------------------------------------- every fact, broken alone, falls back
# (id, scene variant, -D parameters, spp, integrator, sampler, environment, frame keywords)
FALLBACK = [
    ("two_passes", dict(), dict(BASE), 128, dict(type="dopplertofpath", max_depth=4, path_correlation_depth=4, hetero_frequency=1.0, samples_per_pass=64), None, {}, {}),
    ("rr_depth_2", dict(rr_depth=2), dict(BASE), 64, None, None, {}, {}),
    ("path_correlation_depth_1", dict(), dict(BASE, max_depth=4, path_correlation_depth=1), 64, None, None, {}, {}),
    ("independent_sampler", dict(), dict(BASE), 64, None, dict(type="independent", sample_count=64), {}, {}),
    ("path_integrator", dict(), dict(BASE), 64, dict(type="path", max_depth=4), None, {}, {}),
    ("two_point_lights", dict(two_lights=True), dict(BASE), 64, None, None, {}, {}),
    ("spp_48", dict(), dict(BASE), 48, None, None, {}, {}),
    ("stripes", dict(), dict(BASE), 64, None, None, {}, dict(stripes=(1, 2, 4))),
    ("four_variants", dict(), dict(BASE), 64, None, None, {}, dict(planes=4, variants=VARIANTS)),
    ("inline_iters_1", dict(), dict(BASE), 64, None, None, dict(DTOF_INLINE_ITERS="1"), {}),
    ("terminal_form_off", dict(), dict(BASE), 64, None, None, dict(DTOF_TERMINAL_SKIP="0"), {}),
    ("one_block_per_chunk", dict(), dict(BASE), 64, None, None, dict(DTOF_CHUNK_SEGS="8192"), {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FALLBACK, ids=[c[0] for c in FALLBACK])
def test_a_launch_that_breaks_one_fact_takes_the_generic_kernel(mi, orc, wall, monkeypatch, case):
    name, variant, params, spp, integ, sampler, env, kw = case
    for k, v in dict(dict(HEADLINE_SHAPE, DTOF_FUSE_SPLAT="0"), **env).items():
        monkeypatch.setenv(k, v)
    path = wall(**variant)
    sc = mi.load_file(path, **params)
    if integ is not None:
        sc.set_integrator(integ)
    if sampler is not None:
        sc.set_sampler(sampler)
    seed = 6
    monkeypatch.setenv(SWITCH, "0")
    off_a, st_off = _film_frame(sc, seed, spp, **dict(kw))
    off_b, _ = _film_frame(sc, seed, spp, **dict(kw))
    monkeypatch.setenv(SWITCH, "1")
    on, st_on = _film_frame(sc, seed, spp, **dict(kw))
    assert st_on["n_plan_facts_launches"] == 0 and st_off["n_plan_facts_launches"] == 0 and st_on["n_launches_first"] >= 1, (name, st_on)   # the generic form, silently
    assert sc.plan_facts_launches == 0, name
    assert np.isfinite(on).all() and np.abs(on[..., :3]).max() > 0, name
    _same_stats(st_on, st_off, name)
    if np.array_equal(bits(off_a), bits(off_b)):       # a reproducible film: the same bits with the switch in either position
        assert np.array_equal(bits(on), bits(off_a)), (name, int((bits(on) != bits(off_a)).sum()))
    else:                                              # its atomics land in no fixed order: the lanes are the oracle's, as tests/test_gpu_parity.py holds them
        osc = orc.Scene(path, params)
        pd = osc.params(**{k: v for k, v in (("integrator", integ), ("sampler", sampler)) if v is not None})
        W, H = sc.size
        n = W * H * spp
        g, o = sc.sample_lanes(seed, spp, 0, n), osc.render_lanes(pd, seed, spp, 0, n, threads=NCPU)
        for f in ("sample_pos", "time", "ray_d", "rgb"):
            assert np.array_equal(bits(g[f]), bits(o[f])), (name, f, int((bits(g[f]) != bits(o[f])).sum()))
        assert sc.plan_facts_launches == 0, name


@pytest.mark.gpu
def test_a_lane_dump_takes_the_generic_kernel_and_equals_the_oracle(mi, orc, wall, monkeypatch):
    """dtof_sample_lanes asks for the camera rays and valid_ray of its lanes: the launch writes what the specialised kernel has compiled out.  It returns no statistics
    block; the scene's own count of specialised launches says which form ran -- it moves for a frame and stands still for the dump."""
    for k, v in dict(HEADLINE_SHAPE, DTOF_FUSE_SPLAT="0").items():
        monkeypatch.setenv(k, v)
    path, params, spp, seed = wall(), dict(BASE), 64, 6
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    n = 16 * 8 * spp
    o = osc.render_lanes(osc.params(), seed, spp, 0, n, threads=NCPU)
    for v in ("1", "0"):
        monkeypatch.setenv(SWITCH, v)
        before = sc.plan_facts_launches
        g = sc.sample_lanes(seed, spp, 0, n)
        assert sc.plan_facts_launches == before, v
        for f in ("sample_pos", "time", "ray_d", "rgb"):
            assert np.array_equal(bits(g[f]), bits(o[f])), (v, f, int((bits(g[f]) != bits(o[f])).sum()))
        _film_frame(sc, seed, spp)
        assert sc.plan_facts_launches == before + (1 if v == "1" else 0), v


# ---------------------------------------------------------------------------- the pattern-initialised build
@pytest.mark.gpu
def test_core_cases_on_the_pattern_initialised_build():
    """the same-bits cases and the fused splat in a child process whose library starts every uninitialised automatic variable as a NaN / 0xAA pattern"""
    if os.environ.get("DTOF_LIB"):
        pytest.skip("already running against a library variant")
    if not os.path.exists(PATTERN_LIB):
        pytest.skip("libdtof_pattern.so is not built (make -C mitsuba3dopplertof_amd/csrc pattern)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k", "same_bits or fused_splat or lane_dump"],
                       env=dict(os.environ, DTOF_LIB=PATTERN_LIB), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
