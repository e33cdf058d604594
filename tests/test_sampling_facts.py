"""The route facts of C2's first-bounce kernel (k_shade's FACTS mask, dtof_kernels.h: kFactStratifiedPairs, kFactPow2Strata, kFactSineLowPass, kFactEmitterSampled,
kFactIdShift24, and the lane shifts kFactWavePixel proves) against the generic kernels, which DTOF_PLAN_FACTS=0 restores.

Under the facts generate_lane seeds no time stream and takes pair, member, pixel and sample index of a lane by shifts and masks, next_time is its stratified route
with the straight-line Kensler permutation of a power-of-two stratum count, and modulation_weight is the low-pass weight of the sinusoidal wave.  Each replaces a
launch-uniform decision by its value or an integer expression by an identical one: no lane's arithmetic differs, so the films must keep their bits.

  1. the kernel of kHeadlineC2Facts against the generic fused kernel on 1 x 1 crops of cornell_wall 16 x 16 x 64 -- ONE wave per film, so every film word is one atomic
     add onto zero and the film is reproducible (tests/test_flat_facts.py) -- under a tent of radius 1 and 0.75, at two corners, an edge and two interior pixels,
     max_depth 2, 3 and 4, two seeds.  A crop holds the sample indices 0 .. 63 of its pixel: every one of the 32 strata and both members of every pair.
     dtof_scene_last_plan_facts says that the new kernel ran;
  2. each new fact broken alone takes the kernel of kHeadlineFusedFacts (mask 0x1fff) and the film keeps the bits of the switch-off film;
  3. a 16 x 16 x 64 frame through the new kernel against the oracle's film;
  4. the crops of 1 on the pattern-initialised library, in a child process;
  5. (no GPU) the integer identities, swept on the host: tests/sampling_facts_check.cpp compiles permute_kensler and permute_kensler_pow2 from dtof_math.h against each
     other for n = 2 .. 4096, every index, 10^4 seeds, and the shifts and masks against the fdiv forms for every lane of a 16 x 16 x 64 frame.

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
STATS = ("n_paths", "n_bounces", "n_shadow_rays", "n_bounces_inline", "n_launches_trace", "n_launches_shade", "n_launches_shadow", "n_launches_first", "n_fused_splat_launches")
INTEGRATOR = '\t<integrator type="dopplertofpath">\n'


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _masks():
    """(kHeadlineFusedFacts, kHeadlineC2Facts, {fact name: bit}) as dtof_kernels.h defines them"""
    hdr = open(os.path.join(CSRC, "dtof_kernels.h")).read()
    bit = {m.group(1): int(m.group(2)) for m in re.finditer(r"(kFact\w+)\s*=\s*1u << (\d+)", hdr)}
    headline = int(re.search(r"#define DTOF_HEADLINE_FACTS (0x[0-9a-f]+)", hdr).group(1), 16)
    fused = headline | 1 << bit["kFactFusedSplat"]
    return fused, fused | int(re.search(r"#define DTOF_HEADLINE_C2 (0x[0-9a-f]+)", hdr).group(1), 16), bit


FUSED_MASK, C2_MASK, FACT_BIT = _masks()


def _variant(xml, rfilter, crop, integrator_props=""):
    """cornell_wall.xml with another tent radius, a 1 x 1 crop window and further properties of the integrator"""
    assert xml.count('<rfilter type="tent" />') == 1 and xml.count('<string name="file_format"') == 1 and xml.count(INTEGRATOR) == 1
    xml = xml.replace('<rfilter type="tent" />', {"tent": '<rfilter type="tent" />', "tent075": '<rfilter type="tent"><float name="radius" value="0.75" /></rfilter>'}[rfilter])
    if crop is not None:
        xml = xml.replace('<string name="file_format"', '<integer name="crop_offset_x" value="%d" /><integer name="crop_offset_y" value="%d" />'
                          '<integer name="crop_width" value="1" /><integer name="crop_height" value="1" /><string name="file_format"' % crop)
    return xml.replace(INTEGRATOR, INTEGRATOR + integrator_props)


@pytest.fixture(scope="module")
def wall():
    """variants of scenes/cornell_wall.xml written next to it and removed afterwards"""
    made = {}
    base = open(os.path.join(SCENES, "cornell_wall.xml")).read()

    def get(rfilter="tent", crop=None, integrator_props=""):
        key = (rfilter, crop, integrator_props)
        if key not in made:
            made[key] = os.path.join(SCENES, "_sampling_facts_%d_%d.xml" % (os.getpid(), len(made)))
            open(made[key], "w").write(_variant(base, rfilter, crop, integrator_props))
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
    return film.cpu().numpy(), st, sc.last_plan_facts


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


# ---------------------------------------------------------------------------- without a GPU
def test_the_masks():
    """the route facts sit on bits 13 and up; the C2 mask is kHeadlineFusedFacts and every one of them, the two older masks are what they were"""
    assert [FACT_BIT[k] for k in ("kFactStratifiedPairs", "kFactPow2Strata", "kFactSineLowPass", "kFactEmitterSampled", "kFactIdShift24")] == [13, 14, 15, 16, 17]
    assert FUSED_MASK == 0x1fff and C2_MASK == 0x3ffff and C2_MASK & FUSED_MASK == FUSED_MASK


def test_integer_identities_on_the_host(tmp_path):
    """the straight-line Kensler form against permute_kensler, and the shifts and masks against the fdiv forms (tests/sampling_facts_check.cpp)"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"   # dtof_math.h includes the HIP headers (csrc/Makefile's HIPCC)
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc")
    exe = str(tmp_path / "sampling_facts_check")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                           os.path.join(ROOT, "tests", "sampling_facts_check.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe, "10000", "16", "16", "64"], capture_output=True, text=True, timeout=300, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    print(out.stdout)
    r = {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()}
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    assert r["kensler_sizes"] == 12 and r["kensler_seeds"] == 10000 and r["kensler_evaluated"] == 8190 * 10000
    assert r["kensler_mismatches"] == 0 and r["kensler_not_permutation"] == 0
    assert r["lanes"] == 16 * 16 * 64
    for k in ("bad_pix", "bad_si", "bad_quo", "bad_rem", "bad_pair", "bad_wave"):
        assert r[k] == 0, (k, r[k])


# ---------------------------------------------------------------------------- 1. one-pixel crops
CROPS = [("corner_0_0", (0, 0)), ("corner_15_15", (15, 15)), ("edge_15_3", (15, 3)), ("inside_5_9", (5, 9)), ("inside_11_12", (11, 12))]
CROP_CASES = [("%s_%s" % (f, n), f, c) for f in ("tent", "tent075") for n, c in CROPS]


@pytest.mark.gpu
@pytest.mark.parametrize("name,rfilter,crop", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_c2_kernel_film_of_a_one_pixel_crop_is_the_generic_fused_film(mi, wall, monkeypatch, name, rfilter, crop):
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for max_depth in (2, 3, 4):
        sc = mi.load_file(wall(rfilter, crop), resx=16, resy=16, max_depth=max_depth)
        assert sc.size == (1, 1) and (sc.info()["crop_x"], sc.info()["crop_y"]) == crop
        for seed in (4, 11):
            what = (name, max_depth, seed)
            off, on = _on_and_off(sc, monkeypatch, seed, 64, what, C2_MASK)
            assert np.array_equal(bits(on), bits(off)), (what, on, off)


# ---------------------------------------------------------------------------- 2. each new fact broken alone
FALSE = '\t\t<boolean name="%s" value="false" />\n'
BROKEN = [
    ("uniform", dict(time_sampling_method="uniform"), ""),
    ("antithetic", dict(time_sampling_method="antithetic"), ""),
    ("antithetic_mirror", dict(time_sampling_method="antithetic_mirror"), ""),
    ("no_interval_stratification", {}, FALSE % "use_stratified_sampling_for_each_interval"),
    ("time_correlate_number_4", dict(time_correlate_number=4), ""),
    ("rectangular", dict(wave_function_type="rectangular"), ""),
    ("triangular", dict(wave_function_type="triangular"), ""),
    ("trapezoidal", dict(wave_function_type="trapezoidal"), ""),
    ("full_spectrum", {}, FALSE % "low_frequency_component_only"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BROKEN, ids=[c[0] for c in BROKEN])
def test_a_frame_that_breaks_one_route_fact_takes_the_fused_kernel_without_them(mi, wall, monkeypatch, case):
    name, params, props = case
    for k, v in HEADLINE_SHAPE.items():
        monkeypatch.setenv(k, v)
    for rfilter, crop in (("tent", (5, 9)), ("tent075", (0, 0))):
        sc = mi.load_file(wall(rfilter, crop, props), resx=16, resy=16, **params)
        off, on = _on_and_off(sc, monkeypatch, 6, 64, (name, rfilter, crop), FUSED_MASK)
        assert np.array_equal(bits(on), bits(off)), (name, rfilter, crop, on, off)


# ---------------------------------------------------------------------------- 3. a frame against the oracle
@pytest.mark.gpu
def test_c2_kernel_frame_matches_the_oracle_film(mi, orc, monkeypatch):
    """cornell_wall 16 x 16 x 64 with the tent filter into a device film: one launch of the kernel of kHeadlineC2Facts; colour and weight within IMG_TOL of the oracle's film"""
    for k, v in dict(HEADLINE_SHAPE, **{SWITCH: "1"}).items():
        monkeypatch.setenv(k, v)
    path, params, spp = os.path.join(SCENES, "cornell_wall.xml"), dict(resx=16, resy=16), 64
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    got, st, mask = _film_frame(sc, 5, spp)
    assert mask == C2_MASK and st["n_plan_facts_launches"] == 1 and st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1 and st["n_paths"] == 16 * 16 * spp, (st, hex(mask))
    ref = osc.render(osc.params(), seed=5, spp=spp, raw=True, threads=NCPU)[0]
    for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
        err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
        print("C2 kernel, %s: %.3g of the largest value (bound %g)" % (name, err, IMG_TOL))
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
