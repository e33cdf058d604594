"""The terminal form of the last bounce iteration (k_shade: RenderParams::terminal) against the full form, which DTOF_TERMINAL_SKIP=0 restores.

An iteration is terminal when nothing continues any path after it: no further iteration runs, the render has one pass, and the scene has no null lobe that could
still change valid_ray.  The terminal form drops the half of the bounce whose outputs nobody reads -- BSDF sampling, the draws behind the emitter sample, the
continuation ray, throughput / russian roulette, the advance of both streams, the survivor count -- and in the diffuse-only kernels the tangent frame.  Whatever
reaches a lane's result, its valid flag, a film or a statistic must be the same bits in both forms:

  * lane dumps (every lane, every field, `valid` included) over the kernel families, both pipelines, DTOF_INLINE_ITERS 1 and 4, max_depth 1, 2, 3, 4 and 6, russian
    roulette active at the terminal depth, four films per traversal and the resident first-bounce kernels.  A lane dump asks for valid_ray, which keeps the last
    iteration of a scene without surface emitters alive: these reach the terminal form WITHOUT emitter sampling (the emitter-hit iteration);
  * films, for the terminal form WITH emitter sampling (the last iteration that runs when the emitter-hit iteration is skipped): a box filter at 2 samples per pixel
    adds at most two terms to a film value, whose float sum does not depend on their order, so the film is reproducible bit for bit -- shown by rendering it twice
    with the switch off -- and must then be the same bits with the switch on;
  * the C2 shape (64 samples per pixel, tent filter: the first-bounce kernel splats its lanes itself) against the oracle's film, within the tolerance of
    tests/test_device_film.py;
  * a render of several passes never takes the terminal form: its lanes and its image equal the oracle's with the switch in either position;
  * n_bounces, n_shadow_rays and n_bounces_inline are the same in both forms."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SCENES

IMG_TOL = 5e-5            # tests/test_device_film.py: relative to max|ref|; the lanes are bit-exact, only the float32 order of the film sums differs
NCPU = min(os.cpu_count() or 1, 16)
SWITCH = "DTOF_TERMINAL_SKIP"
STATS = ("n_paths", "n_bounces", "n_shadow_rays", "n_bounces_inline", "n_inline_iterations", "n_launches_shade", "n_launches_first", "n_fused_splat_launches")
VARIANTS = [(1.0, 0.0), (1.0, 0.25), (0.0, 0.5), (2.0, 0.75)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rel_linf(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


# ---------------------------------------------------------------------------- without a GPU: the switch is read where the frame is planned, and documented
def test_the_switch_is_read_by_the_frame_plan_and_listed_in_the_design_table():
    src = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "dtof_render.hip")).read()
    plan = src[src.index("FramePlan plan_frame("):src.index("void render_rows(")]
    assert 'on("%s")' % SWITCH in plan                      # per call, like the other development switches
    assert src.count('"%s"' % SWITCH) == 1                  # ... and nowhere else
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^\|\s*`%s`" % SWITCH, design, re.M), "DESIGN 5.35 lists every development switch of the frame path"


def test_the_terminal_flag_travels_in_the_render_parameters():
    """the host decides (launch plan), the kernel reads a uniform flag: no environment access and no scene test on the device side"""
    hdr = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "dtof_kernels.h")).read()
    params = hdr[hdr.index("struct RenderParams {"):hdr.index("struct Queues {")]
    assert re.search(r"int32_t terminal;", params) and re.search(r"float emitter_pmf;", params)
    shade = open(os.path.join(ROOT, "mitsuba3dopplertof_amd", "csrc", "dtof_shade.h")).read()
    assert "rp.terminal" in shade and "sv.n_emitters ? 1.f /" not in shade     # m_emitter_pmf is no longer divided per lane


# ---------------------------------------------------------------------------- scenes
def _with_rr(xml, rr_depth):
    """rr_depth into the integrator of a generated scene"""
    line = '<integer name="max_depth" value="$max_depth" />'
    assert xml.count(line) == 1
    return xml.replace(line, line + '<integer name="rr_depth" value="%d" />' % rr_depth)


def _box(xml):
    assert xml.count('<rfilter type="tent" />') == 1
    return xml.replace('<rfilter type="tent" />', '<rfilter type="box" />')


@pytest.fixture(scope="module")
def scene_file():
    """variants of the generated scenes, written next to them (meshes and textures are found relative to the file) and removed afterwards"""
    made = {}

    def get(name, rr_depth=None, box=False):
        if rr_depth is None and not box:
            return os.path.join(SCENES, name)
        key = (name, rr_depth, box)
        if key not in made:
            xml = open(os.path.join(SCENES, name)).read()
            if rr_depth is not None:
                xml = _with_rr(xml, rr_depth)
            if box:
                xml = _box(xml)
            made[key] = os.path.join(SCENES, "_terminal_%s_rr%s_%s" % ("box" if box else "tent", rr_depth, name))
            open(made[key], "w").write(xml)
        return made[key]
    yield get
    for p in made.values():
        os.remove(p)


FUSED, SPLIT = dict(DTOF_PIPELINE="fused"), dict(DTOF_PIPELINE="split")
INLINE1, INLINE4 = dict(DTOF_INLINE_ITERS="1"), dict(DTOF_INLINE_ITERS="4")


def resident(waves):
    return dict(DTOF_PIPELINE="fused", DTOF_CHUNK_SEGS="0", DTOF_RESIDENT=str(waves))


def _settings():
    for pipe in (FUSED, SPLIT):
        for inl in ((INLINE1, INLINE4) if pipe is FUSED else (INLINE4,)):     # the split pipeline has no inline iterations
            yield dict(pipe, **inl)


# (id, scene, -D parameters, spp, rr_depth or None, settings).  max_depth 1, 2, 3, 4, 6 on the point-light rectangle scene and on the area-light scene; rr_depth at or
# below the terminal depth; the kernel families: plain, plain + area, mesh (boxes, spheres / disk with their lights), every-BSDF without (rough) and with (masked: never
# terminal) a null lobe, blend; the resident first-bounce kernels (Domino, reduced)
LANE_CASES = []
for depth in (1, 2, 3, 4, 6):
    for s in _settings():
        LANE_CASES.append(("wall_d%d" % depth, "cornell_wall.xml", dict(resx=32, resy=24, max_depth=depth), 8, None, s))
        LANE_CASES.append(("area_d%d" % depth, "cornell_area.xml", dict(resx=24, resy=24, max_depth=depth), 8, None, s))
for s in _settings():
    LANE_CASES += [
        ("wall_d4_rr2", "cornell_wall.xml", dict(resx=32, resy=24, max_depth=4), 8, 2, s),
        ("wall_d3_rr1", "cornell_wall.xml", dict(resx=32, resy=24, max_depth=3), 8, 1, s),
        ("area_d4_rr3", "cornell_area.xml", dict(resx=24, resy=24, max_depth=4), 8, 3, s),
        ("area_d5_rr2", "cornell_area.xml", dict(resx=24, resy=24, max_depth=5), 8, 2, s),
        ("boxes_d4", "cornell_boxes.xml", dict(resx=32, resy=32), 8, None, s),
        ("boxes_d3_rr2", "cornell_boxes.xml", dict(resx=32, resy=32, max_depth=3), 8, 2, s),
        ("sphere_light_d5", "cornell_sphere_light.xml", dict(resx=24, resy=24, max_depth=5), 8, None, s),
        ("disk_d3", "cornell_disk.xml", dict(resx=24, resy=24, max_depth=3), 8, None, s),
        ("masked_d4", "cornell_masked.xml", dict(resx=24, resy=24, max_depth=4), 8, None, s),
        ("rough_d3", "cornell_rough.xml", dict(resx=24, resy=24, max_depth=3), 8, None, s),
        ("plastic_d4_rr2", "cornell_plastic.xml", dict(resx=24, resy=24), 8, 2, s),
        ("blend_d4", "cornell_blend.xml", dict(resx=24, resy=24, max_depth=4), 8, None, s),
        ("env_d3", "cornell_env.xml", dict(resx=24, resy=24, max_depth=3), 8, None, s),
    ]
for waves in (12, 16):
    for depth in (2, 4):
        LANE_CASES.append(("domino_d%d" % depth, "domino.xml", dict(resx=48, resy=32, max_depth=depth), 4, None, resident(waves)))
LANE_CASES.append(("domino_d3_rr2", "domino.xml", dict(resx=48, resy=32, max_depth=3), 4, 2, resident(16)))
LANE_CASES.append(("domino_small_d4", "domino_small.xml", dict(resx=32, resy=32), 4, None, FUSED))


def _lane_id(c):
    return c[0] + "-" + "-".join("%s=%s" % (k[5:].lower(), v) for k, v in sorted(c[5].items()))


def _both(monkeypatch, fn):
    """fn() with the terminal form (the default, stated) and without it"""
    out = []
    for v in ("1", "0"):
        monkeypatch.setenv(SWITCH, v)
        out.append(fn())
    return out


def _same_stats(on, off, what):
    for k in STATS:
        assert on[k] == off[k], (what, k, on[k], off[k])


@pytest.mark.gpu
@pytest.mark.parametrize("case", LANE_CASES, ids=[_lane_id(c) for c in LANE_CASES])
def test_lane_dump_is_the_same_bits_with_and_without_the_terminal_form(mi, scene_file, monkeypatch, case):
    name, scene, params, spp, rr_depth, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(scene_file(scene, rr_depth), **params)
    if rr_depth is not None:
        assert sc.info()["rr_depth"] == rr_depth
    w, h = sc.size
    n = w * h * spp
    on, off = _both(monkeypatch, lambda: sc.sample_lanes(2, spp, 0, n))
    # something is rendered -- except at max_depth 1 under a point light, where a path ends at its first vertex with the emitter-hit term alone: all zeros
    assert np.isfinite(off["rgb"]).all() and (np.abs(off["rgb"]).max() > 0) == (name != "wall_d1"), name
    for f in ("sample_pos", "time", "ray_o", "ray_d", "rgb"):
        assert np.array_equal(bits(on[f]), bits(off[f])), (name, f, int((bits(on[f]) != bits(off[f])).sum()))
    assert np.array_equal(on["valid"], off["valid"]), (name, "valid", int((on["valid"] != off["valid"]).sum()))
    # four films per traversal (K = 4 kernels): every film's lanes
    on4, off4 = _both(monkeypatch, lambda: sc.sample_lanes_variants(2, spp, 0, n, VARIANTS))
    assert on4["rgb"].shape == (4, n, 3) and np.array_equal(bits(on4["rgb"]), bits(off4["rgb"])), (name, "K = 4", int((bits(on4["rgb"]) != bits(off4["rgb"])).sum()))
    assert np.array_equal(on4["valid"], off4["valid"])
    # the statistics of the frame (a render, whose last iteration may be another one than the lane dump's: no valid_ray is asked for)
    def frame():
        sc.render(seed=2, spp=spp)
        return sc.last_stats
    s_on, s_off = _both(monkeypatch, frame)
    _same_stats(s_on, s_off, name)


# ---------------------------------------------------------------------------- films: the terminal form WITH emitter sampling (the emitter-hit iteration skipped)
FILM_CASES = []
for depth in (2, 3, 4, 6):
    for s in _settings():
        FILM_CASES.append(("wall_d%d" % depth, "cornell_wall.xml", dict(resx=48, resy=32, max_depth=depth), None, s))
for s in _settings():
    FILM_CASES += [
        ("wall_d4_rr3", "cornell_wall.xml", dict(resx=48, resy=32, max_depth=4), 3, s),
        ("wall_d4_rr1", "cornell_wall.xml", dict(resx=48, resy=32, max_depth=4), 1, s),
        ("boxes_d4", "cornell_boxes.xml", dict(resx=32, resy=32), None, s),
        ("boxes_d3_rr2", "cornell_boxes.xml", dict(resx=32, resy=32, max_depth=3), 2, s),
        ("plastic_d4", "cornell_plastic.xml", dict(resx=24, resy=24), None, s),
        ("rough_d3_rr2", "cornell_rough.xml", dict(resx=24, resy=24, max_depth=3), 2, s),
        ("area_d4", "cornell_area.xml", dict(resx=24, resy=24), None, s),
    ]
for waves in (12, 16):
    FILM_CASES.append(("domino_d4", "domino.xml", dict(resx=48, resy=32), None, resident(waves)))
FILM_CASES.append(("domino_d3_rr2", "domino.xml", dict(resx=48, resy=32, max_depth=3), 2, resident(16)))


def _film_id(c):
    return c[0] + "-" + "-".join("%s=%s" % (k[5:].lower(), v) for k, v in sorted(c[4].items()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", FILM_CASES, ids=[_film_id(c) for c in FILM_CASES])
def test_reproducible_film_is_the_same_bits_with_and_without_the_terminal_form(mi, scene_file, monkeypatch, case):
    name, scene, params, rr_depth, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = mi.load_file(scene_file(scene, rr_depth, box=True), **params)
    spp = 2                # a film value is the sum of at most two terms: the same float in either order
    stats = {}

    def frame(key, **kw):
        img = sc.render(seed=7, spp=spp, **kw)
        stats[key] = sc.last_stats
        return img
    for kw in (dict(), dict(variants=VARIANTS)):
        monkeypatch.setenv(SWITCH, "0")
        off_a, off_b = frame("off", **kw), frame("off", **kw)
        assert np.abs(off_a).max() > 0 and np.isfinite(off_a).all()
        assert np.array_equal(bits(off_a), bits(off_b)), (name, "the film chosen as reproducible is not", int((bits(off_a) != bits(off_b)).sum()))
        monkeypatch.setenv(SWITCH, "1")
        on = frame("on", **kw)
        assert np.array_equal(bits(on), bits(off_a)), (name, kw and "K = 4", int((bits(on) != bits(off_a)).sum()), rel_linf(on, off_a))
        _same_stats(stats["on"], stats["off"], name)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["1", "0"])
def test_fused_splat_frame_of_the_c2_shape_matches_the_oracle_film(mi, orc, monkeypatch, switch):
    """cornell_wall at 64 samples per pixel with the tent filter into a device film: one first-bounce launch runs the whole path and splats its lanes itself.  The
    RGBW film against the oracle's as tests/test_device_film.py holds a plane: colour and weight channels each within IMG_TOL of their largest value."""
    import torch
    monkeypatch.setenv(SWITCH, switch)
    path, params, spp = os.path.join(SCENES, "cornell_wall.xml"), dict(resx=40, resy=32), 64
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    W, H = sc.size
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    st = sc.render_rows(film.data_ptr(), 5, spp, 0, H)
    assert st["n_fused_splat_launches"] == 1 and st["n_launches_shade"] == 1 and st["n_paths"] == W * H * spp, st
    got = film.cpu().numpy()
    ref = osc.render(osc.params(), seed=5, spp=spp, raw=True, threads=NCPU)[0]
    for ch, name in ((slice(0, 3), "rgb"), (3, "W")):
        err = float(np.abs(np.asarray(got[..., ch], np.float64) - ref[..., ch]).max() / max(np.abs(ref[..., ch]).max(), 1e-30))
        assert err <= IMG_TOL, (switch, name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,max_depth", [("cornell_wall.xml", 4), ("cornell_area.xml", 3)])
def test_a_render_of_two_passes_never_takes_the_terminal_form(mi, orc, monkeypatch, scene, max_depth):
    """the streams of a finished path are what its lane starts the next pass with: every (pass, lane) and the image equal the oracle's, the switch in either position"""
    path, params, spp, per_pass = os.path.join(SCENES, scene), dict(resx=24, resy=16, max_depth=max_depth), 8, 4
    integ = dict(type="dopplertofpath", max_depth=max_depth, path_correlation_depth=2, time_sampling_method="antithetic", hetero_frequency=1.0, samples_per_pass=per_pass)
    sc, osc = mi.load_file(path, **params), orc.Scene(path, params)
    sc.set_integrator(integ)
    pd = osc.params(integrator=integ)
    wavefront = 24 * 16 * per_pass
    ref, n = osc.render(pd, seed=4, spp=spp, threads=NCPU)
    lanes = [osc.render_lanes(pd, 4, spp, k * wavefront, wavefront, threads=NCPU) for k in range(spp // per_pass)]
    stats = []
    for v in ("1", "0"):
        monkeypatch.setenv(SWITCH, v)
        for k, o in enumerate(lanes):
            g = sc.sample_lanes(4, spp, k * wavefront, wavefront)
            for f in ("sample_pos", "time", "ray_d", "rgb"):
                assert np.array_equal(bits(g[f]), bits(o[f])), (scene, v, "pass", k, f, int((bits(g[f]) != bits(o[f])).sum()))
            assert np.array_equal(g["valid"], o["valid"])
        img = sc.render(seed=4, spp=spp)
        stats.append(sc.last_stats)
        assert sc.last_stats["n_paths"] == n == 24 * 16 * spp and rel_linf(img, ref) <= IMG_TOL, (scene, v, rel_linf(img, ref))
    _same_stats(stats[0], stats[1], scene)
