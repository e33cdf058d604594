"""The flow film on the device (k_aov<LDS, FLOW = true>; dtof_sample_flow_lanes, dtof_render_flow; Scene.render_flow) against tests/flow_ref.py evaluated on the
ORACLE's hits (aov_ref.py: the oracle's lanes and its surface interaction per lane), with the keyframes from dtof_scene_export kind 0 and S from numpy
(test_flow_cpu.numpy_S), not from the entry under test.

PER LANE  out_lanes12 is bit for bit dtof_sample_lanes (and the oracle's lanes); out_flow2 is bit for bit flow_ref.py; misses and hits on objects with fewer than
          two keyframes are exactly +0.
FILM      for every raw plane and pixel |device - expected| <= moments_ref.BOUND * sum |term| (2^-40, the bound of test_aov_gpu.py) against the sums of the lanes'
          float32 terms over the footprints of moments_ref.py; the developed planes are held as test_aov_gpu.py holds its own.
S         an independent hold on S and on the whole chain: pix(p) of every hit lane's own hit position (the aov film's position lanes) is the lane's
          sample_pos.  Measured on the CPU with the oracle's lanes and numpy's S (test_flow_cpu.py): 3.52e-6 pixels (perspective), 2.08e-6 (orthographic), 1.78e-6 (perspective under a crop) -- the
          float32 rounding of the camera ray and of the hit.  8 x that is allowed here, with S from the entry.
Scenes at 16 x 16 x 4 spp unless said otherwise."""
import numpy as np
import pytest

import aov_ref as aref
import flow_ref as fref
import moments_ref as ref
from test_flow_cpu import SENSORS, numpy_S, pix
from test_moments_gpu import load

pytestmark = pytest.mark.gpu

SEED = 3
U32 = np.uint32
# id -> (scene, -D parameters, spp, edit, integrator override, what the case must contain)
CASES = {
    "wall": ("cornell_wall.xml", dict(resx=16, resy=16), 4, None, None, "moving"),                       # one translating instance; tent filter
    "domino_small": ("domino_small.xml", dict(resx=16, resy=16), 4, None, None, "moving"),               # many animated instances, rotation
    "boxes": ("cornell_boxes.xml", dict(resx=16, resy=16), 4, None, None, None),
    "open_veils": ("open_veils.xml", dict(resx=16, resy=16), 4, None, None, "misses"),
    "wall_box": ("cornell_wall.xml", dict(resx=16, resy=16), 4, "box", None, "moving"),
    "wall_crop": ("cornell_wall.xml", dict(resx=32, resy=24), 4, "crop", None, "moving alone"),          # a crop window at (5, 3) on the moving wall: S is in film pixels
    "wall_path": ("cornell_wall.xml", dict(resx=16, resy=16), 4, None, {"type": "path", "max_depth": 4}, "moving"),
    "wall_two_passes": ("cornell_wall.xml", dict(resx=16, resy=16), 8, None, dict(samples_per_pass=4), "moving"),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


def device_lanes(sc, osc, orc, pd, spp):
    w, h = osc.size
    spw, n_passes = ref.pass_layout(orc, osc, pd, spp)
    per = w * h * spw
    parts_f = [sc.sample_flow_lanes(SEED, spp, k * per, per) for k in range(n_passes)]
    parts_o = [sc.sample_lanes(SEED, spp, k * per, per) for k in range(n_passes)]
    cat = lambda parts, keys: {k: np.concatenate([p[k] for p in parts]) for k in keys}      # noqa: E731
    keys = ("sample_pos", "time", "ray_o", "ray_d", "rgb")
    return cat(parts_f, keys + ("flow",)), cat(parts_o, keys), n_passes


@pytest.mark.parametrize("case", list(CASES))
def test_lanes_and_film_against_the_definition(mi, orc, case):
    scene, params, spp, edit, override, must = CASES[case]
    sc, osc = load(mi, orc, scene, params, edit)
    integ = None
    if override:
        integ = override if "type" in override else ref.integrator_of(osc, **override)
        sc.set_integrator(integ)
    lanes, _, out25, ids, pd = aref.expected_lanes(orc, osc, "p:position", SEED, spp, integ)      # asserts the far-plane condition on the oracle's numbers
    hit = ids[:, 0] >= 0
    n_keys = np.array([o["n_keys"] for o in osc.flat.objects])
    S = numpy_S(sc.export(2), params["resx"], params["resy"])
    want = fref.flow(out25[:, 1:4], lanes["time"], np.where(hit, ids[:, 0], -1), n_keys, sc.export(0), S)
    got, own, n_passes = device_lanes(sc, osc, orc, pd, spp)
    for k in ("sample_pos", "time", "ray_o", "ray_d", "rgb"):
        assert (bits(got[k]) == bits(own[k])).all(), (case, k)
    for k in ("sample_pos", "time", "ray_o", "ray_d"):
        assert (bits(got[k]) == bits(lanes[k])).all(), (case, k)
    moving = hit & (n_keys[np.maximum(ids[:, 0], 0)] > 1)
    differ = (bits(got["flow"]) != bits(want)).any(axis=1)
    print("%s: %d lanes, %d hits, %d on moving objects, largest |flow| %.4g pixels, lanes that differ from the definition: %d" %
          (case, len(lanes), hit.sum(), moving.sum(), np.abs(want).max(), differ.sum()))
    assert not differ.any(), (case, got["flow"][differ][:4], want[differ][:4])
    assert (bits(got["flow"][~moving]) == 0).all(), "a miss or a static object must give exactly +0"
    assert np.isfinite(want).all()
    if must == "moving":
        assert moving.any() and (~moving).any() and np.abs(want[moving]).max() > 1e-3
    if must == "moving alone":
        assert moving.all() and np.abs(want).max() > 1e-3
    if must == "misses":
        assert (~hit).any() and hit.any()
    if case == "wall_two_passes":
        assert n_passes == 2
    # the film: the raw sums, then the developed form
    exp, mags = aref.expected_planes(orc, osc, lanes, want, pd, spp)
    flow, weight = sc.render_flow(SEED, spp, raw=True, weight=True)
    w, h = sc.size
    assert sc.last_stats["n_paths"] == w * h * spp and flow.shape == (h, w, 2) and flow.dtype == np.float64
    raw = np.stack([weight, flow[..., 0], flow[..., 1]])
    ratios = aref.errors_over_bound(raw, exp, mags)
    print("%s film: largest error / bound: weight %.3g, flow %.3g" % (case, ratios[0], ratios[1:].max()))
    assert (ratios <= 1.0).all() and (exp[0] != 0).any(), (case, ratios)
    assert not raw[1:][mags[1:] == 0.0].any()
    dflow, dweight = sc.render_flow(SEED, spp, weight=True)
    dev = np.stack([dweight, dflow[..., 0], dflow[..., 1]])
    assert (aref.errors_over_bound(dev[:1], exp[:1], mags[:1]) <= 1.0).all()      # the weight is never divided
    back = dev[1:] * np.where(dev[0] == 0.0, 1.0, dev[0])
    dratios = (np.abs(back - exp[1:]) - 2.0 ** -52 * np.abs(back)) / np.where(mags[1:] == 0.0, 1.0, ref.BOUND * mags[1:])
    print("%s developed: largest (|developed * W - expected| - 2^-52 |.|) / bound %.3g" % (case, dratios.max()))
    assert (dratios <= 1.0).all(), (case, dratios.max())


def test_two_passes_accumulate_into_one_film(mi, orc):
    sc, osc = load(mi, orc, "cornell_wall.xml", dict(resx=16, resy=16))
    multi, weight = sc.render_flow(SEED, 4, n_passes=2, raw=True, weight=True)
    assert sc.last_stats["n_paths"] == 2 * 16 * 16 * 4
    n_keys = np.array([o["n_keys"] for o in osc.flat.objects])
    S = numpy_S(sc.export(2), 16, 16)
    exp, mags = 0.0, 0.0
    for seed in (SEED, SEED + 1):
        lanes, _, out25, ids, pd = aref.expected_lanes(orc, osc, "p:position", seed, 4)
        want = fref.flow(out25[:, 1:4], lanes["time"], np.where(ids[:, 0] >= 0, ids[:, 0], -1), n_keys, sc.export(0), S)
        e, a = aref.expected_planes(orc, osc, lanes, want, pd, 4)
        exp, mags = exp + e, mags + a
    ratios = aref.errors_over_bound(np.stack([weight, multi[..., 0], multi[..., 1]]), exp, mags)
    print("2 passes against the oracle's seeds s, s + 1: largest error / bound %.3g" % ratios.max())
    assert (ratios <= 1.0).all() and np.abs(exp[1:]).max() > 0


@pytest.mark.parametrize("name,measured", [("perspective", 3.52e-6), ("orthographic", 2.08e-6), ("perspective, cropped", 1.78e-6)])
def test_every_hit_projects_onto_its_sample_position(mi, name, measured):
    """S of the entry and the device's own lanes: pix(hit position) is the lane's sample_pos within 8 x the deviation the oracle's lanes show on the CPU"""
    sc = mi.load_string(SENSORS[name])
    w, h = sc.size
    lanes = sc.sample_aov_lanes("p:position,d:depth", SEED, 8, 0, w * h * 8)
    hit = lanes["values"][:, 3] > 0
    assert hit.sum() > len(hit) // 4
    dev = np.abs(pix(sc.world_to_pixel(), lanes["values"][hit, :3]) - lanes["sample_pos"][hit].astype(np.float64))
    print("%s: %d hits, largest |pix(p) - sample_pos| %.3g pixels (CPU: %.3g)" % (name, int(hit.sum()), dev.max(), measured))
    assert dev.max() <= 8 * measured
    flow = sc.sample_flow_lanes(SEED, 8, 0, w * h * 8)["flow"]
    assert (bits(flow) == 0).all()      # nothing moves in this scene
