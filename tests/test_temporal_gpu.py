"""The denoiser's temporal stage on the device (csrc/dtof_temporal.hip through dtof_denoise_temporal_async and dtof_denoise_temporal), held to tests/temporal_ref.py.

  criterion  EVERY output word of every pixel -- o_colour, o_variance, o_length, o_colour_f32 -- EQUALS the reference bit for bit: the definition has only IEEE
             double + - * /, floor, min / max and comparisons in a fixed order, and the build's rule is -ffp-contract=off.  The sentinel margins around all four
             outputs are untouched, and an output that was not asked for is not written.
  shapes     W x H: 1 x 1, 2 x 2, 7 x 5, 65 x 9 (crosses a wave's 64 lanes, and a 256-lane block) and 130 x 3.
  cases      every shape meets K = 1 .. 4, every subset of {variance, normals, ids} -- all 32 instantiations of the kernel -- with and without a history; the
             flow kind rotates with the case so that every (K, subset) with a history meets five of the six kinds over the shapes, and K = 4 with all guides
             meets all six on the two larger shapes.  Flow kinds: zero; integer shifts; fractional; pointing outside on every side; +-1e30; fractional with a
             NaN or an infinity in about 5 % of the pixels.
  inputs     signed colours scaled by 10^U(-3, 2); about 5 % of the pixels carry a NaN or an infinity in one colour, variance or guide word, and as many history
             pixels in one history word; variances of 0 and -1; history lengths 0, max_length, NaN and +inf among the ordinary ones; id edges and normal edges
             through the image, the history's shifted by a pixel, its normals perturbed around the threshold.  No finite input is large enough for a sum to
             overflow, so no NaN is ever GENERATED and every NaN in an output is a converted input word, whose bits the conversion keeps.
  further    the host entry gives the async entry's bits; three chained frames through mi.Denoiser(temporal=True) equal temporal_ref followed by denoise_ref,
             the latter within the bound of test_denoise_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import SCENES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as R  # noqa: E402
import temporal_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

WALL = os.path.join(SCENES, "cornell_wall.xml")
MARGIN = 64
SENT = -7.5e11      # representable in float32 too
SHAPES = ((1, 1), (2, 2), (7, 5), (65, 9), (130, 3))      # W x H
FLOWS = ("zero", "integer", "fractional", "outside", "huge", "specials")
PARAMS = dict(alpha_min=0.125, max_length=6.0, tau_normal=0.25)
SPECIALS = (np.nan, np.inf, -np.inf)
BUFFERS = ("colour", "variance", "normal", "ids", "flow", "h_colour", "h_variance", "h_normal", "h_ids", "h_length", "o_colour", "o_variance", "o_length", "o_colour_f32")


def make_flow(rng, kind, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "zero":
        return np.zeros((h, w, 2), np.float32)
    if kind == "integer":
        return rng.integers(-2, 3, (h, w, 2)).astype(np.float32)
    if kind == "outside":      # the reprojected position leaves the image on the left, right, top and bottom, by less than a pixel and by many
        side = rng.integers(0, 4, (h, w))
        far = rng.choice([0.25, 1.0, 1.5, 40.0], (h, w))
        fx = np.where(side == 0, xx + far, np.where(side == 1, xx - (w - 1) - far, rng.uniform(-1, 1, (h, w))))
        fy = np.where(side == 2, yy + far, np.where(side == 3, yy - (h - 1) - far, rng.uniform(-1, 1, (h, w))))
        return np.stack([fx, fy], axis=2).astype(np.float32)
    if kind == "huge":
        return rng.choice(np.array([1e30, -1e30, 0.5], np.float32), (h, w, 2))
    f = rng.uniform(-2.5, 2.5, (h, w, 2)).astype(np.float32)
    if kind == "specials":
        for y, x in zip(*np.nonzero(rng.random((h, w)) < 0.05)):
            f[y, x, rng.integers(2)] = SPECIALS[rng.integers(3)]
        f[0, 0, 1] = np.nan
    return f


def make_inputs(seed, k, w, h, flow_kind):
    """the current frame and a history, every buffer present (the caller drops what its case leaves out)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    scale = 10.0 ** rng.uniform(-3, 2, ((h + 2) // 3, (w + 4) // 5))[yy // 3, xx // 5]
    colour = (rng.standard_normal((k, h, w, 3)) * scale[None, :, :, None]).astype(np.float32)
    variance = scale[None] ** 2 * rng.uniform(0.2, 2.0, (k, h, w))
    pick = rng.random((k, h, w))
    variance = np.where(pick < 0.04, 0.0, np.where(pick < 0.06, -1.0, variance))
    h_colour = rng.standard_normal((k, h, w, 3)) * scale[None, :, :, None]
    h_variance = scale[None] ** 2 * rng.uniform(0.05, 1.0, (k, h, w))
    # regions with an edge through the middle of each axis; the history's edges lie a pixel further, so the taps next to an edge meet the other surface
    region = (xx >= (w + 1) // 2).astype(int) + 2 * (yy >= (h + 1) // 2)
    h_region = (xx >= (w + 1) // 2 + 1).astype(int) + 2 * (yy >= (h + 1) // 2 + 1)
    normals = rng.standard_normal((4, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    normal = normals[region].astype(np.float32)
    # perturbations around the threshold: |d| = 0.25 U(0.5, 1.5) in a random direction, so about half of the same-surface taps pass the normal test
    d = rng.standard_normal((h, w, 3))
    d *= (PARAMS["tau_normal"] * rng.uniform(0.5, 1.5, (h, w)) / np.linalg.norm(d, axis=2))[..., None]
    h_normal = (normals[h_region] + np.where(rng.random((h, w, 1)) < 0.5, d, 0.0)).astype(np.float32)
    ids = (region + 1).astype(np.float32)
    h_ids = (h_region + 1).astype(np.float32)
    h_length = rng.integers(0, int(PARAMS["max_length"]) + 1, (h, w)).astype(np.float32)
    pick = rng.random((h, w))
    h_length = np.where(pick < 0.02, np.nan, np.where(pick < 0.04, np.inf, h_length)).astype(np.float32)
    for y, x in zip(*np.nonzero(rng.random((h, w)) < 0.05)):      # one special word per chosen pixel of the current frame
        which, value = rng.integers(4), SPECIALS[rng.integers(3)]
        if which == 0:
            colour[rng.integers(k), y, x, rng.integers(3)] = value
        elif which == 1:
            variance[rng.integers(k), y, x] = value
        elif which == 2:
            normal[y, x, rng.integers(3)] = value
        else:
            ids[y, x] = value
    for y, x in zip(*np.nonzero(rng.random((h, w)) < 0.05)):      # ... and of the history
        which, value = rng.integers(4), SPECIALS[rng.integers(3)]
        if which == 0:
            h_colour[rng.integers(k), y, x, rng.integers(3)] = value
        elif which == 1:
            h_variance[rng.integers(k), y, x] = value
        elif which == 2:
            h_normal[y, x, rng.integers(3)] = value
        else:
            h_ids[y, x] = value
    return {"colour": colour, "variance": variance, "normal": normal, "ids": ids, "flow": make_flow(rng, flow_kind, w, h),
            "h_colour": h_colour, "h_variance": h_variance, "h_normal": h_normal, "h_ids": h_ids, "h_length": h_length}


def select(inputs, mask, history):
    """the buffers of a case: mask 1 variance, 2 normals, 4 ids"""
    use = dict(inputs)
    for bit, name in ((1, "variance"), (2, "normal"), (4, "ids")):
        if not mask & bit:
            use[name] = use["h_" + name] = None
    if not history:
        for name in ("h_colour", "h_variance", "h_normal", "h_ids", "h_length"):
            use[name] = None
    return use


def reference(use):
    hist = None if use["h_colour"] is None else {"colour": use["h_colour"], "variance": use["h_variance"], "normal": use["h_normal"], "ids": use["h_ids"],
                                                 "length": use["h_length"]}
    return T.temporal(use["colour"], use["flow"], use["variance"], use["normal"], use["ids"], hist, **PARAMS)


@pytest.fixture(scope="module")
def torch_scene(mi):
    """a scene whose library calls are enqueued on torch's current stream: torch.cuda.synchronize() then waits for them"""
    import torch
    sc = mi.load_file(WALL, resx=8, resy=8)
    sc.set_stream(torch.cuda.current_stream().cuda_stream)
    yield sc
    torch.cuda.synchronize()
    sc.set_stream(None)


def run_async(mi, sc, use, want_f32=True):
    """dtof_denoise_temporal_async on torch's stream -> dict of the four outputs (None where not asked for); asserts the sentinel margins"""
    import torch
    k, h, w = use["colour"].shape[:3]
    dev = {n: None if use[n] is None else torch.from_numpy(np.ascontiguousarray(use[n])).cuda() for n in BUFFERS[:10]}
    sizes = {"o_colour": (k * h * w * 3, torch.float64), "o_variance": (k * h * w, torch.float64), "o_length": (h * w, torch.float32), "o_colour_f32": (k * h * w * 3, torch.float32)}
    outs = {n: torch.full((count + 2 * MARGIN,), SENT, dtype=dtype, device="cuda") for n, (count, dtype) in sizes.items()}
    asked = {"o_colour": True, "o_variance": use["variance"] is not None, "o_length": True, "o_colour_f32": want_f32}
    ptrs = [None if dev[n] is None else dev[n].data_ptr() for n in BUFFERS[:10]]
    ptrs += [outs[n].data_ptr() + MARGIN * outs[n].element_size() if asked[n] else None for n in BUFFERS[10:]]
    buf, prm = mi._TemporalBuffers(*ptrs), mi._TemporalParams(PARAMS["alpha_min"], PARAMS["max_length"], PARAMS["tau_normal"])
    torch.cuda.synchronize()
    rc = mi._lib().dtof_denoise_temporal_async(sc._h, C.byref(buf), k, w, h, C.byref(prm))
    assert rc == 0, mi._lib().dtof_last_error()
    torch.cuda.synchronize()
    got = {}
    for n, (count, _) in sizes.items():
        a = outs[n].cpu().numpy()
        body, margin = a[MARGIN:MARGIN + count], np.concatenate([a[:MARGIN], a[MARGIN + count:]])
        assert (margin == a.dtype.type(SENT)).all(), "a sentinel margin of %s was written" % n
        if not asked[n]:
            assert (body == a.dtype.type(SENT)).all(), "%s was written without being asked for" % n
        got[n] = body if asked[n] else None
    shapes = {"o_colour": (k, h, w, 3), "o_variance": (k, h, w), "o_length": (h, w), "o_colour_f32": (k, h, w, 3)}
    return {n: None if a is None else a.reshape(shapes[n]) for n, a in got.items()}


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_equal_bits(got, ref, label):
    pairs = [("o_colour", ref["colour"]), ("o_length", ref["length"])]
    if ref["variance"] is not None:
        pairs.append(("o_variance", ref["variance"]))
    if got["o_colour_f32"] is not None:
        pairs.append(("o_colour_f32", ref["colour_f32"]))
        with np.errstate(all="ignore"):
            assert (raw(got["o_colour_f32"]) == raw(got["o_colour"].astype(np.float32))).all(), (label, "o_colour_f32 is o_colour rounded once")
    for name, want in pairs:
        g, r = got[name], np.ascontiguousarray(want)
        assert g.dtype == r.dtype and g.shape == r.shape, (label, name)
        differ = raw(g) != raw(r)
        assert not differ.any(), (label, name, "%d words differ, the first at %s: got %r, want %r" % (differ.sum(), tuple(np.argwhere(differ)[0]), g[differ][0], r[differ][0]))


@pytest.mark.parametrize("shape_index", range(len(SHAPES)))
def test_every_instantiation_equals_the_reference_bit_for_bit(mi, torch_scene, shape_index):
    w, h = SHAPES[shape_index]
    accepted, rejected, anew, invalid = 0, 0, 0, 0
    for k in range(1, 5):
        for mask in range(8):
            for history in (False, True):
                kind = FLOWS[(k + mask + 3 * history + shape_index) % len(FLOWS)]
                use = select(make_inputs(10000 * shape_index + 100 * k + 10 * mask + history, k, w, h, kind), mask, history)
                ref = reference(use)
                got = run_async(mi, torch_scene, use, want_f32=(k + mask) % 2 == 0)
                assert_equal_bits(got, ref, "%dx%d K %d guides %d history %d flow %s" % (w, h, k, mask, history, kind))
                if history:
                    accepted += int(ref["accepted"].sum())
                    rejected += int((4 - ref["accepted"]).sum())
                    anew += int(((ref["accepted"] == 0) & (ref["length"] == 1)).sum())
                invalid += int((ref["length"] == 0).sum())
    print("%dx%d: %d taps accepted, %d rejected, %d valid pixels without history, %d invalid pixels" % (w, h, accepted, rejected, anew, invalid))
    if w * h >= 35:      # the cases decide something
        assert accepted > 0 and rejected > 0 and anew > 0 and invalid > 0


@pytest.mark.parametrize("shape_index", [3, 4])
@pytest.mark.parametrize("kind", FLOWS)
def test_all_guides_meet_every_flow_kind_and_the_host_entry(mi, torch_scene, shape_index, kind):
    """K = 4 with every guide and a history -- the configuration behind a velocity map -- under each flow kind; then the same bits through dtof_denoise_temporal"""
    w, h = SHAPES[shape_index]
    k = 4
    use = select(make_inputs(77 + shape_index, k, w, h, kind), 7, True)
    ref = reference(use)
    got = run_async(mi, torch_scene, use)
    label = "%dx%d flow %s" % (w, h, kind)
    assert_equal_bits(got, ref, label)
    if kind in ("zero", "integer", "fractional", "specials"):
        assert (ref["accepted"] > 0).any() and (ref["accepted"] < 4).any(), label
        assert (ref["length"] == np.float32(PARAMS["max_length"])).any() and (ref["length"] == 0).any(), label
    if kind == "huge":
        half = (use["flow"] == np.float32(0.5)).all(axis=2)      # only the lanes whose flow is (0.5, 0.5) reach their neighbours; 1e30 reaches nothing
        assert half.any() and (ref["accepted"][~half] == 0).all() and (ref["length"][~half] <= 1).all(), label
    host = {"o_colour": np.full((k, h, w, 3), SENT), "o_variance": np.full((k, h, w), SENT), "o_length": np.full((h, w), SENT, np.float32),
            "o_colour_f32": np.full((k, h, w, 3), SENT, np.float32)}
    arrays = dict(use, **host)
    buf = mi._TemporalBuffers(*(np.ascontiguousarray(arrays[n]).ctypes.data for n in BUFFERS))
    prm = mi._TemporalParams(PARAMS["alpha_min"], PARAMS["max_length"], PARAMS["tau_normal"])
    assert mi._lib().dtof_denoise_temporal(C.byref(buf), k, w, h, C.byref(prm)) == 0, mi._lib().dtof_last_error()
    for n in host:
        assert (raw(host[n]) == raw(got[n])).all(), (label, n, "the host entry computes the async entry's bits")


def test_three_chained_frames_through_the_python_class(mi):
    """mi.Denoiser(temporal=True): the history it hands on equals temporal_ref bit for bit, frame after frame (each frame's reference is fed the reference's own
    history), and what it returns is denoise_ref of the accumulated images and variances within the bound of test_denoise_gpu.py"""
    import test_denoise_gpu as D
    w, h, k, levels = 65, 9, 4, 3
    sigmas = dict(sigma_normal=0.3, sigma_position=2.5, sigma_luminance=4.0)
    den = mi.Denoiser((w, h), normals=True, position=True, variance=True, levels=levels, temporal=True, ids=True, **sigmas, **PARAMS)
    history, ref_history = None, None
    for frame in range(3):
        a = make_inputs(500 + frame, k, w, h, ("fractional", "integer", "specials")[frame])
        if frame == 0:
            surfaces = a["normal"].copy()
        a["normal"] = np.where(np.isfinite(a["normal"]), surfaces, a["normal"])      # the same surfaces in every frame; each frame keeps its own special words
        position = np.random.default_rng(frame).uniform(-1, 1, (h, w, 3)).astype(np.float32)
        out, var, history = den(a["colour"], normals=a["normal"], position=position, variance=a["variance"], flow=a["flow"], ids=a["ids"], history=history)
        ref = T.temporal(a["colour"], a["flow"], a["variance"], a["normal"], a["ids"], ref_history, **PARAMS)
        ref_history = {"colour": ref["colour"], "variance": ref["variance"], "length": ref["length"], "normal": a["normal"], "ids": a["ids"]}
        label = "frame %d" % frame
        for name in ("colour", "variance", "length"):
            assert (raw(history[name]) == raw(ref[name])).all(), (label, name)
        assert (raw(history["normals"]) == raw(a["normal"])).all() and (raw(history["ids"]) == raw(a["ids"])).all(), label
        if frame:
            assert (ref["accepted"] > 0).any() and (ref["length"] > 1).any(), label
        spatial = R.denoise(ref["colour_f32"], ref["variance"], a["normal"], position, levels=levels, **sigmas)
        assert out.shape == (k, h, w, 3) and var.shape == (k, h, w)
        worst = D.check_against_reference(out, var, spatial, ref["colour_f32"], ref["variance"], label)
        print("%s: %d pixels with a history, spatial stage at %.3g of its bound" % (label, int((ref["accepted"] > 0).sum()), worst))


def test_temporal_velocity_map_on_the_moving_wall(mi):
    """The moving wall of test_denoise_gpu.py's velocity-map check (512 spp in one pass, max_depth 2) at 64 x 64: four frames of the same scene with the seeds
    0, 64, 128, 192 through harness.TemporalVelocityMap, the flow from Scene.render_flow.  Over the pixels whose shape_index is the wall's, the spread about the
    mean of the temporally and spatially denoised map after frame four is below that of frame one's spatially denoised map, and every pixel's history length is
    in [1, 4]."""
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(WALL, resx=64, resy=64)
    sc.set_integrator(harness.doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, max_depth=2))
    index = sc.render_aovs("s:shape_index", seed=0, spp=64)["s"]
    wall = np.abs(index - np.round(index[32, 32])) < 1e-6
    assert 400 < wall.sum() < 64 * 64
    tvm = harness.TemporalVelocityMap((0.0, 0.25), 0.0015, 30)
    spreads = []
    for frame, seed in enumerate((0, 64, 128, 192)):
        noisy, spatial, temporal = tvm.frame(sc, 1, 512, seed=seed)
        assert noisy.shape == spatial.shape == temporal.shape == (64, 64)
        length = tvm.history["length"]
        spreads.append((float(np.std(noisy[wall])), float(np.std(spatial[wall])), float(np.std(temporal[wall]))))
        print("frame %d: spread over %d wall pixels: noisy %.6g, spatial %.6g, temporal + spatial %.6g; history length %g .. %g, on the wall %g .. %g; largest |flow| %.4g pixels"
              % (frame + 1, int(wall.sum()), *spreads[-1], length.min(), length.max(), length[wall].min(), length[wall].max(), np.nanmax(np.abs(tvm.details["flow"]))))
        assert (length >= 1).all() and (length <= frame + 1).all()
    assert (tvm.history["length"][wall] > 1).any()      # the wall does take its history
    assert spreads[3][2] < spreads[0][1]
