"""The denoised renders on the device (dtof_render_denoised, dtof_render_velocity_map_denoised, dtof_denoise_inputs_async; Scene.render_denoised_device,
Scene.render_velocity_map_denoised) on the GPU.

1. THE FUSED FILMS ARE THE FILMS.  One traversal renders the float64 film, the moment film and the aov film.  The raw moment and aov planes returned through `outputs`
   are held to expectations built from the oracle alone by the criterion of test_moments_gpu / test_aov_gpu (derived there): |device - expected| <= 2^-40 * sum |term|
   per plane and pixel; every pass's image to the oracle's order-independent image by test_film64_gpu's rel_linf_px <= 2^-23.  With the box filter at 1 spp a pixel
   takes one term per plane and pass, so the planes EQUAL those of separate render_moments / render_aovs calls.
2. THE TAIL IS NUMPY'S OF THE SAME FILMS.  tests/denoise_inputs_ref.py of the returned sum, moment planes and aov planes is the returned denoiser input bit for bit;
   dtof_denoise (the host-pointer entry: the same kernels, no atomics) of those inputs is the returned result bit for bit; calc_velocity_from_homo_heteros of the
   returned planes is the returned map bit for bit.
3. THE STAGE ON SYNTHETIC DEVICE BUFFERS, sentinel words around every buffer.
4. A scene with nothing in view.  5. The command line.
Shapes: the smallest at which the run reduction (4 spp: runs shorter than a wave; 24 x 16: more than one block), the tile halo (levels 5: step 16 on a 16-row image)
and the block reduction (n = 63, 64, 65: a wave's edge; 4097: 17 blocks, the last with one pixel) can go wrong."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_ref as aref
import denoise_inputs_ref as dref
import moments_ref as ref
from conftest import SCENES
from test_moments_gpu import K4, load, _xml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3
SPEC = "p:position,n:sh_normal"
IMG_BOUND = 2.0 ** -23      # test_film64_gpu.IMG_BOUND
NCPU = os.cpu_count() or 1
T, W_G = 0.0015, 30.0


def rel_linf_px(a, r, eps=1e-3):
    """test_film64_gpu.rel_linf_px"""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return float((np.abs(a - r) / np.maximum(np.abs(r), eps * max(np.abs(r).max(), 1e-30))).max())


# ---------------------------------------------------------------------------- 1. the fused films are the films
# id -> (-D parameters, spp, passes, edit, integrator override)
FILM_CASES = {
    "tent_24x16": (dict(resx=24, resy=16), 4, 2, None, None),
    "gaussian": (dict(resx=24, resy=16), 4, 2, "gaussian", None),                  # 5 x 5 footprint
    "crop": (dict(resx=32, resy=24), 4, 2, "crop", None),                          # a 16 x 12 window at (5, 3)
    "two_of_four_per_pass": (dict(resx=24, resy=16), 4, 2, None, dict(samples_per_pass=2)),
    "box_7x5_1spp": (dict(resx=7, resy=5, time_sampling_method="uniform"), 1, 2, "box", None),      # (1 spp: no per-interval stratification)
}


@pytest.mark.parametrize("case", list(FILM_CASES))
def test_fused_films_against_the_oracle(mi, orc, case):
    params, spp, n_passes, edit, override = FILM_CASES[case]
    sc, osc = load(mi, orc, "cornell_wall.xml", params, edit, override)
    w, h = sc.size
    r = sc.render_denoised_device(seed=SEED, spp=spp, n_passes=n_passes, variants=K4, details=True)
    assert sc.last_stats["n_paths"] == w * h * spp * n_passes, sc.last_stats      # one traversal per pass, not three
    assert r["moments"].shape == (mi.MOMENT_PLANES(4), h, w) and r["aovs"].shape == (7, h, w) and r["sum"].shape == (4, h, w, 3)
    integ = ref.integrator_of(osc, **override) if override else None
    want_m = mags_m = want_a = mags_a = 0.0
    for seed in range(SEED, SEED + n_passes):
        e, a = ref.expected_moments(orc, osc, seed, spp, variants=K4, override=override)
        want_m, mags_m = want_m + e, mags_m + a
        lanes, values, _, _, pd = aref.expected_lanes(orc, osc, SPEC, seed, spp, integ)
        e, a = aref.expected_planes(orc, osc, lanes, values, pd, spp)
        want_a, mags_a = want_a + e, mags_a + a
    ratios_m, ratios_a = ref.errors_over_bound(r["moments"], want_m, mags_m), aref.errors_over_bound(r["aovs"], want_a, mags_a)
    ref.report(case + " moment planes", ratios_m, 4)
    print("%s aov planes: largest error / bound: weight %.3g, channels %.3g" % (case, ratios_a[0], ratios_a[1:].max()))
    assert np.abs(want_m).max() > 0 and (want_m[0] > 0).any() and np.abs(want_a[1:]).max() > 0 and (want_a[0] != 0).any()
    assert (ratios_m <= 1.0).all(), (case, ratios_m)
    assert (ratios_a <= 1.0).all(), (case, ratios_a)
    # every pass's image: the float64 film's, against the oracle's order-independent image of every variant
    total = 0.0
    for seed in range(SEED, SEED + n_passes):
        one = sc.render_denoised_device(seed=seed, spp=spp, n_passes=1, variants=K4, details=True)
        assert sc.last_stats["n_paths"] == w * h * spp
        assert dref.same_bits(one["image"], one["sum"], nan_equal=True)      # one pass: x / 1.0f
        for k, (f, o) in enumerate(K4):
            pd = osc.params(integrator=ref.integrator_of(osc, hetero_frequency=float(np.float32(f)), hetero_offset=float(np.float32(o)), **(override or {})))
            exact, _ = osc.render_exact(pd, seed=seed, spp=spp, threads=NCPU)
            err = rel_linf_px(one["image"][k], exact)
            print("%s seed %d variant %d: image rel_linf_px %.3g (bound %.3g)" % (case, seed, k, err, IMG_BOUND))
            assert np.abs(exact).max() > 0 and err <= IMG_BOUND, (case, seed, k, err)
        total = one["sum"] if seed == SEED else total + one["sum"]
        magnitude = np.abs(one["sum"]).astype(np.float64) if seed == SEED else magnitude + np.abs(one["sum"])
    if case == "box_7x5_1spp":      # one term per pixel, plane and pass: nothing depends on an order
        assert dref.same_bits(r["sum"], total)
        m = sc.render_moments(SEED, spp, n_passes=n_passes, variants=K4, raw=True)
        from test_moments_gpu import planes_of
        assert dref.same_bits(r["moments"], planes_of(m)) and (r["moments"][0] == n_passes).all()
        g = sc.render_aovs(SPEC, SEED, spp, n_passes=n_passes, raw=True)
        separate = np.stack([g["weight"]] + [g["p"][..., c] for c in range(3)] + [g["n"][..., c] for c in range(3)])
        assert dref.same_bits(r["aovs"], separate)
    else:
        # the same passes, summed in float32 on either side, from films whose doubles differ in their order of additions: every pass image is off by at most one
        # float32 ulp (2^-23 of its magnitude), and the float32 additions round by 2^-24 of the sum on either side
        tol = 2.0 ** -23 * (magnitude + np.abs(total))
        excess = np.abs(r["sum"].astype(np.float64) - total.astype(np.float64)) / np.where(tol == 0.0, 1.0, tol)
        print("%s: sum of the passes against the passes' own sums: largest difference / bound %.3g" % (case, excess.max()))
        assert (excess <= 1.0).all() and not (r["sum"][tol == 0.0]).any()


def test_rgba_scene_renders_its_alpha_plane_and_leaves_it_out(mi):
    """the float64 film of an rgba scene has its alpha plane behind the K colour planes exactly as in a film64 + moments request; nothing of it is returned or denoised.
    Box filter, 1 spp: one term per pixel and plane, so the rgb scene's call returns the same words"""
    params = dict(resx=9, resy=7, time_sampling_method="uniform")
    rgb, rgba = mi.load_string(_xml("cornell_wall.xml", "box"), **params), mi.load_string(_xml("cornell_wall.xml", "box+rgba"), **params)
    assert rgba.info()["has_alpha"] and not rgb.info()["has_alpha"]
    a, b = (sc.render_denoised_device(seed=SEED, spp=1, variants=K4, details=True) for sc in (rgb, rgba))
    assert b["image"].shape == (4, 7, 9, 3) and np.abs(b["image"]).max() > 0
    for key in ("image", "sum", "moments", "aovs", "colour", "variance", "normal", "position", "denoised", "denoised_variance"):
        assert dref.same_bits(a[key], b[key], nan_equal=True), key
    assert a["sigma_position"] == b["sigma_position"]


@pytest.mark.parametrize("plugin", ["velocity", "path"])
def test_other_integrators_fill_the_fused_films(mi, plugin):
    """Without variants the entry takes any integrator (K = 1, its own image), as the host route does.  `velocity` has a kernel of its own in the bounce loop's place:
    it must run in a request that names the aov film AND a film.  Box filter, 2 spp (the replaced integrator keeps the sampler's per-interval stratification, which needs
    time_correlate_number samples): two terms per pixel and plane, and a + b is b + a, so the films equal those of the separate calls"""
    from test_moments_gpu import planes_of
    sc = mi.load_string(_xml("cornell_wall.xml", "box"), resx=9, resy=7)
    sc.set_integrator(dict(type=plugin))
    r = sc.render_denoised_device(seed=SEED, spp=2, details=True, levels=2)
    assert sc.last_stats["n_paths"] == 9 * 7 * 2
    assert r["sum"].shape == (1, 7, 9, 3) and np.abs(r["sum"]).max() > 0 and (r["moments"][0] == 2.0).all()
    assert dref.same_bits(r["moments"], planes_of(sc.render_moments(SEED, 2, raw=True)))
    assert np.abs(r["moments"][1:]).max() > 0
    assert dref.same_bits(r["sum"][0], sc.render(seed=SEED, spp=2, film="float64"))
    g = sc.render_aovs(SPEC, SEED, 2, raw=True)
    assert dref.same_bits(r["aovs"], np.stack([g["weight"]] + [g["p"][..., c] for c in range(3)] + [g["n"][..., c] for c in range(3)]))
    c, v, nrm, pos = dref.inputs(dref.IMAGE, r["sum"].reshape(1, 63, 3), r["moments"].reshape(-1, 63), r["aovs"].reshape(7, 63), 1, 2.0)
    assert dref.same_bits(r["colour"], c.reshape(1, 7, 9, 3), nan_equal=True) and dref.same_bits(r["variance"], v.reshape(7, 9), nan_equal=True)
    assert np.isfinite(r["denoised"]).all() and np.abs(r["denoised"]).max() > 0
    with pytest.raises(mi.DtofError, match="only apply to the dopplertofpath integrator"):
        sc.render_denoised_device(seed=SEED, spp=2, variants=K4)


# ---------------------------------------------------------------------------- 2. the tail is numpy's of the same films
def host_denoise(mi, colour, variance, normal, position, levels, sigma_normal, sigma_position, sigma_luminance):
    k, h, w = colour.shape[:3]
    prm = mi._abi._DenoiseParams(levels, sigma_normal, sigma_position, sigma_luminance)
    out, out_var = np.zeros((k, h, w, 3), np.float64), np.zeros((k, h, w), np.float64)
    rc = mi._lib().dtof_denoise(colour.ctypes.data, k, w, h, variance.ctypes.data, normal.ctypes.data, position.ctypes.data, C.byref(prm), out.ctypes.data, out_var.ctypes.data)
    assert rc == 0, mi._lib().dtof_last_error()
    return out, out_var


def check_tail(mi, mode, d, n_passes, n_samples, levels, sigma_position):
    """d: "sum", "moments", "aovs", "colour", "variance", "normal", "position", "denoised", "denoised_variance", "sigma_position" of one call"""
    K, h, w = d["sum"].shape[:3]
    n = h * w
    c, v, nrm, pos = dref.inputs(mode, d["sum"].reshape(K, n, 3), d["moments"].reshape(-1, n), d["aovs"].reshape(7, n), n_passes, n_samples, T)
    assert np.abs(c).max() > 0 and (v > 0).any() and np.abs(nrm).max() > 0 and np.abs(pos).max() > 0
    assert dref.same_bits(d["colour"], c.reshape(K, h, w, 3), nan_equal=True) and dref.same_bits(d["variance"], v.reshape(K, h, w), nan_equal=True)
    assert dref.same_bits(d["normal"], nrm.reshape(h, w, 3), nan_equal=True) and dref.same_bits(d["position"], pos.reshape(h, w, 3), nan_equal=True)
    want_sigma = dref.sigma_position(d["position"]) if sigma_position is None else sigma_position
    assert d["sigma_position"] == want_sigma and (sigma_position is not None or 0 < want_sigma < 1.0), (d["sigma_position"], want_sigma)
    out, out_var = host_denoise(mi, d["colour"], d["variance"], d["normal"], d["position"], levels, 0.1, d["sigma_position"], 4.0)
    assert dref.same_bits(d["denoised"], out, nan_equal=True) and dref.same_bits(d["denoised_variance"], out_var, nan_equal=True)
    assert (d["denoised"] != d["colour"].astype(np.float64)).any(), "the denoiser ran"


@pytest.mark.parametrize("sigma_position", [None, 0.25])
@pytest.mark.parametrize("levels", [1, 5])
def test_image_mode_tail_is_numpy_of_the_returned_films(mi, levels, sigma_position):
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    n_passes, spp = 2, 4
    r = sc.render_denoised_device(seed=SEED, spp=spp, n_passes=n_passes, variants=K4, details=True, levels=levels, sigma_position=sigma_position)
    n_samples = sc.last_stats["n_paths"] / float(24 * 16)
    assert n_samples == spp * n_passes
    d = dict(r)
    check_tail(mi, dref.IMAGE, d, n_passes, n_samples, levels, sigma_position)
    assert dref.same_bits(r["image"], r["sum"] / np.float32(n_passes), nan_equal=True) and dref.same_bits(r["image"], r["colour"], nan_equal=True)
    if levels == 5 and sigma_position is None:      # without variants: the integrator's own pair, the (H, W, ...) shapes of render_denoised
        one = sc.render_denoised_device(seed=SEED, spp=spp, n_passes=n_passes)
        assert one["image"].shape == (16, 24, 3) and one["denoised"].shape == (16, 24, 3) and one["variance"].shape == (16, 24) == one["denoised_variance"].shape
        assert set(one) == {"image", "denoised", "variance", "denoised_variance", "sigma_position"}


@pytest.mark.parametrize("sigma_position", [None, 0.25])
@pytest.mark.parametrize("levels", [1, 5])
def test_tof_mode_tail_and_maps_are_numpy_of_the_returned_films(mi, levels, sigma_position):
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    n_passes, spp = 2, 4
    noisy, denoised = sc.render_velocity_map_denoised(n_passes, spp, (0.0, 0.25), T, W_G, seed=SEED, details=True, levels=levels, sigma_position=sigma_position)
    n_samples = sc.last_stats["n_paths"] / float(24 * 16)
    assert sc.last_stats["n_paths"] == 24 * 16 * spp * n_passes
    d = sc.denoise_details
    check_tail(mi, dref.TOF, d, n_passes, n_samples, levels, sigma_position)
    assert (d["colour"][..., 0] == d["colour"][..., 1]).all() and (d["colour"][..., 0] == d["colour"][..., 2]).all()
    tof, den = d["colour"][..., 0], d["denoised"][..., 0]
    assert dref.same_bits(noisy, harness.calc_velocity_from_homo_heteros(list(tof[:2]), list(tof[2:]), T, W_G), nan_equal=True)
    assert dref.same_bits(denoised, harness.calc_velocity_from_homo_heteros(list(den[:2]), list(den[2:]), T, W_G), nan_equal=True)
    assert np.isfinite(noisy).all() and np.isfinite(denoised).all() and (noisy != denoised).any()
    assert dref.same_bits(np.stack(d["homodyne"] + d["heterodyne"]), tof) and dref.same_bits(np.stack(d["denoised_homodyne"] + d["denoised_heterodyne"]), den)
    if levels == 1 and sigma_position is None:      # the harness entry: run_scene_velocity_map's integrator dictionary, passes and seeds
        a = harness.run_scene_velocity_map_denoised_device(sc, spp, (0.0, 0.25), denoiser=dict(levels=1))
        assert a[0].shape == (16, 24) and np.isfinite(a[1]).all() and sc.last_stats["n_paths"] == 24 * 16 * spp
        assert set(sc.denoise_details) == {"homodyne", "heterodyne", "denoised_homodyne", "denoised_heterodyne", "variance", "denoised_variance", "sigma_position"}


# ---------------------------------------------------------------------------- 3. the stage on synthetic device buffers
MARGIN = 64
SENT32, SENT64, SENT_U = np.float32(-7.5e11), np.float64(-7.5e111), np.uint32(0xdeadbeef)


@pytest.fixture(scope="module")
def torch_scene(mi):
    """a scene whose library calls are enqueued on torch's current stream: torch.cuda.synchronize() then waits for them"""
    import torch
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=8, resy=8)
    sc.set_stream(torch.cuda.current_stream().cuda_stream)
    yield sc
    torch.cuda.synchronize()
    sc.set_stream(None)


def guarded(torch, host, sentinel):
    """a device copy of `host` (flat) between two margins of sentinel words -> (tensor, pointer to the payload)"""
    flat = np.ascontiguousarray(host).reshape(-1)
    full = np.concatenate([np.full(MARGIN, sentinel, flat.dtype), flat, np.full(MARGIN, sentinel, flat.dtype)])
    if full.dtype == np.uint32:
        t = torch.from_numpy(full.view(np.int32)).cuda()
    else:
        t = torch.from_numpy(full).cuda()
    return t, t.data_ptr() + MARGIN * t.element_size()


def split_margins(t, n, dtype):
    a = t.cpu().numpy().view(dtype)
    return a[MARGIN:MARGIN + n], np.concatenate([a[:MARGIN], a[MARGIN + n:]])


def synthetic_films(rng, K, n, kind):
    """(sum (K, n, 3) float32, moment cells (n, 32), aov cells (n, 32)) and the raw planes the cells hold"""
    P = 1 + 6 * K + K * (K - 1) // 2
    total = (rng.normal(0.0, 1.0, (K, n, 3)) * 3.0).astype(np.float32)
    moments = rng.normal(0.0, 1.0, (P, n))
    moments[0] = rng.uniform(0.5, 40.0, n)
    for k in range(K):
        moments[1 + 6 * k + 4] = moments[1 + 6 * k + 1] ** 2 / moments[0] + rng.uniform(-0.5, 3.0, n) * moments[0]      # some variances are negative
    aovs = rng.normal(0.0, 2.0, (7, n))
    aovs[0] = rng.uniform(0.5, 40.0, n)
    for i in rng.integers(0, n, max(n // 8, 1)):      # W == 0 pixels, NaN / Inf words
        what = rng.integers(0, 6)
        if what == 0:
            moments[:, i] = 0.0
            aovs[:, i] = 0.0
        elif what == 1:
            moments[0, i] = 0.0
            aovs[0, i] = 0.0
        elif what == 2:
            moments[1 + 6 * rng.integers(K) + rng.choice([1, 4]), i] = rng.choice([np.nan, np.inf, -np.inf])
        elif what == 3:
            aovs[rng.integers(1, 7), i] = rng.choice([np.nan, np.inf, -np.inf])
        elif what == 4:
            total[rng.integers(K), i, rng.integers(3)] = rng.choice([np.nan, np.inf, -np.inf]).astype(np.float32)
        else:
            aovs[0, i] = np.inf
    if kind == "extremes":      # the finite position extremes at the first and at the last pixel
        aovs[0, 0] = aovs[0, n - 1] = 2.0
        aovs[1:4, 0], aovs[1:4, n - 1] = (-200.0, 300.0, -400.0), (500.0, -600.0, 700.0)
    elif kind == "none_finite":
        aovs[1, :] = np.nan
    elif kind == "one_finite":
        aovs[2, :] = np.inf
        aovs[:, n // 2] = (4.0, 1.0, 2.0, 3.0, 0.0, 0.0, 4.0)
    cells_m, cells_a = np.full((n, 32), 9.75), np.full((n, 32), 9.75)      # the words of a cell no plane uses are never read
    cells_m[:, :P], cells_a[:, :7] = moments.T, aovs.T
    return total, cells_m, cells_a, moments, aovs


STAGE_CASES = [(n, K, "extremes") for n in (1, 63, 64, 65, 4097) for K in (1, 4)] + [(4097, 1, "random"), (65, 4, "none_finite"), (65, 1, "one_finite")]


@pytest.mark.parametrize("mode", [dref.IMAGE, dref.TOF])
@pytest.mark.parametrize("n,K,kind", STAGE_CASES)
def test_stage_on_synthetic_device_buffers(mi, torch_scene, n, K, kind, mode):
    import torch
    sc = torch_scene
    rng = np.random.default_rng(1000 * n + 10 * K + mode)
    total, cells_m, cells_a, moments, aovs = synthetic_films(rng, K, n, kind)
    n_passes, n_samples = 3, 12.0
    ins = [guarded(torch, total, SENT32), guarded(torch, cells_m, SENT64), guarded(torch, cells_a, SENT64)]
    outs = {"colour": guarded(torch, np.full(K * n * 3, SENT32, np.float32), SENT32), "variance": guarded(torch, np.full(K * n, SENT64), SENT64),
            "normal": guarded(torch, np.full(n * 3, SENT32, np.float32), SENT32), "position": guarded(torch, np.full(n * 3, SENT32, np.float32), SENT32),
            "extent": guarded(torch, np.full(8, SENT_U, np.uint32), SENT_U)}
    torch.cuda.synchronize()
    rc = mi._lib().dtof_denoise_inputs_async(sc._h, mode, ins[0][1], ins[1][1], ins[2][1], K, n, n_passes, n_samples, T, outs["colour"][1], outs["variance"][1],
                                             outs["normal"][1], outs["position"][1], outs["extent"][1])
    assert rc == 0, mi._lib().dtof_last_error()
    torch.cuda.synchronize()
    c, v, nrm, pos = dref.inputs(mode, total, moments, aovs, n_passes, n_samples, T)
    got = {}
    for key, count, dtype, sentinel in (("colour", K * n * 3, np.float32, SENT32), ("variance", K * n, np.float64, SENT64), ("normal", n * 3, np.float32, SENT32),
                                        ("position", n * 3, np.float32, SENT32), ("extent", 8, np.uint32, SENT_U)):
        got[key], margin = split_margins(outs[key][0], count, dtype)
        assert (margin == sentinel).all(), ("margin of " + key, n)
    for (t, _), count, dtype, sentinel, host in zip(ins, (K * n * 3, n * 32, n * 32), (np.float32, np.float64, np.float64), (SENT32, SENT64, SENT64), (total, cells_m, cells_a)):
        payload, margin = split_margins(t, count, dtype)
        assert (margin == sentinel).all() and dref.same_bits(payload, host.reshape(-1))      # the inputs are read only
    assert dref.same_bits(got["colour"], c.reshape(-1), nan_equal=True) and dref.same_bits(got["variance"], v.reshape(-1), nan_equal=True)
    assert dref.same_bits(got["normal"], nrm.reshape(-1), nan_equal=True) and dref.same_bits(got["position"], pos.reshape(-1), nan_equal=True)
    assert (v[np.isfinite(v)] < 0).any() or n < 8, "negative variances are among the inputs"
    lo, hi, count = dref.extent_words(pos)
    words = got["extent"]
    # the sign of a zero extreme is the one thing an order could change, and the extent does not read it: min and max are compared as values
    assert words[6] == count and words[7] == 0 and (words[0:3].view(np.float32) == lo).all() and (words[3:6].view(np.float32) == hi).all(), (words, lo, hi, count)
    finite = pos[np.isfinite(pos).all(axis=1)].astype(np.float64)
    extent = float((words[3:6].view(np.float32).astype(np.float64) - words[0:3].view(np.float32).astype(np.float64)).max()) if count else 0.0
    sigma = 0.01 * extent if extent > 0 else 1.0
    assert sigma == dref.sigma_position(pos)
    if kind == "extremes" and n > 1:
        assert (lo == np.float32([-100.0, -300.0, -200.0])).all() and (hi == np.float32([250.0, 150.0, 350.0])).all() and sigma == 0.01 * 550.0
    if kind == "none_finite":
        assert count == 0 and sigma == 1.0
    if kind == "one_finite" or n == 1:
        assert count == 1 and extent == 0.0 and sigma == 1.0 and len(finite) == 1
    # without the extent: the same four arrays, and nothing else written
    alone = guarded(torch, np.full(n * 3, SENT32, np.float32), SENT32)
    rc = mi._lib().dtof_denoise_inputs_async(sc._h, mode, ins[0][1], ins[1][1], ins[2][1], K, n, n_passes, n_samples, T, outs["colour"][1], outs["variance"][1],
                                             outs["normal"][1], alone[1], None)
    assert rc == 0, mi._lib().dtof_last_error()
    torch.cuda.synchronize()
    payload, margin = split_margins(alone[0], n * 3, np.float32)
    assert (margin == SENT32).all() and dref.same_bits(payload, pos.reshape(-1), nan_equal=True)


# ---------------------------------------------------------------------------- 4. a scene with nothing in view
def test_nothing_in_view(mi):
    from mitsuba3dopplertof_amd import harness
    xml = _xml("cornell_wall.xml", None)
    towards, away = '<matrix value="-1 0 0 0 0 1 0 1 0 0 -1 6.8 0 0 0 1" />', '<matrix value="1 0 0 0 0 1 0 1 0 0 1 6.8 0 0 0 1" />'
    assert towards in xml
    sc = mi.load_string(xml.replace(towards, away), resx=12, resy=9)
    r = sc.render_denoised_device(seed=SEED, spp=4, variants=K4, details=True)
    assert not r["aovs"][1:].any() and (r["aovs"][0] > 0).all() and not r["position"].any() and not r["normal"].any()
    assert r["sigma_position"] == 1.0 and not r["sum"].any()
    assert np.isfinite(r["denoised"]).all() and np.isfinite(r["denoised_variance"]).all() and not r["denoised"].any()
    noisy, denoised = sc.render_velocity_map_denoised(1, 4, (0.0, 0.25), T, W_G, seed=SEED, details=True)
    d = sc.denoise_details
    assert d["sigma_position"] == 1.0 and not d["position"].any() and np.isfinite(d["denoised"]).all()
    tof, den = d["colour"][..., 0], d["denoised"][..., 0]
    assert dref.same_bits(noisy, harness.calc_velocity_from_homo_heteros(list(tof[:2]), list(tof[2:]), T, W_G), nan_equal=True)
    assert dref.same_bits(denoised, harness.calc_velocity_from_homo_heteros(list(den[:2]), list(den[2:]), T, W_G), nan_equal=True)
    assert np.isfinite(noisy).all() and np.isfinite(denoised).all()      # a vanishing homodyne film: ratio 0, velocity 0


# ---------------------------------------------------------------------------- 5. the command line
def test_command_line_device_route_writes_the_python_entrys_arrays(mi, tmp_path):
    """The box filter at 1 spp: every film takes one term per pixel and plane, so two processes compute the same words and the files can be held to equality"""
    wall = str(tmp_path / "wall_box.xml")
    open(wall, "w").write(_xml("cornell_wall.xml", "box"))
    out_img, out_map = str(tmp_path / "img.npy"), str(tmp_path / "map.npy")
    base = [sys.executable, "-m", "mitsuba3dopplertof_amd", wall, "-Dresx=16", "-Dresy=12", "-Dtime_sampling_method=uniform", "--spp", "1", "--denoise", "--denoise-route",
            "device", "--denoise-levels", "2"]
    r = subprocess.run(base + ["--seed", "3", "-o", out_img], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["--velocity-map", "0,0.25", "-o", out_map], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    sc = mi.load_file(wall, resx=16, resy=12, time_sampling_method="uniform")
    want = sc.render_denoised_device(seed=3, spp=1, levels=2)
    assert dref.same_bits(np.load(out_img), want["denoised"])
    assert dref.same_bits(np.load(str(tmp_path / "img_noisy.npy")), want["image"])      # write_image stores float32
    noisy, denoised = sc.render_velocity_map_denoised(1, 1, (0.0, 0.25), levels=2)
    assert dref.same_bits(np.load(out_map), denoised) and dref.same_bits(np.load(str(tmp_path / "map_noisy.npy")), noisy)
