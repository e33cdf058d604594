"""The depth map on the device (dtof_depth.hip through dtof_depth_map_async and dtof_render_depth_map) against tests/depth_ref.py, the numpy restatement of the
definition in include/dtof.h: every output word EQUAL, a NaN where the reference has one.

  synthetic  dtof_depth_map_async on sums uploaded from the host, no render: 1 .. 4 frequencies; pixel counts around the block and wave sizes; random I / Q, phasors
             of known path lengths up to max_path_length, the special words (0, -0, denormals, inf, NaN) and I = Q = 0; output buffers between sentinels
  rendered   Scene.render_depth_map, both films: bit for bit harness.calc_depth_from_homodynes over the returned ToF images, which are the passes' mean of
             render(variants=triples) -- bit for bit with the float64 film, within the order of the float32 film's sums otherwise; the statistics"""
import os

import numpy as np
import pytest

import depth_ref
from conftest import SCENES

pytestmark = pytest.mark.gpu

IMG_TOL = 5e-5     # test_gpu_parity.IMG_TOL: relative to max|ref|; two atomic orders of the same lanes
MARGIN = 64        # sentinel elements on both sides of every output buffer
SENT32, SENT64, SENT_I = np.float32(-7.5e11), np.float64(-7.5e111), np.int32(-777)
SIZES = (1, 63, 64, 65, 255, 256, 257)
FREQUENCIES = (30.0, 40.0, 70.0, 17.3)
SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-38, -1e-39, 3e38, 1.0, -1.0], np.float32)
T = 0.0015


def phasor_sums(rng, n, frequencies, max_path, n_passes):
    """sums whose ToF values are close to A cos(phi), -A sin(phi) at known path lengths up to max_path (grey pixels: the luminance weights add up to 1)"""
    paths, amp = rng.uniform(0.0, max_path, n), rng.uniform(0.05, 4.0, n)
    s = np.zeros((2 * len(frequencies), n, 3), np.float32)
    for j, f in enumerate(frequencies):
        phi = depth_ref.TWO_PI * (paths / (300.0 / f))
        s[2 * j], s[2 * j + 1] = (amp * np.cos(phi) * n_passes / T).astype(np.float32)[:, None], (-amp * np.sin(phi) * n_passes / T).astype(np.float32)[:, None]
    return s


def make_sums(rng, kind, n, frequencies, max_path, n_passes):
    planes = 2 * len(frequencies)
    if kind == "random":
        return (rng.standard_normal((planes, n, 3)) * 10.0 ** rng.uniform(-3, 3, (planes, n, 1))).astype(np.float32)
    if kind == "phasors":
        return phasor_sums(rng, n, frequencies, max_path, n_passes)
    if kind == "zero":
        return np.zeros((planes, n, 3), np.float32)
    s = rng.standard_normal((planes, n, 3)).astype(np.float32)      # "special": a special word in every pixel, in one plane (all channels) or one channel
    for i in range(n):
        word = SPECIALS[rng.integers(len(SPECIALS))]
        if rng.random() < 0.5:
            s[rng.integers(planes), i, :] = word
        else:
            s[rng.integers(planes), i, rng.integers(3)] = word
    return s


@pytest.fixture(scope="module")
def torch_scene(mi):
    """a scene whose library calls are enqueued on torch's current stream: torch.cuda.synchronize() then waits for them"""
    import torch
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=8, resy=8)
    sc.set_stream(torch.cuda.current_stream().cuda_stream)
    yield sc
    torch.cuda.synchronize()
    sc.set_stream(None)


def guarded(torch, n, dtype, sentinel):
    t = torch.full((n + 2 * MARGIN,), sentinel.item(), dtype=dtype, device="cuda")
    return t, t.data_ptr() + MARGIN * t.element_size()


def split_margins(t, n):
    a = t.cpu().numpy()
    return a[MARGIN:MARGIN + n], np.concatenate([a[:MARGIN], a[MARGIN + n:]])


def run_synthetic(orc, sc, sums, frequencies, i_planes, q_planes, n_passes, max_path):
    """upload the sum, reconstruct on the device -> {output: words that differ from the reference}"""
    import torch
    F, n = len(frequencies), sums.shape[1]
    d_sum = torch.from_numpy(sums).cuda()
    bufs = {"depth": guarded(torch, n, torch.float64, SENT64), "residual": guarded(torch, n, torch.float64, SENT64), "wraps": guarded(torch, F * n, torch.int32, SENT_I),
            "amplitude": guarded(torch, F * n, torch.float64, SENT64), "phase": guarded(torch, F * n, torch.float32, SENT32)}
    torch.cuda.synchronize()
    sc.depth_map_async(d_sum.data_ptr(), i_planes, q_planes, frequencies, n_passes, n, bufs["depth"][1], exposure_time=T, max_path_length=max_path,
                       d_residual_ptr=bufs["residual"][1], d_wraps_ptr=bufs["wraps"][1], d_amplitude_ptr=bufs["amplitude"][1], d_phase_ptr=bufs["phase"][1])
    alone = guarded(torch, n, torch.float64, SENT64)      # without the optional outputs: the same depth
    sc.depth_map_async(d_sum.data_ptr(), i_planes, q_planes, frequencies, n_passes, n, alone[1], exposure_time=T, max_path_length=max_path)
    torch.cuda.synchronize()
    want = depth_ref.depth_map_of_sum(depth_ref.atan2f(orc), sums, i_planes, q_planes, frequencies, n_passes, T, max_path)
    bad = {}
    for key, (t, _) in bufs.items():
        count = n if key in ("depth", "residual") else F * n
        got, margin = split_margins(t, count)
        assert (margin == {"wraps": SENT_I, "phase": SENT32}.get(key, SENT64)).all(), ("margin of " + key, n)
        got = got.reshape(want[key].shape)
        bad[key] = 0 if depth_ref.same_words(got, want[key]) else int(((got != want[key]) & ~(np.isnan(got.astype(np.float64)) & np.isnan(want[key].astype(np.float64)))).sum())
    got, margin = split_margins(alone[0], n)
    assert (margin == SENT64).all()
    bad["depth alone"] = 0 if depth_ref.same_words(got, want["depth"]) else 1
    return bad, want


@pytest.mark.parametrize("kind", ["random", "phasors", "special", "zero"])
@pytest.mark.parametrize("n_freq", [1, 2, 3, 4])
def test_synthetic_sums_are_reconstructed_word_for_word(mi, orc, torch_scene, n_freq, kind):
    rng = np.random.default_rng(100 * n_freq + len(kind))
    frequencies = list(FREQUENCIES[:n_freq])
    planes = 2 * n_freq
    finite = total = unwrapped = 0
    for k, n in enumerate(SIZES):
        n_passes = 1 + k % 3
        max_path = (29.9, 30.0, 75.0)[k % 3]      # 3, 4 and 8 candidates of the 10 m wavelength
        order = rng.permutation(planes)            # the I / Q planes anywhere in the sum
        i_planes, q_planes = [int(x) for x in order[:n_freq]], [int(x) for x in order[n_freq:]]
        sums = make_sums(rng, kind, n, frequencies, max_path, n_passes)
        if kind == "phasors":                      # make_sums laid I / Q out as planes 2 j, 2 j + 1
            i_planes, q_planes = list(range(0, planes, 2)), list(range(1, planes, 2))
        bad, want = run_synthetic(orc, torch_scene, sums, frequencies, i_planes, q_planes, n_passes, max_path)
        print("kind", kind, "F", n_freq, "n", n, "mismatches", bad, "finite", int(np.isfinite(want["depth"]).sum()))
        assert not any(bad.values()), (kind, n_freq, n, bad)
        finite += int(np.isfinite(want["depth"]).sum()); total += n
        unwrapped += int((want["wraps"][0] > 0).sum())
    if kind in ("random", "phasors", "zero"):      # the comparison is about numbers, not NaN == NaN
        assert finite == total, (finite, total)
    if kind == "phasors" and n_freq > 1:
        assert unwrapped > total // 4, (unwrapped, total)      # wrap counts above 0 are exercised
    if kind == "special":
        assert 0 < finite < total, (finite, total)


# ---------------------------------------------------------------- rendered
def rel_linf(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def host_route_tof(mi, sc, n_passes, spp, frequencies, film):
    """the ToF images of harness.run_scene_depth_map's host renders for these passes: seeds 0 .. n_passes - 1, one traversal per group and pass, numpy after that"""
    triples = [tuple(float(x) for x in v) for v in mi.depth_map_variants(frequencies)]
    tof = []
    for g in range(0, len(triples), 4):
        acc = None
        for i in range(n_passes):
            img = sc.render(seed=i, spp=spp, variants=triples[g:g + 4], film=film).astype(np.float32)
            acc = img if acc is None else acc + img
        tof += [mi.to_tof_image(im, T) for im in acc / np.float32(n_passes)]
    return tof


@pytest.mark.parametrize("film", ["float32", "float64"])
@pytest.mark.parametrize("frequencies", [(30.0, 40.0), (30.0, 40.0, 70.0)], ids=["two_frequencies", "three_frequencies"])
def test_rendered_depth_map_on_the_wall(mi, frequencies, film):
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    sc.set_film_layout(2)      # the caller's film layout is neither read nor changed
    n_passes, spp, F = 2, 8, len(frequencies)
    out = sc.render_depth_map(n_passes, spp, frequencies, exposure_time=T, film=film)
    assert sc.last_stats["n_paths"] == 24 * 16 * spp * n_passes * ((F + 1) // 2)
    assert sc._film_layout == (2, 0)
    assert out["depth"].shape == (16, 24) and out["depth"].dtype == np.float64 and out["wraps"].shape == (F, 16, 24) and out["wraps"].dtype == np.int32
    assert out["amplitude"].shape == (F, 16, 24) and out["phase"].dtype == np.float32 and out["tof"].shape == (2 * F, 16, 24) and out["tof"].dtype == np.float32
    want = harness.calc_depth_from_homodynes(out["tof"][0::2], out["tof"][1::2], frequencies, 30.0)      # max_path_length=None: 300 / gcd(30, 40[, 70]) = 30
    for key in ("depth", "residual", "wraps", "amplitude", "phase"):
        assert depth_ref.same_words(out[key], want[key]), (key, int((out[key] != want[key]).sum()))
    assert np.isfinite(out["depth"]).all() and out["depth"].max() > 0 and (out["amplitude"] > 0).mean() > 0.9
    tof = host_route_tof(mi, sc, n_passes, spp, frequencies, film)
    for k in range(2 * F):
        assert np.abs(tof[k]).max() > 0
        if film == "float64":      # no atomics' order in the film: the passes' mean of render(variants=triples), bit for bit
            assert depth_ref.same_words(out["tof"][k], tof[k]), (k, int((out["tof"][k] != tof[k]).sum()))
        else:
            assert rel_linf(out["tof"][k], tof[k]) <= IMG_TOL, (k, rel_linf(out["tof"][k], tof[k]))
    if film == "float64":
        host = harness.calc_depth_from_homodynes(tof[0::2], tof[1::2], frequencies, 30.0)
        for key in ("depth", "residual", "wraps", "amplitude", "phase"):
            assert depth_ref.same_words(out[key], host[key]), key
    only = sc.render_depth_map(n_passes, spp, frequencies, exposure_time=T, film=film, outputs=("depth",))      # without the optional outputs
    assert sorted(only) == ["depth"]
    if film == "float64":
        assert depth_ref.same_words(only["depth"], out["depth"])


def test_harness_routes_agree(mi):
    """run_scene_depth_map (host) and run_scene_depth_map_device: the same dict word for word with the float64 film"""
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=24, resy=16)
    kw = dict(total_spp=16, frequencies=(30.0, 40.0), film="float64", time_sampling_method="antithetic", path_correlation_depth=16, max_depth=2)
    host, dev = harness.run_scene_depth_map(sc, **kw), harness.run_scene_depth_map_device(sc, **kw)
    assert len(sc.pass_stats) == 1 and sc.pass_stats[0]["n_paths"] == 24 * 16 * 16      # four films, one traversal
    for key in ("depth", "residual", "wraps", "amplitude", "phase", "tof"):
        assert depth_ref.same_words(np.asarray(host[key]), np.asarray(dev[key])), key
