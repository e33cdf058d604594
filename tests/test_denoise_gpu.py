"""The denoiser on the device (csrc/dtof_denoise.hip through dtof_denoise_async and dtof_denoise), held to tests/denoise_ref.py:

  synthetic  shapes smaller than one halo, than one tile, no tile multiple, and more than two tiles in both axes at the largest step; levels 1, 2, 5, 6 (step 32
             exceeds several of the sizes); 1 .. 4 planes; all eight guide subsets.  Every shape meets every number of levels and every guide subset, every
             (planes, subset) pair -- every instantiation of the level kernel -- occurs twice, at one number of levels each: 64 cases, CASES below.  Signed colours scaled by 10^U(-6, 2);
             piecewise-planar guides with sharp edges through tile interiors and on tile borders; about 5 % of the pixels carry a NaN or an infinity in one colour,
             variance or guide word; variances of 0, -1 and denormal; neighbours of equal luminance under a zero variance.
  criterion  for EVERY pixel of every case: where the reference is finite |got - ref| <= 2^-40 envelope (colour) and 2^-39 envelope (variance); invalid centres
             carry the converted input bit for bit; the sentinel margins around both outputs are untouched.
  the bound  all validity and zero-denominator decisions are exact decisions on the same doubles; a tap's weight has a relative error of about |e| 2^-51 plus an
             ulp or two of the device's exp, a tap enters with exp(e), and |e| exp(e) <= 0.37: a level adds about 2^-50 of the envelope, six stay below 2^-47.
             2^-40 is the bound of the project's other double films (test_aov_gpu.py, test_film64_gpu.py).
             Measured: most cases stay below 0.02 of the bound; K = 4 with all guides at five levels on 63 x 65 reaches 0.34 of it.  The likely reason (reasoned, not
             isolated by a measurement): the estimate above leaves out that Y(p) - Y(q) cancels: the luminances carry the 2^-50 of the level before, the filtered variance shrinks from level to level while Y does not, and the
             exponent's error is that 2^-50 times Y / den.  That would be a property of the definition, which the reference shares, not of the kernel.
  further    K = 4 (and 1, 2) with all guides at 2, 5 and 6 levels against the reference again; the host entry computes the async entry's bits; a plane that is 3 times another (its
             variance 9 times) comes out as 3 times the other: one set of weights; Scene.render_denoised on the wall equals the reference applied to its own image,
             variance and guides; on the moving wall the denoised velocity map of run_scene_velocity_map_denoised is closer to -10 m/s than the noisy one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import SCENES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

WALL = os.path.join(SCENES, "cornell_wall.xml")
MARGIN = 64
SENT64 = np.float64(-7.5e111)
TOL_COLOUR, TOL_VARIANCE = 2.0 ** -40, 2.0 ** -39
SHAPES = ((1, 1), (7, 1), (1, 7), (5, 3), (63, 65), (64, 64), (130, 70), (257, 9))      # W x H
LEVELS = (1, 2, 5, 6)
SIGMAS = dict(sigma_normal=0.3, sigma_position=2.5, sigma_luminance=4.0)
# (shape index, levels, planes, guide mask: 1 normal, 2 position, 4 variance)
CASES = [(a, LEVELS[li], 1 + (li + t + a) % 4, (2 * li + t + a) % 8) for a in range(len(SHAPES)) for li in range(4) for t in range(2)]
assert len({(k, m) for _, _, k, m in CASES}) == 32 and all(len({m for b, _, _, m in CASES if b == a}) == 8 for a in range(len(SHAPES)))
SPECIALS = (np.nan, np.inf, -np.inf)


def make_inputs(seed, k, w, h):
    """colour (K, H, W, 3) float32, variance (K, H, W) float64, normal, position (H, W, 3) float32"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    # the magnitude changes from one 5 x 5 block to the next; inside a block neighbours are comparable, so the luminance term decides something
    scale = 10.0 ** rng.uniform(-6, 2, ((h + 4) // 5, (w + 4) // 5))[yy // 5, xx // 5]
    colour = ((rng.standard_normal((k, h, w, 3)) * 0.5 + rng.choice([-1.0, 1.0], (k, 1, 1, 3))) * scale[None, :, :, None]).astype(np.float32)
    variance = (0.5 * scale[None]) ** 2 * rng.uniform(0.2, 2.0, (k, h, w))
    pick = rng.random((k, h, w))
    variance = np.where(pick < 0.04, 0.0, np.where(pick < 0.06, -1.0, np.where(pick < 0.08, 5e-324 * rng.integers(1, 9, (k, h, w)), variance)))
    if w >= 3:      # neighbours of equal luminance under a zero variance: only they pass the luminance term
        y = h // 2
        colour[:, y, 1:3] = colour[:, y, 0:1]
        variance[:, y, 0:3] = 0.0
    # three planes: edges at x = 32 (inside a tile), x = 64 (a tile border), and at rows 2 and 4 (inside a tile of rows, and on its border at step 1); small
    # images get one through their middle
    region = (xx >= 32).astype(int) + (xx >= 64) + 3 * ((yy >= 2).astype(int) + (yy >= 4)) + 9 * (xx >= (w + 1) // 2)
    normals = rng.standard_normal((32, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    normal = normals[region % 32].astype(np.float32)
    depth = rng.uniform(-5, 5, 32)[region % 32] + 0.05 * xx * normals[region % 32, 0] - 0.03 * yy * normals[region % 32, 1]
    position = np.stack([0.4 * xx, 0.4 * yy, depth], axis=2).astype(np.float32)
    for y, x in zip(*np.nonzero(rng.random((h, w)) < 0.05)):      # one special word per chosen pixel
        which, value = rng.integers(4), SPECIALS[rng.integers(3)]
        if which == 0:
            colour[rng.integers(k), y, x, rng.integers(3)] = value
        elif which == 1:
            variance[rng.integers(k), y, x] = value
        elif which == 2:
            normal[y, x, rng.integers(3)] = value
        else:
            position[y, x, rng.integers(3)] = value
    return colour, variance, normal, position


@pytest.fixture(scope="module")
def torch_scene(mi):
    """a scene whose library calls are enqueued on torch's current stream: torch.cuda.synchronize() then waits for them"""
    import torch
    sc = mi.load_file(WALL, resx=8, resy=8)
    sc.set_stream(torch.cuda.current_stream().cuda_stream)
    yield sc
    torch.cuda.synchronize()
    sc.set_stream(None)


def guarded(torch, n):
    t = torch.full((n + 2 * MARGIN,), float(SENT64), dtype=torch.float64, device="cuda")
    return t, t.data_ptr() + MARGIN * 8


def split_margins(t, n):
    a = t.cpu().numpy()
    return a[MARGIN:MARGIN + n], np.concatenate([a[:MARGIN], a[MARGIN + n:]])


def run_async(mi, sc, colour, variance, normal, position, levels, want_variance=True):
    """dtof_denoise_async on torch's stream -> (colour (K, H, W, 3), variance (K, H, W) or None); asserts the sentinel margins"""
    import torch
    k, h, w = colour.shape[:3]
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (colour, variance, normal, position)]
    d_out, p_out = guarded(torch, k * h * w * 3)
    d_var, p_var = guarded(torch, k * h * w)
    prm = mi._DenoiseParams(levels, SIGMAS["sigma_normal"], SIGMAS["sigma_position"], SIGMAS["sigma_luminance"])
    torch.cuda.synchronize()
    rc = mi._lib().dtof_denoise_async(sc._h, dev[0].data_ptr(), k, w, h, None if dev[1] is None else dev[1].data_ptr(), None if dev[2] is None else dev[2].data_ptr(),
                                      None if dev[3] is None else dev[3].data_ptr(), C.byref(prm), p_out, p_var if variance is not None and want_variance else None)
    assert rc == 0, mi._lib().dtof_last_error()
    torch.cuda.synchronize()
    out, m_out = split_margins(d_out, k * h * w * 3)
    var, m_var = split_margins(d_var, k * h * w)
    assert (m_out == SENT64).all() and (m_var == SENT64).all(), "a sentinel margin was written"
    if variance is None or not want_variance:
        assert (var == SENT64).all(), "the variance output was written without being asked for"
        return out.reshape(k, h, w, 3), None
    return out.reshape(k, h, w, 3), var.reshape(k, h, w)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_against_reference(got, got_var, ref, colour, variance, label):
    """the criterion of the module docstring over every pixel; returns the largest error in units of the bound (printed by the caller)"""
    valid = ref["valid"]
    worst = 0.0
    pairs = [("colour", got, ref["colour"], ref["envelope_colour"][-1], TOL_COLOUR, colour.astype(np.float64), valid[None, :, :, None])]
    if got_var is not None:
        pairs.append(("variance", got_var, ref["variance"], ref["envelope_variance"][-1], TOL_VARIANCE, variance, valid[None]))
    for name, g, r, env, tol, converted, v in pairs:
        v = np.broadcast_to(v, r.shape)
        assert np.isfinite(r[v]).all(), (label, name, "the reference is finite at every valid pixel of these inputs")
        err = np.abs(g[v] - r[v])
        bound = tol * env[v]
        assert (err <= bound).all(), (label, name, "worst |got - ref| / envelope = 2^%.1f" % np.log2((err / np.where(env[v] > 0, env[v], 1.0)).max()))
        if (bound > 0).any():
            worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert (bits(g[~v]) == bits(converted[~v])).all(), (label, name, "an invalid centre must carry the converted input")
    return worst


@pytest.mark.parametrize("shape_index", range(len(SHAPES)))
def test_synthetic_images_against_the_reference(mi, torch_scene, shape_index):
    w, h = SHAPES[shape_index]
    for a, levels, k, mask in CASES:
        if a != shape_index:
            continue
        colour, variance, normal, position = make_inputs(1000 * a + 10 * levels + mask, k, w, h)
        variance, normal, position = variance if mask & 4 else None, normal if mask & 1 else None, position if mask & 2 else None
        ref = R.denoise(colour, variance, normal, position, levels=levels, **SIGMAS)
        got, got_var = run_async(mi, torch_scene, colour, variance, normal, position, levels)
        label = "%dx%d levels %d planes %d guides %d" % (w, h, levels, k, mask)
        worst = check_against_reference(got, got_var, ref, colour, variance, label)
        print("%s: %d invalid pixels, worst error %.3g of the bound" % (label, int((~ref["valid"]).sum()), worst))
        if w * h >= 64:
            assert (~ref["valid"]).any() and ref["valid"].any(), label


@pytest.mark.parametrize("shape_index,levels,k", [(4, 5, 4), (6, 6, 4), (7, 2, 1), (3, 6, 2)])
def test_production_configuration_against_the_reference_and_the_host_entry(mi, torch_scene, shape_index, levels, k):
    """all three guides -- with K = 4 the configuration of Scene.render_denoised and of the velocity map -- at the deeper levels, against the reference like the
    synthetic cases; then the same bits without the optional output, through the host entry and through mi.Denoiser"""
    w, h = SHAPES[shape_index]
    colour, variance, normal, position = make_inputs(77 + shape_index, k, w, h)
    L = mi._lib()
    tiled, tiled_var = run_async(mi, torch_scene, colour, variance, normal, position, levels)
    ref = R.denoise(colour, variance, normal, position, levels=levels, **SIGMAS)
    label = "%dx%d levels %d planes %d guides 7" % (w, h, levels, k)
    worst = check_against_reference(tiled, tiled_var, ref, colour, variance, label)
    print("%s: %d invalid pixels, worst error %.3g of the bound" % (label, int((~ref["valid"]).sum()), worst))
    # without the optional output the colours are the same and nothing else is written
    alone, none = run_async(mi, torch_scene, colour, variance, normal, position, levels, want_variance=False)
    assert none is None and (bits(alone) == bits(tiled)).all()
    # dtof_denoise: host pointers, no scene
    out, out_var = np.full((k, h, w, 3), SENT64), np.full((k, h, w), SENT64)
    prm = mi._DenoiseParams(levels, SIGMAS["sigma_normal"], SIGMAS["sigma_position"], SIGMAS["sigma_luminance"])
    assert L.dtof_denoise(colour.ctypes.data, k, w, h, variance.ctypes.data, normal.ctypes.data, position.ctypes.data, C.byref(prm), out.ctypes.data, out_var.ctypes.data) == 0
    assert (bits(out) == bits(tiled)).all() and (bits(out_var) == bits(tiled_var)).all()
    # ... and mi.Denoiser on top of it
    den = mi.Denoiser((w, h), normals=True, position=True, variance=True, levels=levels, **SIGMAS)
    py, py_var = den(colour, normals=normal, position=position, variance=variance)
    assert (bits(py) == bits(tiled)).all() and (bits(py_var) == bits(tiled_var)).all()


def test_planes_share_one_set_of_weights(mi, torch_scene):
    """plane 1 = 3 x plane 0, its variance 9 x: d_1 = |3 dY| / (3 den) is d_0 up to rounding, the weights are common, so the output of plane 1 is 3 x the output of
    plane 0 within the bound, and the ratio image is constant.  The last two mantissa bits of plane 0 are cleared, so that 3 x is exact in float32."""
    w, h = 130, 70
    colour, variance, normal, position = make_inputs(5, 2, w, h)
    colour[0] = (colour[0].view(np.uint32) & np.uint32(0xfffffffc)).view(np.float32)
    with np.errstate(all="ignore"):
        colour[1] = colour[0] * np.float32(3.0)
        assert np.array_equal(colour[1].astype(np.float64), colour[0].astype(np.float64) * 3.0, equal_nan=True)
    variance[1] = variance[0] * 9.0
    ref = R.denoise(colour, variance, normal, position, levels=5, **SIGMAS)
    got, got_var = run_async(mi, torch_scene, colour, variance, normal, position, 5)
    check_against_reference(got, got_var, ref, colour, variance, "shared weights")
    v = ref["valid"]
    assert v.sum() > w * h // 2
    env = ref["envelope_colour"][-1]
    assert (np.abs(got[1][v] - 3.0 * got[0][v]) <= 3.0 * TOL_COLOUR * env[0][v] + TOL_COLOUR * env[1][v]).all()
    env_v = ref["envelope_variance"][-1]
    normal_range = v & (env_v[0] > 1e-290)      # sums of denormal variances round to multiples of 5e-324, which is no small fraction of them
    assert (np.abs(got_var[1][normal_range] - 9.0 * got_var[0][normal_range]) <= 9.0 * TOL_VARIANCE * env_v[0][normal_range] + TOL_VARIANCE * env_v[1][normal_range]).all()
    assert normal_range.sum() > v.sum() // 2
    big = v[..., None] & (np.abs(got[0]) > 2.0 ** -20 * env[0])      # where the sum did not cancel, the ratio itself is 3 to a few ulps of 2^-20
    assert big.sum() > 1000 and np.abs(got[1][big] / got[0][big] - 3.0).max() < 2.0 ** -18


VARIANTS = [(0, 0), (0, .25), (1, 0), (1, .25)]


def test_render_denoised_equals_the_reference_on_its_own_films(mi):
    sc = mi.load_file(WALL, resx=32, resy=32)
    # What the call itself rendered is kept: a second traversal of the same seed adds its terms in another order of the atomics, in the float32 film
    # (test_gpu_parity.IMG_TOL) and, under the tent filter, in the double films of the moments and the guides too (test_moments_gpu.py).
    kept = {}

    def keep(name):
        inner = getattr(sc, name)

        def call(*a, **kw):
            kept.setdefault(name, []).append(inner(*a, **kw))
            return kept[name][-1]
        setattr(sc, name, call)

    for name in ("render", "render_moments", "render_aovs"):
        keep(name)
    d = sc.render_denoised(seed=3, spp=16, variants=VARIANTS)
    for name in ("render", "render_moments", "render_aovs"):
        delattr(sc, name)
    assert [len(kept[name]) for name in ("render", "render_moments", "render_aovs")] == [1, 1, 1]
    assert d["image"].dtype == np.float32 and np.array_equal(d["image"].view(np.uint32), kept["render"][0].view(np.uint32))      # "image" is the call's own render()
    again = sc.render(seed=3, spp=16, variants=VARIANTS)
    assert np.abs(again - d["image"]).max() <= 5e-5 * np.abs(again).max()
    m, guides = kept["render_moments"][0], kept["render_aovs"][0]
    assert np.array_equal(d["variance"], (m["m2"][..., 1] - m["mean"][..., 1] ** 2) / 16.0)
    assert guides["channels"] == ["p.X", "p.Y", "p.Z", "n.X", "n.Y", "n.Z"]
    den = d["denoiser"]
    assert den.levels == 5 and den.last_sigma_position > 0
    ref = R.denoise(d["image"], d["variance"], guides["n"].astype(np.float32), guides["p"].astype(np.float32), levels=5, sigma_normal=den.sigma_normal,
                    sigma_position=den.last_sigma_position, sigma_luminance=den.sigma_luminance)
    assert d["denoised"].shape == (4, 32, 32, 3) and d["denoised_variance"].shape == (4, 32, 32) and d["denoised"].dtype == np.float64
    check_against_reference(d["denoised"], d["denoised_variance"], ref, d["image"], d["variance"], "render_denoised")
    assert ref["valid"].all()
    assert d["denoised_variance"].sum() < d["variance"].sum()      # it denoises: the variance estimate of the weighted means is smaller
    single = sc.render_denoised(seed=3, spp=16, levels=2)
    assert single["image"].shape == (32, 32, 3) and single["denoised"].shape == (32, 32, 3) and single["variance"].shape == (32, 32)


def test_denoised_velocity_map_is_closer_to_the_walls_velocity(mi):
    """The moving wall of test_io_and_harness.py's -10 m/s check (512 spp in one pass, max_depth 2) at 64 x 64: over the pixels whose camera rays all end on the wall
    (the aov film's shape_index), the RMS error of the denoised map against the analytic -10 m/s is smaller than that of the noisy map.  Measured on an MI355X:
    see profiles/denoise_wall.txt."""
    from mitsuba3dopplertof_amd import harness
    sc = mi.load_file(WALL, resx=64, resy=64)
    noisy, denoised = harness.run_scene_velocity_map_denoised(sc, 512, max_depth=2)
    assert noisy.shape == (64, 64) and denoised.shape == (64, 64)
    index = sc.render_aovs("s:shape_index", seed=0, spp=64)["s"]
    # the back wall fills the centre of the frame; the index is a filtered mean, an integer up to rounding where every sample of the footprint met the same shape
    wall = np.abs(index - np.round(index[32, 32])) < 1e-6
    assert 400 < wall.sum() < 64 * 64
    rms_noisy = float(np.sqrt(np.mean((noisy[wall] + 10.0) ** 2)))
    rms_denoised = float(np.sqrt(np.mean((denoised[wall] + 10.0) ** 2)))
    print("wall pixels %d: RMS error against -10 m/s noisy %.6g, denoised %.6g" % (int(wall.sum()), rms_noisy, rms_denoised))
    assert rms_denoised < rms_noisy
