"""Expected values of the per-pixel moment film (dtof_render_moments), from the oracle alone: nothing here touches the library under test.

  lanes     sample_pos and rgb of every lane from orc.Scene.render_lanes, per variant with the integrator dictionary test_film64_gpu.integrator_of builds
  weights   orc_kat_filter (ReconstructionFilter::eval) per lane and tap, through ctypes.  orc_kat_filter returns 0 for |x| >= radius; ImageBlock::put calls eval()
            without that test (imageblock.cpp:510-517), and so do orc_render_exact and splat_lane.  Only the gaussian's clamped polynomial is not 0 there (it stays
            positive a few 1e-4 beyond the radius): those taps alone are evaluated by gaussian_eval below, a float32 restatement of the oracle's filter_eval that every
            call first checks, bit for bit, against orc_kat_filter on the taps inside the radius.  (The Lanczos filter differs only for |x| == radius exactly.)
  footprint the arithmetic of splat_lane (csrc/dtof_device.h) in numpy float32: n = ceil(radius - .5), floor(pos) - n, rel = (float) pix + .5f - pos, the crop
            offset; the box filter puts the value itself and 1 at the lane's own pixel, lane = pixel * spp + sample (per pass of a multi-pass render)
  values    X = (0.412453f r + 0.357580f g) + 0.180423f b, ... (srgb_to_xyz), the squares and the pair products Y_j Y_k, in numpy float32 -- elementwise float32
            operations, so nothing is contracted
  sums      the float32 terms value * (wx * wy), converted to float64 and added in float64; beside every sum the sum of the terms' magnitudes, which scales the bound
"""
import ctypes as C
import os

import numpy as np

F32 = np.float32
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
BOUND = 2.0 ** -40      # |device - expected| <= BOUND * sum |term| per pixel: <= 2^12 terms a pixel, each addition 2^-53 of the magnitudes, on either side
NCPU = os.cpu_count() or 1
XYZ = np.asarray([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], F32)


def n_planes(K):
    return 1 + 6 * K + K * (K - 1) // 2


def integrator_of(osc, **override):
    """test_film64_gpu.integrator_of: the scene file's integrator as the dictionary Scene.params(integrator=...) takes, with properties replaced"""
    ip = osc.flat.integrator
    conv = {"float": float, "int": int, "bool": bool}
    d = {"type": ip.plugin}
    d.update({k: conv.get(t, str)(v) for k, (t, v) in ip.items()})
    d.update(override)
    return d


def lanes_of(orc, osc, pd, seed, spp):
    """every lane of the render (all passes): index = pass * wavefront + lane"""
    w, h = osc.size
    return osc.render_lanes(pd, seed, spp, 0, w * h * spp, threads=NCPU)


def pass_layout(orc, osc, pd, spp):
    """(samples per wavefront, passes) of the render (orc_pass_layout)"""
    w, h = osc.size
    spw, n_passes = C.c_uint32(0), C.c_uint32(0)
    orc.lib().orc_pass_layout(w, h, spp, pd["samples_per_pass"], C.byref(spw), C.byref(n_passes))
    return spw.value, n_passes.value


_GAUSS = (9.992604880e-1, -4.977025247e-1, 1.222248550e-1, -1.932406282e-2, 2.136713061e-3, -1.679873860e-4, 9.202145248e-6, -3.329417433e-7, 7.128382794e-9,
          -6.821193280e-11)      # oracle/dtof_oracle.c: gaussian_coeffs


def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _estrin10(x, c):
    """oracle/dtof_oracle.c: estrin10"""
    x = np.asarray(x, F32)
    x2 = x * x; x4 = x2 * x2; x8 = x4 * x4
    a = [_fma(x, c[2 * i + 1], c[2 * i]) for i in range(5)]
    b0, b1 = _fma(x2, a[1], a[0]), _fma(x2, a[3], a[2])
    return _fma(x8, a[4], _fma(x4, b1, b0))


def gaussian_eval(x, radius, stddev):
    """oracle/dtof_oracle.c: filter_eval of the gaussian, max(estrin10(x * x, gc), 0) WITHOUT a test against the radius"""
    gc, scale = [], 1.0
    for c in _GAUSS:
        gc.append(F32(c * scale))
        scale /= float(stddev) * float(stddev)
    gc[0] = F32(gc[0] - _estrin10(F32(radius) * F32(radius), gc))
    x = np.asarray(x, F32)
    return np.maximum(_estrin10(x * x, gc), F32(0))


def footprint(orc, osc, pos, spw, first=None):
    """The taps of every lane: (flat pixel index (N, T) int64, in-bounds mask (N, T), weight w = wx * wy (N, T) float32 -- None for the box filter, whose one tap
    adds the value itself).  first: the film pixel (N, 2) the footprint starts at instead of floor(pos) - n -- what a splat that anchors a sample at another pixel
    than its own would compute (splat_ref's mutations; no expected value is built with it)."""
    se = osc.flat.sensor
    W, H = int(se["crop_w"]), int(se["crop_h"])
    N = len(pos)
    if int(se["filter"]) == 0:      # box: the lane's own pixel
        pix = (np.arange(N, dtype=np.int64) % (W * H * spw)) // spw
        return pix[:, None], np.ones((N, 1), bool), None
    radius = F32(se["filter_radius"])
    n = int(np.ceil(radius - F32(.5)))
    cnt = 2 * n + 1
    pos = np.ascontiguousarray(pos, F32)
    pix = np.floor(pos).astype(np.int32) - np.int32(n) if first is None else np.asarray(first, np.int32).reshape(N, 2)      # (N, 2): x, y
    rel = (pix.astype(F32) + F32(.5)) - pos                             # (float) pix + .5f - pos, left to right, float32
    anchor = pix - np.asarray([se["crop_x"], se["crop_y"]], np.int32)
    L = orc.lib()
    kind, stddev, B, Cc = int(se["filter"]), float(F32(se["filter_stddev"])), float(F32(se["filter_b"])), float(F32(se["filter_c"]))
    taps = np.zeros((N, 2, cnt), F32)
    for a in range(cnt):
        x = rel + F32(a)                                                # float32
        for i in range(N):
            taps[i, 0, a] = L.orc_kat_filter(kind, float(radius), stddev, B, Cc, float(x[i, 0]))
            taps[i, 1, a] = L.orc_kat_filter(kind, float(radius), stddev, B, Cc, float(x[i, 1]))
    if kind == 2:      # gaussian: the taps at and beyond the radius, where orc_kat_filter answers 0 and eval() does not
        x = rel[:, :, None] + np.arange(cnt, dtype=F32)[None, None, :]
        own = gaussian_eval(x, radius, F32(se["filter_stddev"]))
        inner = np.abs(x) < radius
        assert (own[inner].view(np.uint32) == taps[inner].view(np.uint32)).all(), "gaussian_eval is not the oracle's filter inside the radius"
        assert not taps[~inner].any()
        taps = np.where(inner, taps, own)
    w = (taps[:, 0, None, :] * taps[:, 1, :, None]).astype(F32)         # [lane, ys, xs] = wx * wy, a float32 product
    xs = anchor[:, 0, None, None] + np.arange(cnt)[None, None, :]
    ys = anchor[:, 1, None, None] + np.arange(cnt)[None, :, None]
    xs, ys = np.broadcast_arrays(xs, ys)
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    flat = np.where(inside, ys.astype(np.int64) * W + xs, 0)
    return flat.reshape(N, -1), inside.reshape(N, -1), w.reshape(N, -1)


def splat(osc, fp, values):
    """values (N, C) float32 through the footprint -> (sums (C, H, W) float64, sums of magnitudes (C, H, W) float64); the terms are float32 products"""
    flat, inside, w = fp
    W, H = osc.size
    values = np.ascontiguousarray(values, F32)
    C_ = values.shape[1]
    sums, mags = np.zeros((C_, H * W)), np.zeros((C_, H * W))
    idx = flat[inside]
    for c in range(C_):
        v = values[:, c, None]
        term = np.broadcast_to(v, flat.shape) if w is None else (v * w).astype(F32)      # float32
        t = term[inside].astype(np.float64)
        np.add.at(sums[c], idx, t)
        np.add.at(mags[c], idx, np.abs(t))
    return sums.reshape(C_, H, W), mags.reshape(C_, H, W)


def expected_rgbw(orc, osc, pd, seed, spp):
    """The raw RGBW film of one render of the oracle's lanes: (sums (4, H, W), sums of magnitudes (4, H, W)), the channels r, g, b and the weight's value 1"""
    lanes = lanes_of(orc, osc, pd, seed, spp)
    spw, _ = pass_layout(orc, osc, pd, spp)
    fp = footprint(orc, osc, lanes["sample_pos"], spw)
    return splat(osc, fp, np.concatenate([lanes["rgb"], np.ones((len(lanes), 1), F32)], axis=1))


def xyz(rgb):
    """srgb_to_xyz in float32, the sums left to right: (N, 3) float32"""
    rgb = np.ascontiguousarray(rgb, F32)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return np.stack([(XYZ[i, 0] * r + XYZ[i, 1] * g) + XYZ[i, 2] * b for i in range(3)], axis=1).astype(F32)


def moment_values(rgbs):
    """rgbs: K arrays (N, 3) float32 -> (N, P(K)) float32 in plane order; column 0 is the weight's value 1"""
    K = len(rgbs)
    cols = [np.ones(len(rgbs[0]), F32)]
    ys = []
    for rgb in rgbs:
        v = xyz(rgb)
        cols += [v[:, 0], v[:, 1], v[:, 2], v[:, 0] * v[:, 0], v[:, 1] * v[:, 1], v[:, 2] * v[:, 2]]
        ys.append(v[:, 1])
    cols += [ys[j] * ys[k] for j, k in PAIRS if k < K]
    out = np.stack(cols, axis=1).astype(F32)
    assert out.shape[1] == n_planes(K)
    return out


def expected_moments(orc, osc, seed, spp, variants=None, override=None):
    """The raw planes of one pass with `seed`: (sums (P, H, W), sums of magnitudes (P, H, W)).  variants: (hetero_frequency, hetero_offset) pairs, None = the
    integrator of the scene (with `override` applied)."""
    if variants is None:
        pds = [osc.params(integrator=integrator_of(osc, **override)) if override else osc.params()]
    else:
        pds = [osc.params(integrator=integrator_of(osc, hetero_frequency=float(F32(f)), hetero_offset=float(F32(o)), **(override or {}))) for f, o in variants]
    lanes = [lanes_of(orc, osc, pd, seed, spp) for pd in pds]
    for ln in lanes[1:]:
        assert (ln["sample_pos"] == lanes[0]["sample_pos"]).all()      # the variants share their paths
    spw, _ = pass_layout(orc, osc, pds[0], spp)
    fp = footprint(orc, osc, lanes[0]["sample_pos"], spw)
    return splat(osc, fp, moment_values([ln["rgb"] for ln in lanes]))


def errors_over_bound(got, want, mags):
    """per plane the largest |got - want| / (BOUND * sum |term|) over the pixels; a pixel without terms must be exactly 0 on both sides"""
    got, want, mags = np.asarray(got), np.asarray(want), np.asarray(mags)
    assert got.shape == want.shape == mags.shape, (got.shape, want.shape, mags.shape)
    diff = np.abs(got - want)
    empty = mags == 0.0
    assert not diff[empty].any(), "a pixel without terms is not zero"
    ratio = np.where(empty, 0.0, diff / np.where(empty, 1.0, BOUND * mags))
    ratio = np.where(np.isfinite(got) & np.isfinite(want), ratio, np.inf)
    return ratio.reshape(len(got), -1).max(axis=1)


def groups(K):
    """plane groups of the printed report: name -> slice or index list"""
    g = {"weight": [0], "mean": [1 + 6 * k + c for k in range(K) for c in range(3)], "m2": [1 + 6 * k + 3 + c for k in range(K) for c in range(3)]}
    if K > 1:
        g["cross"] = list(range(1 + 6 * K, n_planes(K)))
    return g


def report(what, ratios, K):
    text = ", ".join("%s %.3g" % (name, max(ratios[i] for i in idx if i < len(ratios))) for name, idx in groups(K).items() if idx[0] < len(ratios))
    print("%s: largest error / bound per plane group: %s" % (what, text))
    return text
