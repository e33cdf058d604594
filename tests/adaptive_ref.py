"""The numpy definition of adaptive sampling's selection step (dtof_adaptive_select, csrc/dtof_adaptive.hip) and the expected films of a render over a pixel list,
from the oracle alone: nothing here touches the library under test.

  selection  the text of include/dtof.h in float64 numpy, operation for operation: S = the (P(K), n) RAW moment sums, count the samples of every pixel.  np.maximum
             is the device's max: the larger operand, a NaN of either side comes through.  test_adaptive_cpu.py pins both metrics, bit for bit, to
             harness.moment_statistics / velocity_standard_error, which were merged before this file.
  lists      Lanes: the oracle's lanes of a dense render, their footprint and moment / film values (moments_ref); sums(pixels) adds only the lanes of the listed pixels --
             what a sparse pass must put into the films, since lane pixel * spp + sample of a list is that lane of the dense render.
"""
import numpy as np

import moments_ref as ref

MODES = ("image", "velocity")


def cross_plane(K, j, k):
    """the plane of sum w Y_j Y_k among the P(K) planes"""
    j, k = min(j, k), max(j, k)
    return 1 + 6 * K + [p for p in ref.PAIRS if p[1] < K].index((j, k))


def variant_stats(S, K):
    """(mean_Y (K, n), var_Y (K, n), Wd (n,)) of the raw planes"""
    S = np.asarray(S, np.float64)
    Wd = np.where(S[0] == 0.0, 1.0, S[0])
    mean = np.stack([S[1 + 6 * k + 1] / Wd for k in range(K)])
    m2 = np.stack([S[1 + 6 * k + 4] / Wd for k in range(K)])
    return mean, m2 - mean * mean, Wd


def image_metric(S, K, count, floor):
    """(metric (n,), se (K, n))"""
    with np.errstate(all="ignore"):
        mean, var, _ = variant_stats(S, K)
        n = np.asarray(count).astype(np.float64)
        se = np.sqrt(np.maximum(var, 0.0) / n)
        metric = None
        for k in range(K):
            q = se[k] / np.maximum(np.abs(mean[k]), floor)
            metric = q if metric is None else np.maximum(metric, q)
        return np.where(np.asarray(count) == 0, 0.0, metric), se


def pair_se(S, K, count, h, t, exposure_time, w_g):
    """one pair: (se (n,), valid (n,), var_h, var_t)"""
    with np.errstate(all="ignore"):
        S = np.asarray(S, np.float64)
        mean, var, Wd = variant_stats(S, K)
        n = np.asarray(count).astype(np.float64)
        a, b = mean[h], mean[t]
        cov = S[cross_plane(K, h, t)] / Wd - a * b
        r = b / a
        var_r = ((var[t] - (2.0 * r) * cov) + (r * r) * var[h]) / ((a * a) * n)
        slope = ((0.5 * 3e8) / (w_g * 1e6)) / (exposure_time * ((r - 1.0) * (r - 1.0)))
        se = np.sqrt(np.maximum(var_r, 0.0)) * slope
        valid = (a != 0) & (r > -1.0) & (r < 0.999)
        return se, valid, var[h], var[t]


def velocity_metric(S, K, count, pairs, tol, exposure_time, w_g):
    """(metric (n,), selected (n,) bool)"""
    n_px = np.asarray(S).shape[1]
    best, any_, selected = np.full(n_px, np.nan), np.zeros(n_px, bool), np.zeros(n_px, bool)
    with np.errstate(all="ignore"):
        for h, t in pairs:
            se, valid, var_h, var_t = pair_se(S, K, count, h, t, exposure_time, w_g)
            usable = valid & np.isfinite(se)
            selected |= np.where(usable, se > tol, (var_h > 0) | (var_t > 0))
            better = usable & (~any_ | (se > best))
            best = np.where(better, se, best)
            any_ |= usable
    return best, selected


def select(S, K, count, spp, mode, tol, floor=1e-3, pairs=(), exposure_time=0.0015, w_g=30):
    """(ascending list (uint32), metric (n,), updated count (uint32))"""
    count = np.asarray(count, np.uint32)
    if mode == "image":
        metric, _ = image_metric(S, K, count, floor)
        with np.errstate(all="ignore"):
            selected = (metric > tol) & (count != 0)
    else:
        metric, selected = velocity_metric(S, K, count, pairs, tol, exposure_time, w_g)
    return np.flatnonzero(selected).astype(np.uint32), metric, (count + np.where(selected, np.uint32(spp), np.uint32(0))).astype(np.uint32)


def developed_dict(S, K, shape):
    """the dict Scene.render_moments returns for the raw planes S (P, n): every plane but the weight divided by (W == 0 ? 1 : W)"""
    S = np.asarray(S, np.float64)
    h, w = shape
    Wd = np.where(S[0] == 0.0, 1.0, S[0])
    dev = np.concatenate([S[:1], S[1:] / Wd]).reshape(-1, h, w)
    per = dev[1:1 + 6 * K].reshape(K, 6, h, w)
    cross = np.zeros((K, K, h, w))
    for a in range(K):
        cross[a, a] = per[a, 4]
    for j, k in ref.PAIRS:
        if k < K:
            cross[j, k] = cross[k, j] = dev[cross_plane(K, j, k)]
    return {"weight": dev[0], "mean": np.moveaxis(per[:, 0:3], 1, -1), "m2": np.moveaxis(per[:, 3:6], 1, -1), "cross": cross}


class Lanes:
    """The oracle's lanes of ONE dense pass (seed, spp, variants), their footprint, moment values and film values, computed once; sums(pixels) splats the lanes of the
    listed pixels only.  variants None: the scene's integrator."""

    def __init__(self, orc, osc, seed, spp, variants=None):
        if variants is None:
            pds = [osc.params()]
        else:
            pds = [osc.params(integrator=ref.integrator_of(osc, hetero_frequency=float(ref.F32(f)), hetero_offset=float(ref.F32(o)))) for f, o in variants]
        self.osc, self.spp, self.K = osc, spp, len(pds)
        self.lanes = [ref.lanes_of(orc, osc, pd, seed, spp) for pd in pds]
        spw, n_passes = ref.pass_layout(orc, osc, pds[0], spp)
        assert (spw, n_passes) == (spp, 1)
        self.fp = ref.footprint(orc, osc, self.lanes[0]["sample_pos"], spw)
        self.moment_values = ref.moment_values([ln["rgb"] for ln in self.lanes])
        ones = np.ones((len(self.lanes[0]), 1), ref.F32)
        self.film_values = [np.concatenate([ln["rgb"], ones], axis=1) for ln in self.lanes]       # r, g, b, 1 per variant
        self.alpha_values = np.concatenate([np.asarray(self.lanes[0]["valid"], ref.F32).reshape(-1, 1), 0 * ones, 0 * ones, ones], axis=1)   # (A, 0, 0, W)

    def lane_mask(self, pixels):
        w, h = self.osc.size
        keep = np.zeros(w * h, bool)
        keep[np.asarray(pixels, np.int64)] = True
        return np.repeat(keep, self.spp)

    def _splat(self, values, keep):
        flat, inside, wgt = self.fp
        return ref.splat(self.osc, (flat[keep], inside[keep], None if wgt is None else wgt[keep]), values[keep])

    def sums(self, pixels, film=False, alpha=False):
        """(moment sums (P, H, W), magnitudes) of the listed pixels' lanes; film=True: also (film sums (K [+ 1], H, W, 4), magnitudes)"""
        keep = self.lane_mask(pixels)
        m, mm = self._splat(self.moment_values, keep)
        if not film:
            return m, mm
        planes = [self._splat(v, keep) for v in self.film_values] + ([self._splat(self.alpha_values, keep)] if alpha else [])
        f = np.stack([np.moveaxis(p[0], 0, -1) for p in planes])
        fm = np.stack([np.moveaxis(p[1], 0, -1) for p in planes])
        return m, mm, f, fm


def synthetic(rng, n, K, noisy, edges=False, spp_so_far=(16, 65)):
    """Seeded raw planes (P(K), n) and counts (n,) for the selection tests, no render involved: signed Y means, a variance of about 1e-10 ("quiet") or about 1
    (`noisy`, a bool mask) per variant, even variants homodyne-like, odd ones a ratio in (-0.9, 0.5) times them (pairs (0, 1), (2, 3), (2, 1) are valid), correlated pairs, weights around the count.  edges=True overwrites a few
    pixels with what a film can hold at its worst: count 0, weight 0, m2 a little below mean^2, a homodyne mean of exactly 0, ratios outside the clip interval on
    both sides and at its ends, infinities."""
    P = ref.n_planes(K)
    count = rng.integers(spp_so_far[0], spp_so_far[1], n).astype(np.uint32)
    W = count * rng.uniform(0.9, 1.1, n)
    a = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    mean = np.stack([a * (1.0 if k % 2 == 0 else rng.uniform(-0.9, 0.5, n)) * rng.uniform(0.95, 1.05, n) ** (k // 2) for k in range(K)])
    var = np.where(noisy, 1.0, 1e-10)[None, :] * rng.uniform(0.5, 2.0, (K, n))
    S = np.zeros((P, n))
    S[0] = W
    for k in range(K):
        S[1 + 6 * k: 1 + 6 * k + 3] = rng.normal(size=(3, n)) * W
        S[1 + 6 * k + 3: 1 + 6 * k + 6] = rng.uniform(1, 2, (3, n)) * W
        S[1 + 6 * k + 1] = mean[k] * W
        S[1 + 6 * k + 4] = (var[k] + mean[k] * mean[k]) * W
    for j, k in ref.PAIRS:
        if k < K:
            S[cross_plane(K, j, k)] = (rng.uniform(-0.9, 0.9, n) * np.sqrt(var[j] * var[k]) + mean[j] * mean[k]) * W
    if edges and n >= 16:
        idx = rng.permutation(n)[:16]
        count[idx[0]] = 0
        S[0, idx[1]] = 0.0
        S[1 + 4, idx[2]] = S[1 + 1, idx[2]] ** 2 / S[0, idx[2]] * (1 - 2.0 ** -30)      # var slightly negative
        S[1 + 1, idx[3]] = 0.0                                                            # a == 0
        if K > 1:
            S[7 + 1, idx[4]] = 2.0 * S[1 + 1, idx[4]]                                     # r = 2
            S[7 + 1, idx[5]] = -3.0 * S[1 + 1, idx[5]]                                    # r = -3
            S[7 + 1, idx[6]] = -1.0 * S[1 + 1, idx[6]]                                    # r = -1: the closed end
            S[7 + 1, idx[7]] = 0.999 * S[1 + 1, idx[7]]
            S[7 + 4, idx[8]] = np.inf
            S[cross_plane(K, 0, 1), idx[9]] = -np.inf
        S[1 + 4, idx[10]] = np.inf
        S[1 + 1, idx[11]] = np.inf
        S[1 + 1, idx[12]] = -np.inf
        S[0, idx[13]] = np.inf
        S[1 + 4, idx[14]] = S[1 + 1, idx[14]] ** 2 / S[0, idx[14]]                        # var about 0, either sign
        count[idx[15]] = 1
    return S, count
