"""Expected raw float32 films of the splat kernels (k_splat_x8, k_splat_pixel, k_splat_tent3, k_splat_generic of csrc/dtof_kernels.hip and the splat fused into k_shade)
and the bound they are held to, from the oracle alone: nothing here touches the library under test.  On top of moments_ref (footprint, weights, terms) and
adaptive_ref.Lanes (the oracle's lanes of one dense pass).

Per pixel and channel:  E  the float64 sum of the float32 terms t = value * (wx * wy) of the oracle's lanes (the box filter: the values themselves),
                        M  the sum of |t|,
                        n  the number of in-bounds taps that land on the pixel (the number of terms).

CRITERION (derived, not measured):   |device - E| <= (n + 2) * 2^-24 * M   for every pixel and channel, and a pixel with M == 0 is exactly 0.
  - w = fl(wx * wy) is the same float32 on both sides: the device evaluates the filter with the oracle's arithmetic on the same float32 offsets (splat_lane).
  - a device term is either fl(r * w), the reference's own float32 term, or it enters its sum through fmaf(r, w, acc) unrounded: either way within 2^-24 |t| of the
    reference's term -- 2^-24 M over the pixel, and as much again for the first-order slack of M itself: the "+ 2".
  - a float32 sum of n values in ANY order (serial in a lane, DPP tree across a segment, LDS, float atomics on the film) deviates from the exact sum by at most
    (n - 1) * 2^-24 * M to first order.
With n <= 25 * 64 the bound stays below 1e-4 M, while one sample lost or counted twice moves the W channel of its own pixel by about M / spp: every spp the tests
use is small enough for that to exceed the bound (tests/test_splat_cpu.py shows it case by case, with the mutations below).

The mutation helpers return a perturbed COPY of a lane set -- what a subtly wrong kernel would have splatted -- and never feed an expected value."""
import numpy as np

import moments_ref as ref

EPS = 2.0 ** -24
F32 = ref.F32


class LaneSet:
    """What gets splatted: per lane the taps (flat pixel, in-bounds mask, weight -- moments_ref.footprint) and per film plane the (N, 4) float32 values (r, g, b, 1) --
    the alpha plane (A, 0, 0, 1) last when asked for.  `pixel` is the lane's nominal pixel in the crop window (lane // spp), `pos` its film position."""

    def __init__(self, osc, spp, flat, inside, wgt, values, pos):
        self.osc, self.spp, self.flat, self.inside, self.wgt, self.values, self.pos = osc, spp, flat, inside, wgt, values, pos

    @classmethod
    def of(cls, lanes, alpha=False, rows=None):
        """from adaptive_ref.Lanes; rows (r0, r1): only the lanes of those rows' pixels, as render_rows renders them"""
        flat, inside, wgt = lanes.fp
        values = list(lanes.film_values) + ([lanes.alpha_values] if alpha else [])
        pos = np.ascontiguousarray(lanes.lanes[0]["sample_pos"], F32)
        if rows is not None:
            w, h = lanes.osc.size
            keep = lanes.lane_mask(np.arange(rows[0] * w, rows[1] * w))
            inside = inside & keep[:, None]
        return cls(lanes.osc, lanes.spp, flat, inside, wgt, values, pos)

    def copy(self):
        return LaneSet(self.osc, self.spp, self.flat.copy(), self.inside.copy(), None if self.wgt is None else self.wgt.copy(), [v.copy() for v in self.values], self.pos)

    @property
    def n_lanes(self):
        return len(self.flat)

    def nominal(self, i=None):
        """(x, y) of the nominal pixel in the crop window"""
        w, _ = self.osc.size
        pix = (np.arange(self.n_lanes) if i is None else np.asarray(i)) // self.spp
        return pix % w, pix // w

    def irregular(self):
        """(x mask, y mask): lanes whose float position floors into another pixel than their own -- the `irregular` mask of k_splat_x8, `fx != px` elsewhere.  The box
        filter splats at the lane's own pixel whatever the position."""
        se = self.osc.flat.sensor
        px, py = self.nominal()
        fx = np.floor(self.pos[:, 0]).astype(np.int64) - int(se["crop_x"])
        fy = np.floor(self.pos[:, 1]).astype(np.int64) - int(se["crop_y"])
        return fx != px, fy != py


def film(ls):
    """(E (planes, H, W, 4) float64, M, n (H, W) int64) of a lane set"""
    W, H = ls.osc.size
    fp = (ls.flat, ls.inside, ls.wgt)
    E, M = [], []
    for v in ls.values:
        s, m = ref.splat(ls.osc, fp, v)
        E.append(np.moveaxis(s, 0, -1)); M.append(np.moveaxis(m, 0, -1))
    n = np.bincount(ls.flat[ls.inside], minlength=W * H).reshape(H, W)
    return np.stack(E), np.stack(M), n


def bound(M, n):
    return (np.asarray(n, np.float64)[None, :, :, None] + 2.0) * EPS * M


def errors_over_bound(got, E, M, n):
    """per plane and channel the largest |got - E| / ((n + 2) 2^-24 M) over the pixels: (planes, 4).  A pixel without terms must be exactly 0."""
    got, E, M = np.asarray(got, np.float64), np.asarray(E), np.asarray(M)
    assert got.shape == E.shape == M.shape and E.shape[1:3] == n.shape, (got.shape, E.shape, M.shape, n.shape)
    diff = np.abs(got - E)
    empty = M == 0.0
    assert not got[empty].any(), "a pixel and channel without terms is not exactly 0"
    ratio = np.where(empty, 0.0, diff / np.where(empty, 1.0, bound(M, n)))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return ratio.max(axis=(1, 2))


def flagged(ls_mutated, E, M, n):
    """does the criterion, held against the TRUE (E, M, n), see the film of the mutated lane set?  (pixels, channels) over the bound or non-zero where nothing lands"""
    got = film(ls_mutated)[0]
    over = np.abs(got - E) > bound(M, n)
    return int((over | ((M == 0) & (got != 0))).sum())


# ---------------------------------------------------------------------------- mutations
def drop_lane(ls, i):
    out = ls.copy()
    out.inside[i] = False
    return out


def double_lane(ls, i):
    out = ls.copy()
    out.flat, out.inside = np.concatenate([out.flat, out.flat[i:i + 1]]), np.concatenate([out.inside, out.inside[i:i + 1]])
    out.wgt = None if out.wgt is None else np.concatenate([out.wgt, out.wgt[i:i + 1]])
    out.values = [np.concatenate([v, v[i:i + 1]]) for v in out.values]
    return out


def misplace_irregular(ls, orc, i, reweigh=False):
    """lane i (irregular) splatted at its NOMINAL pixel's anchor instead of at floor(pos): its weights, computed for floor(pos), land one pixel off.
    reweigh=True: the weights are evaluated again for the nominal anchor too -- what a kernel WITHOUT a separate path for irregular samples computes.  That is no
    bug for the filters here: a position only floors into the next pixel by rounding up to exactly that integer, the taps then sit at half-integer offsets, the
    outermost of either anchor at n + .5 >= radius where the filter is 0, and the other 2n taps are the same pixels with the same weights
    (test_splat_cpu.test_the_irregular_sample_frames holds that the two films are equal)."""
    ix, iy = ls.irregular()
    assert ix[i] or iy[i], "lane %d is not irregular" % i
    se = ls.osc.flat.sensor
    reach = int(np.ceil(F32(se["filter_radius"]) - F32(.5)))
    px, py = ls.nominal(i)
    first = np.asarray([[px + int(se["crop_x"]) - reach, py + int(se["crop_y"]) - reach]], np.int32)
    flat, inside, wgt = ref.footprint(orc, ls.osc, ls.pos[i:i + 1], ls.spp, first=first)
    out = ls.copy()
    out.flat[i], out.inside[i] = flat[0], inside[0]
    if reweigh:
        out.wgt[i] = wgt[0]
    return out


def swap_channels(ls, i, a=0, b=1):
    out = ls.copy()
    for v in out.values:
        v[i, [a, b]] = v[i, [b, a]]
    return out


def shift_row(ls, i):
    """lane i's taps one pixel row further down; the lane's whole footprint must be inside the window before and after"""
    W, H = ls.osc.size
    assert ls.inside[i].all() and (ls.flat[i] // W + 1 < H).all(), "choose a lane whose footprint and its shifted copy lie inside the window"
    out = ls.copy()
    out.flat[i] = out.flat[i] + W
    return out


def interior_lane(ls):
    """the lane, among those whose footprint stays inside the window when moved one row down, whose first two channels differ most under its largest weight"""
    W, H = ls.osc.size
    v = ls.values[0].astype(np.float64)
    ok = ls.inside.all(axis=1) & (ls.flat // W + 1 < H).all(axis=1)
    assert ok.any(), "no such lane"
    wmax = 1.0 if ls.wgt is None else np.abs(ls.wgt).max(axis=1)
    return int(np.argmax(np.where(ok, np.abs(v[:, 0] - v[:, 1]) * wmax, -1.0)))


def loss_seen(ls, M, n):
    """per lane: would the criterion see this ONE lane lost (or counted twice)?  Either moves every pixel of its footprint by exactly the lane's term there, so it is
    seen where a term is larger than the pixel's bound -- no film has to be splatted again (drop_lane / double_lane give the same answer one lane at a time)."""
    b = bound(M, n).reshape(len(M), -1, 4)
    seen = np.zeros(ls.n_lanes, bool)
    for p, v in enumerate(ls.values):
        for ch in range(4):
            t = np.broadcast_to(v[:, ch, None], ls.flat.shape) if ls.wgt is None else (v[:, ch, None] * ls.wgt).astype(F32)
            seen |= (ls.inside & (np.abs(t.astype(np.float64)) > b[p][:, ch][ls.flat])).any(axis=1)
    return seen
