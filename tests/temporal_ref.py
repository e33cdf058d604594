"""The definition of the denoiser's temporal stage (include/dtof.h) in numpy float64, vectorised over the pixels, one gather per tap.  Every operation
is the double operation the kernel performs, in its order: taps j outer, i inner; the squared norm (a a + b b) + c c; sums in tap order.  A rejected tap adds +0.0,
which changes no partial sum (the sums start at +0.0 and, all weights being > 0, a sum of accepted taps can only be -0.0 if every product is, and +0.0 + -0.0 = +0.0).

Only IEEE double + - * /, floor, min / max written as comparisons, and comparisons: the device is held to these bits exactly (tests/test_temporal_gpu.py)."""
import numpy as np


def cur_ok(colour, variance=None, normal=None, ids=None):
    """(H, W) bool: every colour word of every plane, every variance and every present guide word of the pixel is finite"""
    ok = np.isfinite(colour).all(axis=(0, 3))
    if variance is not None:
        ok &= np.isfinite(variance).all(axis=0)
    if normal is not None:
        ok &= np.isfinite(normal).all(axis=2)
    if ids is not None:
        ok &= np.isfinite(ids)
    return ok


def temporal(colour, flow, variance=None, normal=None, ids=None, history=None, alpha_min=0.2, max_length=32.0, tau_normal=0.25):
    """colour (K, H, W, 3) float32, flow (H, W, 2) float32, variance (K, H, W) float64 or None, normal (H, W, 3) / ids (H, W) float32 or None;
    history None or a dict "colour" (K, H, W, 3) float64, "length" (H, W) float32 and "variance", "normal", "ids" for every present buffer of the current frame ->
    dict "colour" float64, "variance" float64 or None, "length" float32, "colour_f32" float32, "accepted" (H, W) int: the taps each pixel accepted"""
    c32 = np.asarray(colour, dtype=np.float32)
    c = c32.astype(np.float64)
    k_planes, h, w = c.shape[:3]
    v = None if variance is None else np.asarray(variance, dtype=np.float64)
    n = None if normal is None else np.asarray(normal, dtype=np.float32).astype(np.float64)
    idp = None if ids is None else np.asarray(ids, dtype=np.float32)
    f = np.asarray(flow, dtype=np.float32)
    ok = cur_ok(c, v, n, idp)
    alpha_min, max_length = float(alpha_min), float(max_length)
    tau2 = float(tau_normal) * float(tau_normal)

    sw, sn = np.zeros((h, w)), np.zeros((h, w))
    sc = np.zeros_like(c)
    sv = None if v is None else np.zeros_like(v)
    accepted = np.zeros((h, w), np.int64)
    with np.errstate(all="ignore"):
        if history is not None:
            hc = np.asarray(history["colour"], dtype=np.float64)
            hl = np.asarray(history["length"], dtype=np.float32)
            hv = None if v is None else np.asarray(history["variance"], dtype=np.float64)
            hn = None if n is None else np.asarray(history["normal"], dtype=np.float32).astype(np.float64)
            hi = None if idp is None else np.asarray(history["ids"], dtype=np.float32)
            yy, xx = np.mgrid[0:h, 0:w]
            flow_ok = np.isfinite(f).all(axis=2)
            fx, fy = np.where(flow_ok, f[..., 0], 0).astype(np.float64), np.where(flow_ok, f[..., 1], 0).astype(np.float64)
            rx, ry = xx.astype(np.float64) - fx, yy.astype(np.float64) - fy
            x0, y0 = np.floor(rx), np.floor(ry)
            a, b = rx - x0, ry - y0
            for j in range(2):
                for i in range(2):
                    wt = (a if i else 1.0 - a) * (b if j else 1.0 - b)
                    qx, qy = x0 + float(i), y0 + float(j)
                    take = ok & flow_ok & (wt > 0.0) & (qx >= 0.0) & (qx <= float(w - 1)) & (qy >= 0.0) & (qy <= float(h - 1))     # on the doubles
                    ix, iy = np.where(take, qx, 0.0).astype(np.int64), np.where(take, qy, 0.0).astype(np.int64)
                    take &= hl[iy, ix] > np.float32(0)
                    take &= np.isfinite(hc[:, iy, ix]).all(axis=(0, 3))
                    if hv is not None:
                        take &= np.isfinite(hv[:, iy, ix]).all(axis=0)
                    if hi is not None:
                        take &= np.isfinite(hi[iy, ix]) & (hi[iy, ix] == idp)
                    if hn is not None:
                        d = n - hn[iy, ix]
                        take &= np.isfinite(hn[iy, ix]).all(axis=2) & (((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) <= tau2)
                    accepted += take
                    sw = sw + np.where(take, wt, 0.0)
                    sc = sc + np.where(take[None, :, :, None], wt[None, :, :, None] * hc[:, iy, ix], 0.0)
                    if hv is not None:
                        sv = sv + np.where(take[None], wt[None] * hv[:, iy, ix], 0.0)
                    sn = sn + np.where(take, wt * hl[iy, ix].astype(np.float64), 0.0)
        blend = sw > 0.0
        den = np.where(blend, sw, 1.0)
        n1 = sn / den + 1.0
        length = np.where(n1 < max_length, n1, max_length)
        r = 1.0 / length
        alpha = np.where(r > alpha_min, r, alpha_min)
        keep = 1.0 - alpha
        o_colour = np.where(blend[None, :, :, None], keep[None, :, :, None] * (sc / den[None, :, :, None]) + alpha[None, :, :, None] * c, c)
        o_variance = None if v is None else np.where(blend[None], (keep * keep)[None] * (sv / den[None]) + (alpha * alpha)[None] * v, v)
        o_length = np.where(blend, length.astype(np.float32), np.where(ok, np.float32(1), np.float32(0))).astype(np.float32)
        return {"colour": o_colour, "variance": o_variance, "length": o_length, "colour_f32": o_colour.astype(np.float32), "accepted": accepted}
