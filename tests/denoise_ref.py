"""The definition of the joint variance-guided a-trous denoiser (include/dtof.h) in numpy float64, vectorised over the pixels, one shifted slice per
tap.  Every operation is the double operation the kernel performs, in its order: taps j outer, i inner, both ascending; squared norms (a a + b b) + c c; the
exponent -((dn + dx) + dl); one weight per tap for all planes and for the variance.  A skipped tap adds +0.0, which changes no partial sum (the sums start at +0.0
and can therefore never be -0.0).

Besides the result it returns an ENVELOPE per level: the same filter with the same weights applied to |colour| at level 0 and to the previous envelope afterwards
(for the variance: w^2 and |variance|).  It bounds what a relative error of the weights or of the sums can do to a pixel, so a tolerance of 2^-40 times the envelope
is a tolerance in units of what the pixel was summed from, not of what may have cancelled."""
import numpy as np

B3 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def luminance(c):
    return (0.2126 * c[..., 0] + 0.7152 * c[..., 1]) + 0.0722 * c[..., 2]


def validity(colour, variance=None, normal=None, position=None):
    """(H, W) bool: every colour word of every plane, every variance and every present guide word of the pixel is finite"""
    ok = np.isfinite(colour).all(axis=(0, 3))
    if variance is not None:
        ok &= np.isfinite(variance).all(axis=0)
    if normal is not None:
        ok &= np.isfinite(normal).all(axis=2)
    if position is not None:
        ok &= np.isfinite(position).all(axis=2)
    return ok


def denoise(colour, variance=None, normal=None, position=None, levels=5, sigma_normal=0.1, sigma_position=1.0, sigma_luminance=4.0):
    """colour (K, H, W, 3), variance (K, H, W) or None, normal / position (H, W, 3) or None -> dict:
        "colour" (K, H, W, 3), "variance" (K, H, W) or None   the result after `levels` levels
        "valid" (H, W)                                         the valid pixels; the others carry the converted input
        "envelope_colour", "envelope_variance"                 lists, one array per level, shaped like the results (0 at invalid pixels)"""
    c = np.array(colour, dtype=np.float64)
    k_planes, h, w = c.shape[:3]
    v = None if variance is None else np.array(variance, dtype=np.float64)
    n = None if normal is None else np.array(normal, dtype=np.float64)
    x = None if position is None else np.array(position, dtype=np.float64)
    valid = validity(c, v, n, x)
    sn2, sx2, sl = float(sigma_normal) * float(sigma_normal), float(sigma_position) * float(sigma_position), float(sigma_luminance)
    env_c, env_v = np.abs(c), None if v is None else np.abs(v)
    envs_c, envs_v = [], []
    with np.errstate(all="ignore"):
        for level in range(levels):
            s = 1 << level
            lum = luminance(c) if v is not None else None                                        # (K, H, W)
            den = None if v is None else sl * np.sqrt(np.where(v > 0.0, v, 0.0))                 # at the centre
            sum_w = np.zeros((h, w))
            acc, acc_e = np.zeros_like(c), np.zeros_like(c)
            acc_v, acc_ev = (None, None) if v is None else (np.zeros_like(v), np.zeros_like(v))
            for j in range(-2, 3):
                for i in range(-2, 3):
                    dy, dx_ = j * s, i * s
                    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx_), min(w, w - dx_)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    p = (slice(y0, y1), slice(x0, x1))
                    q = (slice(y0 + dy, y1 + dy), slice(x0 + dx_, x1 + dx_))
                    e_n = e_x = e_l = 0.0
                    if n is not None:
                        d = n[p] - n[q]
                        e_n = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sn2
                    if x is not None:
                        d = x[p] - x[q]
                        e_x = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sx2
                    if v is not None:
                        e_l = np.zeros((y1 - y0, x1 - x0))
                        for k in range(k_planes):
                            lp, lq, dk = lum[k][p], lum[k][q], den[k][p]
                            d = np.where(dk > 0.0, np.abs(lp - lq) / dk, np.where(lp == lq, 0.0, np.inf))
                            e_l = np.where(d > e_l, d, e_l)
                    wt = (B3[i + 2] * B3[j + 2]) * np.exp(-((e_n + e_x) + e_l))
                    wt = np.where(valid[q], wt, 0.0) + np.zeros((y1 - y0, x1 - x0))
                    sum_w[p] = sum_w[p] + wt
                    for k in range(k_planes):
                        acc[k][p] = acc[k][p] + np.where(valid[q][..., None], wt[..., None] * c[k][q], 0.0)
                        acc_e[k][p] = acc_e[k][p] + np.where(valid[q][..., None], wt[..., None] * env_c[k][q], 0.0)
                        if v is not None:
                            acc_v[k][p] = acc_v[k][p] + np.where(valid[q], (wt * wt) * v[k][q], 0.0)
                            acc_ev[k][p] = acc_ev[k][p] + np.where(valid[q], (wt * wt) * env_v[k][q], 0.0)
            c = np.where(valid[None, :, :, None], acc / sum_w[None, :, :, None], c)
            env_c = np.where(valid[None, :, :, None], acc_e / sum_w[None, :, :, None], 0.0)
            envs_c.append(env_c)
            if v is not None:
                v = np.where(valid[None], acc_v / (sum_w * sum_w)[None], v)
                env_v = np.where(valid[None], acc_ev / (sum_w * sum_w)[None], 0.0)
                envs_v.append(env_v)
    return {"colour": c, "variance": v, "valid": valid, "envelope_colour": envs_c, "envelope_variance": envs_v}
