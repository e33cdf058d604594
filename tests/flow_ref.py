"""The definition of the flow film's per-lane value (include/dtof.h: the flow film) in numpy: float64 operations on float32 inputs, every one the operation the
kernel performs, in its order.  numpy's elementwise float64 arithmetic contracts nothing, so this IS the sequence of IEEE operations the header writes out.

  inputs   p (N, 3) float32 the hit position, time (N,) float32 the ray's time, obj (N,) the hit object (-1: a miss), n_keys per object, `export0` =
           dtof_scene_export kind 0 (per object t0, t1, key0[16], key1[16]), S (3, 4) float64 world to film pixel
  output   (N, 2) float32: +0 on a miss and on an object with n_keys <= 1, the NaN 0x7fc00000 where the point is not in front of the camera at both shutter ends"""
import numpy as np

F32 = np.float32


def row_point(m, x, y, z):
    """a point through the row (m0, m1, m2, m3): ((m0 x + m1 y) + m2 z) + m3"""
    return ((m[..., 0] * x + m[..., 1] * y) + m[..., 2] * z) + m[..., 3]


def flow(p, time, obj, n_keys, export0, S):
    p, time, obj = np.asarray(p, F32), np.asarray(time, F32), np.asarray(obj, np.int64)
    ob = np.asarray(export0, F32).reshape(-1, 34)
    S = np.asarray(S, np.float64)
    out = np.zeros((len(p), 2), F32)
    moving = (obj >= 0) & (np.asarray(n_keys, np.int64)[np.maximum(obj, 0)] > 1)
    if not moving.any():
        return out
    o = ob[obj[moving]].astype(np.float64)
    t0, t1 = o[:, 0], o[:, 1]
    key0, key1 = o[:, 2:18].reshape(-1, 4, 4)[:, :3], o[:, 18:34].reshape(-1, 4, 4)[:, :3]      # (n, 3, 4)
    with np.errstate(all="ignore"):
        x = (time[moving].astype(np.float64) - t0) / (t1 - t0)
        u = np.where(x > 0.0, x, 0.0)
        u = np.where(u < 1.0, u, 1.0)[:, None, None]
        m = key0 * (1.0 - u) + key1 * u
        a00, a01, a02, a10, a11, a12, a20, a21, a22 = (m[:, r, c] for r in range(3) for c in range(3))
        c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
        det = (a00 * c00 + a01 * c01) + a02 * c02
        i_d = 1.0 / det
        inv = np.zeros_like(m)
        inv[:, 0, 0], inv[:, 0, 1], inv[:, 0, 2] = c00 * i_d, (a02 * a21 - a01 * a22) * i_d, (a01 * a12 - a02 * a11) * i_d
        inv[:, 1, 0], inv[:, 1, 1], inv[:, 1, 2] = c01 * i_d, (a00 * a22 - a02 * a20) * i_d, (a02 * a10 - a00 * a12) * i_d
        inv[:, 2, 0], inv[:, 2, 1], inv[:, 2, 2] = c02 * i_d, (a01 * a20 - a00 * a21) * i_d, (a00 * a11 - a01 * a10) * i_d
        tx, ty, tz = m[:, 0, 3], m[:, 1, 3], m[:, 2, 3]
        for r in range(3):
            inv[:, r, 3] = -((inv[:, r, 0] * tx + inv[:, r, 1] * ty) + inv[:, r, 2] * tz)
        px, py, pz = (p[moving, c].astype(np.float64) for c in range(3))
        q = [row_point(inv[:, r], px, py, pz) for r in range(3)]
        P0 = [row_point(key0[:, r], *q) for r in range(3)]
        P1 = [row_point(key1[:, r], *q) for r in range(3)]
        w0, w1 = row_point(S[2][None], *P0), row_point(S[2][None], *P1)
        fx = row_point(S[0][None], *P1) / w1 - row_point(S[0][None], *P0) / w0
        fy = row_point(S[1][None], *P1) / w1 - row_point(S[1][None], *P0) / w0
        front = (w0 > 0.0) & (w1 > 0.0)
        out[moving] = np.where(front[:, None], np.stack([fx, fy], axis=1).astype(F32), F32(np.nan))
    return out
