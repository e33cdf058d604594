"""The depth map of include/dtof.h ("depth map") restated in numpy, one pixel at a time in the words of the definition: what k_depth_map (dtof_depth.hip) and
harness.calc_depth_from_homodynes are held to, word for word.  The float32 atan2 is the oracle library's exported orc_atan2f, called through ctypes; everything else
is IEEE double arithmetic on Python floats / numpy float64 scalars."""
import ctypes as C
import math

import numpy as np

TWO_PI = 6.283185307179586
NAN = float("nan")


def atan2f(orc):
    """orc_atan2f as a function of two float32 arrays"""
    fn = orc.lib().orc_atan2f
    fn.restype, fn.argtypes = C.c_float, [C.c_float, C.c_float]

    def call(y, x):
        y, x = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(x, np.float32)
        return np.array([fn(float(a), float(b)) for a, b in zip(y.ravel(), x.ravel())], np.float32).reshape(y.shape)
    return call


def tof_of(rgb_sum, plane, n_passes, exposure_time):
    """tof_of of dtof_reconstruct.h: rgb_sum (planes, n, 3) float32 -> (n,) float32"""
    f = np.float32
    p = np.ascontiguousarray(rgb_sum, f)[plane]
    with np.errstate(all="ignore"):
        r, g, b = p[:, 0] / f(n_passes), p[:, 1] / f(n_passes), p[:, 2] / f(n_passes)
        return ((f(0.2126) * r + f(0.7152) * g) + f(0.0722) * b) * f(exposure_time)


def n_candidates(frequencies, max_path_length):
    return int(math.floor(max_path_length / (300.0 / float(frequencies[0])))) + 1


def depth_pixel(I, Q, ph, frequencies, max_path_length):
    """one pixel: I, Q float32 scalars per frequency, ph their float32 phases -> (depth, residual, [wraps], [amplitude], [phase])"""
    F = len(frequencies)
    L, w, amp = [], [], []
    for j in range(F):
        p = float(ph[j])
        if p < 0:
            p = p + TWO_PI
        frac = p / TWO_PI
        amp.append(math.sqrt(float(I[j]) * float(I[j]) + float(Q[j]) * float(Q[j])))
        L.append(300.0 / float(frequencies[j]))
        w.append(frac * L[j])
    if F == 1:
        return 0.5 * w[0], 0.0, [0], amp, [ph[0]]
    best = None
    for n in range(n_candidates(frequencies, max_path_length)):
        c = w[0] + float(n) * L[0]
        err, e, m = 0.0, [None], [float(n)]
        for j in range(1, F):
            mj = float(np.rint(np.float64((c - w[j]) / L[j])))
            if mj < 0:
                mj = 0.0
            ej = w[j] + mj * L[j]
            r = ej - c
            err = err + r * r
            e.append(ej); m.append(mj)
        if err == err and (best is None or err < best[0]):
            best = (err, c, e, m)
    if best is None:
        return NAN, NAN, [-1] * F, [NAN] * F, [np.float32(NAN)] * F
    err, c, e, m = best
    S, num = amp[0], amp[0] * c
    for j in range(1, F):
        S, num = S + amp[j], num + amp[j] * e[j]
    path = num / S if S > 0 else 0.0
    return 0.5 * path, math.sqrt(err), [int(x) for x in m], amp, [ph[j] for j in range(F)]


def depth_map(atan2, i_tof, q_tof, frequencies, max_path_length):
    """i_tof, q_tof: (F, n) float32 ToF values -> dict of depth (n,), residual (n,), wraps (F, n) int32, amplitude (F, n), phase (F, n) float32"""
    i_tof, q_tof = np.ascontiguousarray(i_tof, np.float32), np.ascontiguousarray(q_tof, np.float32)
    F, n = i_tof.shape
    ph = np.stack([atan2(-q_tof[j], i_tof[j]) for j in range(F)])
    out = {"depth": np.zeros(n), "residual": np.zeros(n), "wraps": np.zeros((F, n), np.int32), "amplitude": np.zeros((F, n)), "phase": np.zeros((F, n), np.float32)}
    with np.errstate(all="ignore"):
        for i in range(n):
            d, r, wr, am, p = depth_pixel(i_tof[:, i], q_tof[:, i], ph[:, i], frequencies, max_path_length)
            out["depth"][i], out["residual"][i] = d, r
            out["wraps"][:, i], out["amplitude"][:, i], out["phase"][:, i] = wr, am, p
    return out


def depth_map_of_sum(atan2, rgb_sum, i_planes, q_planes, frequencies, n_passes, exposure_time, max_path_length):
    """the reference of dtof_depth_map_async: rgb_sum (2 F, n, 3) float32"""
    i_tof = np.stack([tof_of(rgb_sum, p, n_passes, exposure_time) for p in i_planes])
    q_tof = np.stack([tof_of(rgb_sum, p, n_passes, exposure_time) for p in q_planes])
    return depth_map(atan2, i_tof, q_tof, frequencies, max_path_length)


def same_words(a, b):
    """equal word for word; a NaN equals a NaN (payloads are unspecified)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u))) | (np.isnan(a) & np.isnan(b))).all())
