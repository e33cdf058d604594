"""Denoiser: the joint variance-guided a-trous filter and its temporal stage (dtof_denoise, dtof_denoise_temporal) over host arrays."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import MAX_VARIANTS, DtofError, _check, _DenoiseParams, _ptr, _TemporalBuffers, _TemporalParams


class Denoiser:
    """The counterpart of the reference's mi.OptixDenoiser(input_size, albedo, normals, temporal) (src/render/python/optixdenoiser_v.cpp), written in HIP
    (dtof_denoise): an edge-avoiding a-trous wavelet filter whose luminance term is normalised by the per-pixel variance, over up to four images that share ONE set
    of weights (include/dtof.h has the definition).  `input_size`: (width, height).  `normals`, `position`, `variance`: which guides every call will bring.
    `sigma_position=None`: 1 % of the largest extent of the finite positions of a call, computed with numpy and kept in `last_sigma_position`.  There is no albedo
    guide (the aov film refuses that channel) and no alpha plane.

        denoised = mi.Denoiser((w, h))(noisy)
        denoised, variance = mi.Denoiser((w, h), normals=True, position=True, variance=True)(noisy, normals=n, position=p, variance=v)

    `temporal=True` puts the temporal stage (dtof_denoise_temporal; include/dtof.h has the definition) in front of the spatial levels: every call then takes `flow`
    (H, W, 2), the pixel motion from the previous frame to this one, `ids` (H, W) if declared with `ids=True` (e.g. the aov film's shape_index plane) and `history`,
    None for a first frame or the dict the previous call returned.  The previous frame's accumulated images are reprojected through the flow, history whose id differs
    or whose normal is further than `tau_normal` away is rejected, and mean and variance are blended with weight max(1 / length, alpha_min), the length clamped to
    `max_length`; the spatial levels then filter the accumulated images, guided by the variance of the accumulated estimate.  The call returns the spatial result, its
    variance if one was brought, and the new history: the temporal result ("colour"), its "variance" and "length", and the current "normals" / "ids".  There is no
    world-space position test of the history and no 3 x 3 variance prefilter.

        den = mi.Denoiser((w, h), normals=True, variance=True, temporal=True, ids=True)
        history = None
        for frame in frames:
            denoised, variance, history = den(frame.noisy, normals=frame.n, variance=frame.v, flow=frame.flow, ids=frame.ids, history=history)"""

    def __init__(self, input_size, normals=False, position=False, variance=False, levels=5, sigma_normal=0.1, sigma_position=None, sigma_luminance=4.0,
                 temporal=False, ids=False, alpha_min=0.2, max_length=32, tau_normal=0.25):
        try:
            w, h = (int(v) for v in input_size)
        except (TypeError, ValueError):
            raise DtofError("Denoiser: input_size must be (width, height)")
        if w < 1 or h < 1:
            raise DtofError("Denoiser: input_size must be at least 1 x 1")
        if not 1 <= int(levels) <= 6:
            raise DtofError("Denoiser: levels must be between 1 and 6")
        self.input_size = (w, h)
        self.normals, self.position, self.variance = bool(normals), bool(position), bool(variance)
        self.levels = int(levels)
        self.sigma_normal, self.sigma_position, self.sigma_luminance = float(sigma_normal), None if sigma_position is None else float(sigma_position), float(sigma_luminance)
        self.last_sigma_position = None
        self.temporal, self.ids = bool(temporal), bool(ids)
        if self.ids and not self.temporal:
            raise DtofError("Denoiser: ids belong to the temporal stage (temporal=True)")
        self.alpha_min, self.max_length, self.tau_normal = float(alpha_min), float(max_length), float(tau_normal)
        if self.temporal and not (0 < self.alpha_min <= 1 and 1 <= self.max_length < float("inf") and 0 < self.tau_normal < float("inf")):
            raise DtofError("Denoiser: alpha_min must be in (0, 1], max_length finite and >= 1, tau_normal finite and > 0")

    def _guide(self, name, declared, value, shape, dtype):
        if declared != (value is not None):
            raise DtofError("Denoiser: the denoiser was created with %s=%s, so the call must %s it" % (name, declared, "bring" if declared else "not bring"))
        if value is None:
            return None
        a = np.ascontiguousarray(value, dtype=dtype)
        if a.shape != shape:
            raise DtofError("Denoiser: %s must have the shape %s, not %s" % (name, shape, a.shape))
        return a

    def _history(self, history, k, has_variance, has_normals):
        """the `history` argument of a temporal call -> its arrays in the order of dtof_temporal_buffers (None where the current frame brings no such buffer)"""
        w, h = self.input_size
        if history is None:
            return None, None, None, None, None
        if not isinstance(history, dict):
            raise DtofError("Denoiser: history must be None or the history a previous call returned")
        want = {"colour": ((k, h, w, 3), np.float64, True), "variance": ((k, h, w), np.float64, has_variance), "normals": ((h, w, 3), np.float32, has_normals),
                "ids": ((h, w), np.float32, self.ids), "length": ((h, w), np.float32, True)}
        out = []
        for name, (shape, dtype, needed) in want.items():
            if not needed:
                out.append(None)
                continue
            if history.get(name) is None:
                raise DtofError('Denoiser: the history holds no "%s"; it must come from a call with the same guides' % name)
            a = np.ascontiguousarray(history[name], dtype=dtype)
            if a.shape != shape:
                raise DtofError('Denoiser: the history\'s "%s" must have the shape %s, not %s' % (name, shape, a.shape))
            out.append(a)
        return tuple(out)

    def _accumulate(self, col, var, nrm, flow, ids, history):
        """the temporal stage over host arrays (dtof_denoise_temporal) -> (accumulated colour rounded to float32, its variance, the new history)"""
        k, h, w = col.shape[:3]
        f = self._guide("flow", True, flow, (h, w, 2), np.float32)
        idp = self._guide("ids", self.ids, ids, (h, w), np.float32)
        h_col, h_var, h_nrm, h_ids, h_len = self._history(history, k, var is not None, nrm is not None)
        o_col, o_len, o_f32 = np.zeros((k, h, w, 3), np.float64), np.zeros((h, w), np.float32), np.zeros((k, h, w, 3), np.float32)
        o_var = None if var is None else np.zeros((k, h, w), np.float64)
        arrays = (col, var, nrm, idp, f, h_col, h_var, h_nrm, h_ids, h_len, o_col, o_var, o_len, o_f32)
        buf = _TemporalBuffers(*(_ptr(a) for a in arrays))
        prm = _TemporalParams(self.alpha_min, self.max_length, self.tau_normal)
        _check(_abi._lib().dtof_denoise_temporal(C.byref(buf), k, w, h, C.byref(prm)))
        return o_f32, o_var, {"colour": o_col, "variance": o_var, "length": o_len, "normals": nrm, "ids": idp}

    def __call__(self, noisy, normals=None, position=None, variance=None, flow=None, ids=None, history=None):
        """noisy (H, W, 3) or (K, H, W, 3), K <= 4; normals, position (H, W, 3); variance (H, W) or (K, H, W): the variance of every image's luminance estimate.
        Returns the filtered images as float64 in the shape of `noisy`, and with a variance the tuple (images, filtered variance).  With temporal=True: flow (H, W, 2),
        ids (H, W) if declared, history None or the last element of the previous call's result, which gains the new history as its last element; the history's arrays
        keep the (K, ...) form whatever the shape of `noisy`."""
        w, h = self.input_size
        if not self.temporal and (flow is not None or ids is not None or history is not None):
            raise DtofError("Denoiser: flow, ids and history belong to a denoiser created with temporal=True")
        col = np.ascontiguousarray(noisy, dtype=np.float32)
        single = col.ndim == 3
        if single:
            col = col[None]
        if col.ndim != 4 or col.shape[1:] != (h, w, 3) or not 1 <= col.shape[0] <= MAX_VARIANTS:
            raise DtofError("Denoiser: noisy must be (%d, %d, 3) or (K, %d, %d, 3) with 1 <= K <= 4, not %s" % (h, w, h, w, np.shape(noisy)))
        k = col.shape[0]
        nrm = self._guide("normals", self.normals, normals, (h, w, 3), np.float32)
        pos = self._guide("position", self.position, position, (h, w, 3), np.float32)
        if variance is not None and single and np.ndim(variance) == 2:
            variance = np.asarray(variance)[None]
        var = self._guide("variance", self.variance, variance, (k, h, w), np.float64)
        sigma_x = self.sigma_position
        if pos is not None and sigma_x is None:
            finite = pos[np.isfinite(pos).all(axis=2)].astype(np.float64)
            extent = float((finite.max(axis=0) - finite.min(axis=0)).max()) if len(finite) else 0.0
            sigma_x = 0.01 * extent if extent > 0 else 1.0      # one point: every position difference is 0 whatever the sigma
            self.last_sigma_position = sigma_x
        new_history = None
        if self.temporal:      # the spatial levels below then filter the accumulated images, guided by the accumulated variance
            col, var, new_history = self._accumulate(col, var, nrm, flow, ids, history)
        prm = _DenoiseParams(self.levels, self.sigma_normal, 1.0 if sigma_x is None else sigma_x, self.sigma_luminance)
        out = np.zeros((k, h, w, 3), np.float64)
        out_var = None if var is None else np.zeros((k, h, w), np.float64)
        _check(_abi._lib().dtof_denoise(col.ctypes.data, k, w, h, _ptr(var), _ptr(nrm), _ptr(pos), C.byref(prm), out.ctypes.data, _ptr(out_var)))
        if single:
            out, out_var = out[0], None if out_var is None else out_var[0]
        if self.temporal:
            return (out, new_history) if out_var is None else (out, out_var, new_history)
        return out if out_var is None else (out, out_var)
