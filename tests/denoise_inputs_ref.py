"""The numpy definition of the stage between the raw films of one traversal and the denoiser's arguments (dtof_denoise_inputs_async, csrc/dtof_denoise_inputs.hip;
the tail of dtof_render_denoised / dtof_render_velocity_map_denoised).  Nothing here touches the library under test.  Every operation is the one
Scene.render_denoised and harness.velocity_map_denoised perform inline on the developed dicts, in their order; tests/test_denoise_inputs_cpu.py holds it to the
harness's own expressions.

  sum        (K, n, 3) float32: the sum of the developed passes
  moments    (P(K), n) float64: the RAW planes of the moment film (dtof.h: 0 the weight, 1 + 6 k + 1 sum w Y_k, 1 + 6 k + 4 sum w Y_k^2)
  aovs       (7, n) float64: the RAW planes of the aov film of "p:position,n:sh_normal" (weight, position x y z, normal x y z)
"""
import numpy as np

F32 = np.float32
IMAGE, TOF = 0, 1


def tof_image(mean, exposure_time):
    """to_tof_image (mitsuba3dopplertof_amd.to_tof_image) on a float32 image (..., 3): the Python scalars stay weak against float32"""
    return ((0.2126 * mean[..., 0] + 0.7152 * mean[..., 1]) + 0.0722 * mean[..., 2]) * exposure_time


def inputs(mode, total, moments, aovs, n_passes, n_samples, exposure_time=0.0015):
    """-> (colour (K, n, 3) float32, variance (K, n) float64, normal (n, 3) float32, position (n, 3) float32)"""
    total, moments, aovs = np.asarray(total, F32), np.asarray(moments, np.float64), np.asarray(aovs, np.float64)
    K = total.shape[0]
    with np.errstate(all="ignore"):
        mean_image = total / F32(n_passes)
        if mode == TOF:
            colour = np.repeat(tof_image(mean_image, exposure_time).astype(F32)[..., None], 3, axis=-1)
        else:
            colour = mean_image
        wd = np.where(moments[0] == 0.0, 1.0, moments[0])
        mean = np.stack([moments[1 + 6 * k + 1] / wd for k in range(K)])
        m2 = np.stack([moments[1 + 6 * k + 4] / wd for k in range(K)])
        variance = (m2 - mean ** 2) / n_samples
        if mode == TOF:
            variance = variance * (exposure_time * exposure_time)
        wa = np.where(aovs[0] == 0.0, 1.0, aovs[0])
        position = np.stack([aovs[1 + c] / wa for c in range(3)], axis=-1).astype(F32)
        normal = np.stack([aovs[4 + c] / wa for c in range(3)], axis=-1).astype(F32)
    return np.ascontiguousarray(colour, F32), variance, normal, position


def extent_words(position):
    """the eight words the reduction leaves: (min (3,) float32, max (3,) float32, count) over the pixels whose three words are finite; +inf / -inf without one"""
    p = np.asarray(position, F32).reshape(-1, 3)
    finite = p[np.isfinite(p).all(axis=1)]
    if len(finite) == 0:
        return np.full(3, np.inf, F32), np.full(3, -np.inf, F32), 0
    return finite.min(axis=0), finite.max(axis=0), len(finite)


def sigma_position(position):
    """Denoiser.__call__'s automatic sigma_position, word for word"""
    pos = np.asarray(position, F32).reshape(-1, 1, 3)
    finite = pos[np.isfinite(pos).all(axis=2)].astype(np.float64)
    extent = float((finite.max(axis=0) - finite.min(axis=0)).max()) if len(finite) else 0.0
    return 0.01 * extent if extent > 0 else 1.0


def same_bits(a, b, nan_equal=False):
    """bit for bit; nan_equal: two NaNs count as equal whatever their payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    eq = a.view(u) == b.view(u)
    if nan_equal:
        eq = eq | (np.isnan(a) & np.isnan(b))
    return bool(eq.all())
