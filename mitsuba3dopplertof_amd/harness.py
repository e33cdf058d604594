"""The experiment-driver contract of the reference's tutorials on top of the C ABI:
multi-pass seed averaging, the exact integrator dictionaries, ToF images and velocity maps.

Mirrors doppler_tutorials/src/program_runner.py:11-31 (mean over seeds 0..n-1 of min(1024,total)-spp passes), :33-80 (velocity /
radiance ground truth with the `velocity` / `path` integrators), :82-153 (Doppler render; `antithetic_shift` defaults to 0.5 for
"antithetic" and 0 otherwise) and doppler_tutorials/src/utils/image_utils.py:20-31,140-199 (luminance * exposure time; radial
velocity from the heterodyne / homodyne ratio)."""
import os

import numpy as np

from . import load_dict, load_file, render_multi_pass, to_tof_image   # noqa: F401
from .io import write_npy


def doppler_integrator_dict(wave_function_type="sinusoidal", low_frequency_component_only=True, hetero_frequency=1.0,
                            hetero_offset=0.0, time_sampling_method="antithetic", antithetic_shift=None,
                            path_correlation_depth=16, exposure_time=0.0015, w_g=30, max_depth=4,
                            use_stratified_sampling_for_each_interval=True):
    """The dictionary program_runner.py:127-141 hands to mi.load_dict."""
    if antithetic_shift is None:
        antithetic_shift = 0.5 if time_sampling_method == "antithetic" else 0.0
    return {"type": "dopplertofpath", "is_doppler_integrator": True, "max_depth": max_depth, "w_g": w_g, "time": exposure_time,
            "hetero_frequency": hetero_frequency, "hetero_offset": hetero_offset, "antithetic_shift": antithetic_shift,
            "time_sampling_method": time_sampling_method, "path_correlation_depth": path_correlation_depth,
            "low_frequency_component_only": low_frequency_component_only, "wave_function_type": wave_function_type,
            "use_stratified_sampling_for_each_interval": use_stratified_sampling_for_each_interval}


def _passes(total_spp):
    single = min(1024, total_spp)
    return single, max(total_spp // single, 1)


def run_scene_doppler_tof(scene, total_spp=1024, output_file=None, **integrator_kwargs):
    single, _ = _passes(total_spp)
    img = render_multi_pass(scene, load_dict(doppler_integrator_dict(**integrator_kwargs)), total_spp, single)
    if output_file:
        os.makedirs(os.path.dirname(os.path.abspath(output_file)), exist_ok=True)
        write_npy(output_file, img)
    return img


def run_scene_doppler_tof_offsets(scene, hetero_offsets, total_spp=1024, output_files=None, **integrator_kwargs):
    """The same as run_scene_doppler_tof for SEVERAL hetero_offset values of one otherwise identical setting: every traversal
    of the scene evaluates up to four modulation offsets at once (dtof_render_offsets; the paths do not depend on the offset,
    only the modulation weight does), so an 11-offset row of the experiment grids costs 3 traversals instead of 11.
    Returns the images in the order of `hetero_offsets`."""
    single, n_pass = _passes(total_spp)
    integrator_kwargs = dict(integrator_kwargs)
    integrator_kwargs.pop("hetero_offset", None)
    scene.set_integrator(doppler_integrator_dict(hetero_offset=0.0, **integrator_kwargs))
    images = []
    for g in range(0, len(hetero_offsets), 4):
        group = [float(o) for o in hetero_offsets[g:g + 4]]
        acc = None
        for i in range(n_pass):
            img = scene.render(seed=i, spp=single, offsets=group).astype(np.float32)
            acc = img if acc is None else acc + img
        images += list(acc / np.float32(n_pass))
    if output_files:
        for path, img in zip(output_files, images):
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            write_npy(path, img)
    return images


def run_scene_doppler_tof_variants(scene, variants, total_spp=1024, output_files=None, film="float32", **integrator_kwargs):
    """run_scene_doppler_tof for SEVERAL (hetero_frequency, hetero_offset) pairs of one otherwise identical setting: neither property reaches anything but the
    modulation weight, so every traversal evaluates up to four pairs at once (dtof_render_variants) and the images of one group share their paths.  Same passes and
    seeds as run_scene_doppler_tof_offsets; returns the images in the order of `variants`.  film="float64": every traversal into the float64 film (Scene.render)."""
    single, n_pass = _passes(total_spp)
    integrator_kwargs = dict(integrator_kwargs)
    integrator_kwargs.pop("hetero_offset", None)
    integrator_kwargs.pop("hetero_frequency", None)
    scene.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, **integrator_kwargs))
    images, stats = [], []
    for g in range(0, len(variants), 4):
        group = [(float(f), float(o)) for f, o in variants[g:g + 4]]
        acc = None
        for i in range(n_pass):
            img = scene.render(seed=i, spp=single, variants=group, film=film).astype(np.float32)
            stats.append(scene.last_stats)
            acc = img if acc is None else acc + img
        images += list(acc / np.float32(n_pass))
    scene.pass_stats = stats   # last_stats of every traversal, in order
    if output_files:
        for path, img in zip(output_files, images):
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            write_npy(path, img)
    return images


def run_scene_velocity_map(scene, total_spp=1024, offsets=(0.0, 0.25), film="float32", **integrator_kwargs):
    """The radial velocity map of image_utils.py:170-199 from ONE traversal per pass: the homodyne (hetero_frequency 0) and heterodyne (1) films of every offset are
    variants of the same paths, so their ratio's noise is correlated instead of independent.  Two offsets are the four films of one traversal; more are grouped by
    pairs of offsets.  Returns (velocity map (H, W), {"homodyne": [...], "heterodyne": [...]} ToF images in the order of `offsets`)."""
    offsets = [float(o) for o in offsets]
    variants = []
    for g in range(0, len(offsets), 2):   # a homodyne / heterodyne pair never straddles two traversals
        variants += [(0.0, o) for o in offsets[g:g + 2]] + [(1.0, o) for o in offsets[g:g + 2]]
    images = run_scene_doppler_tof_variants(scene, variants, total_spp, film=film, **integrator_kwargs)
    exposure_time, w_g = integrator_kwargs.get("exposure_time", 0.0015), integrator_kwargs.get("w_g", 30)
    homo, hetero = [], []
    for g in range(0, len(offsets), 2):
        n = len(offsets[g:g + 2])
        homo += [to_tof_image(im, exposure_time) for im in images[2 * g:2 * g + n]]
        hetero += [to_tof_image(im, exposure_time) for im in images[2 * g + n:2 * g + 2 * n]]
    return calc_velocity_from_homo_heteros(homo, hetero, exposure_time, w_g), {"homodyne": homo, "heterodyne": hetero}


def run_scene_velocity_map_device(scene, total_spp=1024, offsets=(0.0, 0.25), film="float32", **integrator_kwargs):
    """run_scene_velocity_map with everything behind the film splat on the GPU (Scene.render_velocity_map): the same integrator, passes, seeds and traversals, but the
    films are developed, averaged and turned into the map by two kernels and only the results cross to the host.  Same return value; the map is bit for bit what
    calc_velocity_from_homo_heteros makes of the returned ToF images."""
    single, n_pass = _passes(total_spp)
    integrator_kwargs = dict(integrator_kwargs)
    integrator_kwargs.pop("hetero_offset", None)
    integrator_kwargs.pop("hetero_frequency", None)
    scene.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, **integrator_kwargs))
    exposure_time, w_g = integrator_kwargs.get("exposure_time", 0.0015), integrator_kwargs.get("w_g", 30)
    return scene.render_velocity_map(n_pass, single, [float(o) for o in offsets], exposure_time, w_g, film=film)


def velocity_map_denoised(scene, n_passes, spp, offsets=(0.0, 0.25), exposure_time=0.0015, w_g=30, **denoiser_kw):
    """The velocity map of the scene's OWN dopplertofpath integrator with the four ToF films of its traversal denoised JOINTLY before the ratio is formed
    (Denoiser): one set of weights for (0, o0), (0, o1), (1, o0), (1, o1), so a pixel's heterodyne / homodyne ratio stays a ratio of identically weighted
    neighbourhoods.  Exactly two offsets: one traversal group.  The films are accumulated over passes of `spp` samples with seeds 0, 1, ... and turned into
    to_tof_image values as run_scene_velocity_map does; the variance of every ToF film is that of the pass mean from the moment film of the same passes and seeds,
    (m2_Y - mean_Y^2) / (passes x spp) times exposure_time^2 (Y of the moment film is a luminance with the coefficients of srgb_to_xyz rather than to_tof_image's
    rounded ones); the guides are the position and shading normal of the aov film.  The luminance of a ToF plane is the plane itself: it is handed to the denoiser
    REPLICATED into three channels (the weights (0.2126 + 0.7152) + 0.0722 sum to 1 up to rounding, and the three outputs are equal) and channel 0 of the result is
    taken -- the C entry has no one-channel path.  These are three traversals per pass (images, moments, aovs) with numpy between the films and the denoiser: the
    host route.  Scene.render_velocity_map_denoised is the device route: one traversal per pass and everything up to the maps on the GPU.
    `denoiser_kw`: levels and the sigmas of Denoiser.  Returns (noisy map (H, W), denoised map (H, W)); the films, their variances, the guides and the Denoiser are
    left in scene.denoise_details."""
    from . import Denoiser
    offsets = [float(o) for o in offsets]
    if len(offsets) != 2:
        raise ValueError("a denoised velocity map takes two offsets: the four films of one traversal")
    variants = [(0.0, o) for o in offsets] + [(1.0, o) for o in offsets]
    acc = None
    for i in range(n_passes):
        img = scene.render(seed=i, spp=spp, variants=variants).astype(np.float32)
        acc = img if acc is None else acc + img
    stats = scene.last_stats
    tof = [to_tof_image(im, exposure_time) for im in acc / np.float32(n_passes)]
    noisy_map = calc_velocity_from_homo_heteros(tof[:2], tof[2:], exposure_time, w_g)
    m = scene.render_moments(seed=0, spp=spp, n_passes=n_passes, variants=variants)
    n_samples = scene.last_stats["n_paths"] / float(tof[0].shape[0] * tof[0].shape[1])           # passes x spp as rendered (spp = 0: the sampler's count)
    variance = moment_statistics(m, n_samples)["variance"][..., 1] / n_samples * (exposure_time * exposure_time)
    guides = scene.render_aovs("p:position,n:sh_normal", seed=0, spp=spp, n_passes=n_passes)
    scene.last_stats = stats
    films = np.stack(tof).astype(np.float32)                                                     # (4, H, W)
    h, w = films.shape[1:]
    den = Denoiser((w, h), normals=True, position=True, variance=True, **denoiser_kw)
    out, out_var = den(np.repeat(films[..., None], 3, axis=3), normals=guides["n"], position=guides["p"], variance=variance)
    out = out[..., 0]
    denoised_map = calc_velocity_from_homo_heteros(list(out[:2]), list(out[2:]), exposure_time, w_g)
    scene.denoise_details = {"homodyne": tof[:2], "heterodyne": tof[2:], "denoised_homodyne": list(out[:2]), "denoised_heterodyne": list(out[2:]),
                             "variance": variance, "denoised_variance": out_var, "guides": guides, "denoiser": den}
    return noisy_map, denoised_map


def run_scene_velocity_map_denoised(scene, total_spp, offsets=(0.0, 0.25), denoiser=None, **integrator_kwargs):
    """velocity_map_denoised under run_scene_velocity_map's integrator dictionary, passes (min(1024, total_spp) samples each) and seeds: the noisy map it returns is
    computed as run_scene_velocity_map computes it.  `denoiser`: a dict of Denoiser keyword arguments (levels, sigmas).  Returns (noisy map, denoised map)."""
    single, n_pass = _passes(total_spp)
    integrator_kwargs = dict(integrator_kwargs)
    integrator_kwargs.pop("hetero_offset", None)
    integrator_kwargs.pop("hetero_frequency", None)
    scene.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, **integrator_kwargs))
    exposure_time, w_g = integrator_kwargs.get("exposure_time", 0.0015), integrator_kwargs.get("w_g", 30)
    return velocity_map_denoised(scene, n_pass, single, offsets, exposure_time, w_g, **(denoiser or {}))


def run_scene_velocity_map_denoised_device(scene, total_spp, offsets=(0.0, 0.25), denoiser=None, details=False, **integrator_kwargs):
    """run_scene_velocity_map_denoised with ONE traversal per pass and everything behind it on the GPU (Scene.render_velocity_map_denoised): the same integrator
    dictionary, passes and seeds; the float64 film, the moment film and the aov film come from the same lanes, and only the maps (and what scene.denoise_details
    holds) cross to the host.  The films are the float64 film's, so the maps are those of the host route up to the float32 film's rounding.  Same return value."""
    single, n_pass = _passes(total_spp)
    integrator_kwargs = dict(integrator_kwargs)
    integrator_kwargs.pop("hetero_offset", None)
    integrator_kwargs.pop("hetero_frequency", None)
    scene.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, **integrator_kwargs))
    exposure_time, w_g = integrator_kwargs.get("exposure_time", 0.0015), integrator_kwargs.get("w_g", 30)
    return scene.render_velocity_map_denoised(n_pass, single, [float(o) for o in offsets], exposure_time, w_g, details=details, **(denoiser or {}))


class TemporalVelocityMap:
    """velocity_map_denoised over the frames of an animation, with the denoiser's temporal stage between the films and the spatial levels: every frame's four ToF
    films are blended with the history of the frames before, reprojected through the flow film (Scene.render_flow times `flow_scale`, the frame interval over
    the exposure) and rejected where the aov film's shape_index or shading normal says the surface is another.  Exactly two offsets, as there.  `denoiser_kw`:
    levels and sigmas of Denoiser, and alpha_min, max_length, tau_normal of its temporal stage.  The loop over the frames' scenes stays with the caller:

        tvm = TemporalVelocityMap((0.0, 0.25), 0.0015, 30)
        for i, scene in enumerate(frames):
            noisy, spatial, temporal = tvm.frame(scene, n_passes, spp, seed=i * n_passes)

    The state is the history of the last frame (`history`; None before the first); `details` holds the last frame's films, variances, guides and flow.  The
    sharded renders and the command line have no temporal mode."""

    def __init__(self, offsets=(0.0, 0.25), exposure_time=0.0015, w_g=30, flow_scale=1.0, **denoiser_kw):
        self.offsets = [float(o) for o in offsets]
        if len(self.offsets) != 2:
            raise ValueError("a denoised velocity map takes two offsets: the four films of one traversal")
        self.exposure_time, self.w_g, self.flow_scale = exposure_time, w_g, float(flow_scale)
        self.temporal_kw = {k: denoiser_kw.pop(k) for k in ("alpha_min", "max_length", "tau_normal") if k in denoiser_kw}
        self.denoiser_kw = denoiser_kw
        self.history, self.details = None, None

    def frame(self, scene, n_passes, spp, seed=0):
        """One frame: passes of `spp` samples with seeds seed, seed + 1, ... -> (noisy map, spatially denoised map, temporally and spatially denoised map), (H, W)"""
        from . import Denoiser
        t, w_g = self.exposure_time, self.w_g
        variants = [(0.0, o) for o in self.offsets] + [(1.0, o) for o in self.offsets]
        acc = None
        for i in range(n_passes):
            img = scene.render(seed=seed + i, spp=spp, variants=variants).astype(np.float32)
            acc = img if acc is None else acc + img
        stats = scene.last_stats
        tof = [to_tof_image(im, t) for im in acc / np.float32(n_passes)]
        noisy_map = calc_velocity_from_homo_heteros(tof[:2], tof[2:], t, w_g)
        m = scene.render_moments(seed=seed, spp=spp, n_passes=n_passes, variants=variants)
        n_samples = scene.last_stats["n_paths"] / float(tof[0].shape[0] * tof[0].shape[1])
        variance = moment_statistics(m, n_samples)["variance"][..., 1] / n_samples * (t * t)
        guides = scene.render_aovs("p:position,n:sh_normal,i:shape_index", seed=seed, spp=spp, n_passes=n_passes)
        flow = (scene.render_flow(seed=seed, spp=spp, n_passes=n_passes) * self.flow_scale).astype(np.float32)
        scene.last_stats = stats
        films = np.repeat(np.stack(tof).astype(np.float32)[..., None], 3, axis=3)      # (4, H, W, 3): a ToF plane replicated, as in velocity_map_denoised
        h, w = films.shape[1:3]
        kw = dict(normals=guides["n"], position=guides["p"], variance=variance)
        spatial, _ = Denoiser((w, h), normals=True, position=True, variance=True, **self.denoiser_kw)(films, **kw)
        den = Denoiser((w, h), normals=True, position=True, variance=True, temporal=True, ids=True, **self.denoiser_kw, **self.temporal_kw)
        # the index plane is a filtered mean: a whole number up to rounding where every sample of the footprint met one shape -- made exact, so that frames compare
        # equal there -- and a fraction on the edges, which matches no history but its own
        ids = np.where(np.abs(guides["i"] - np.rint(guides["i"])) < 1e-4, np.rint(guides["i"]), guides["i"])
        out, out_var, self.history = den(films, flow=flow, ids=ids, history=self.history, **kw)
        maps = [calc_velocity_from_homo_heteros(list(o[:2, ..., 0]), list(o[2:, ..., 0]), t, w_g) for o in (spatial, out)]
        self.details = {"homodyne": tof[:2], "heterodyne": tof[2:], "variance": variance, "denoised_variance": out_var, "guides": guides, "flow": flow, "denoiser": den}
        return noisy_map, maps[0], maps[1]


def camera_flow(position, S_prev, S_cur):
    """The flow of STATIC geometry under a moving camera, for Denoiser(temporal=True): `position` (H, W, 3), the aov film's position plane of the current frame;
    S_prev, S_cur (3, 4), Scene.world_to_pixel() of the previous and of the current frame's scene (what `to_sensor` is for in the reference's denoiser call).
    flow = pix_cur(p) - pix_prev(p) as (H, W, 2) float32: a point's pixel motion from the previous frame to this one.  NaN -- "no history" to the temporal stage --
    where the point is not in front of both cameras.  A pixel whose rays missed carries the plane's 0 and a meaningless flow; its id rejects the history."""
    p = np.concatenate([np.asarray(position, np.float64), np.ones(np.shape(position)[:-1] + (1,))], axis=-1)
    pix = []
    for S in (np.asarray(S_prev, np.float64), np.asarray(S_cur, np.float64)):
        w = p @ S[2]
        with np.errstate(all="ignore"):
            pix.append(np.where((w > 0)[..., None], np.stack([p @ S[0], p @ S[1]], axis=-1) / w[..., None], np.nan))
    return (pix[1] - pix[0]).astype(np.float32)


def run_scene_moments(scene, total_spp=1024, variants=((0, 0), (1, 0)), **integrator_kwargs):
    """The moment film of run_scene_doppler_tof_variants' render: the same integrator dictionary, the same passes (min(1024, total_spp) samples each) and seeds
    0, 1, ..., but ONE Scene.render_moments call whose passes all accumulate into one film.  `variants`: up to four (hetero_frequency, hetero_offset) pairs of one
    traversal -- the default is the homodyne / heterodyne pair of a velocity map.  Returns (the dict of Scene.render_moments, n_samples = passes x spp, the sample
    count moment_statistics and velocity_standard_error take)."""
    single, n_pass = _passes(total_spp)
    integrator_kwargs = dict(integrator_kwargs)
    integrator_kwargs.pop("hetero_offset", None)
    integrator_kwargs.pop("hetero_frequency", None)
    scene.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, **integrator_kwargs))
    m = scene.render_moments(seed=0, spp=single, n_passes=n_pass, variants=[(float(f), float(o)) for f, o in variants])
    return m, single * n_pass


def run_scene_aovs(scene, total_spp, aovs, **integrator_kwargs):
    """The geometry channels along the camera rays of run_scene_doppler_tof's render: the same integrator dictionary, the same passes (min(1024, total_spp) samples
    each) and seeds 0, 1, ... as run_scene_moments, in ONE Scene.render_aovs call whose passes all accumulate into one film.  `aovs`: the `aovs` string of the
    reference's aov integrator.  Returns (the dict of Scene.render_aovs, n_samples = passes x spp)."""
    single, n_pass = _passes(total_spp)
    scene.set_integrator(doppler_integrator_dict(**integrator_kwargs))
    m = scene.render_aovs(aovs, seed=0, spp=single, n_passes=n_pass)
    return m, single * n_pass


def moment_statistics(m, n_samples):
    """Per-pixel sample statistics from the developed dict of Scene.render_moments (all numpy, float64):
        "variance" (K, H, W, 3)   m2 - mean^2 of X, Y, Z: the variance of ONE sample
        "cov_y"    (K, K, H, W)   cross[j, k] - mean_y[j] mean_y[k]: the covariance of the Y of two variants of the same paths (its diagonal is variance[..., 1])
        "stderr"   (K, H, W, 3)   sqrt(max(variance, 0) / n_samples): the standard error of the pixel's mean
    n_samples is passes x spp.  With a filter wider than the box, a pixel's mean is a weighted mean over its neighbours' samples too, so this is the NOMINAL count:
    the effective one is (sum w)^2 / sum w^2 of the pixel."""
    mean, m2, cross = np.asarray(m["mean"], np.float64), np.asarray(m["m2"], np.float64), np.asarray(m["cross"], np.float64)
    variance = m2 - mean ** 2
    mean_y = mean[..., 1]
    cov_y = cross - mean_y[:, None] * mean_y[None, :]
    return {"variance": variance, "cov_y": cov_y, "stderr": np.sqrt(np.maximum(variance, 0.0) / n_samples)}


def velocity_standard_error(m, homodyne, heterodyne, n_samples, exposure_time=0.0015, w_g=30):
    """The standard error of the velocity map of calc_velocity_from_homo_hetero for the variants `homodyne` and `heterodyne` (indices into the dict of
    Scene.render_moments), by the delta method on _velocity_from_ratio.  With a, b the Y means of the two variants and r = b / a:
        Var r   ~ (var_b - 2 r cov_ab + r^2 var_a) / (a^2 n)
        |dv/dr| = 0.5 * 3e8 / (w_g 1e6) / (T (r - 1)^2)
    and the result is sqrt(Var r) |dv/dr|, (H, W) float64.  NaN where a == 0 or r lies outside the open clip interval (-1, 0.999): the map is constant there.
    The exposure-time factor of to_tof_image scales a and b alike and cancels in r (and Y is a luminance with the coefficients of srgb_to_xyz rather than
    to_tof_image's rounded ones).  n_samples is passes x spp -- for filters wider than the box the nominal count, see moment_statistics."""
    st = moment_statistics(m, n_samples)
    mean_y = np.asarray(m["mean"], np.float64)[..., 1]
    a, b = mean_y[homodyne], mean_y[heterodyne]
    var_a, var_b, cov = st["cov_y"][homodyne, homodyne], st["cov_y"][heterodyne, heterodyne], st["cov_y"][homodyne, heterodyne]
    with np.errstate(all="ignore"):
        r = b / a
        var_r = (var_b - 2.0 * r * cov + r * r * var_a) / (a * a * n_samples)
        slope = 0.5 * 3e8 / (w_g * 1e6) / (exposure_time * (r - 1.0) ** 2)
        se = np.sqrt(np.maximum(var_r, 0.0)) * slope
    return np.where((a != 0) & (r > -1.0) & (r < 0.999), se, np.nan)


def velocity_map_adaptive(scene, spp, max_passes, tol_mps, offsets=(0.0, 0.25), base_passes=1, seed=0, exposure_time=0.0015, w_g=30):
    """The velocity map of the scene's OWN dopplertofpath integrator by adaptive sampling (Scene.render_adaptive, mode "velocity"): `base_passes` dense passes of `spp`
    samples, then up to max_passes - base_passes passes over the pixels whose map's standard error -- the delta method of velocity_standard_error, per offset pair, from
    the moment film of the passes so far -- is still above `tol_mps` (m/s).  One or two offsets: the films (0, o), (1, o) of ONE traversal.  The ToF images are
    to_tof_image of the float64 film all passes accumulated into, the map calc_velocity_from_homo_heteros of them.  Returns (map (H, W), its standard-error map (H, W):
    the largest finite error over the pairs, NaN where no pair has a usable ratio, count (H, W): samples rendered in every pixel).  The adaptive estimator is slightly
    biased (pixels that look converged by chance stop early); base_passes and spp bound that.  The result dict is left in scene.adaptive_details."""
    offsets = [float(o) for o in offsets]
    if not 1 <= len(offsets) <= 2:
        raise ValueError("an adaptive velocity map takes one or two offsets: the films of one traversal")
    n = len(offsets)
    variants = [(0.0, o) for o in offsets] + [(1.0, o) for o in offsets]
    r = scene.render_adaptive(seed=seed, spp=spp, base_passes=base_passes, max_passes=max_passes, variants=variants, mode="velocity", tol=tol_mps,
                              pairs=[(k, n + k) for k in range(n)], exposure_time=exposure_time, w_g=w_g)
    tof = [to_tof_image(im, exposure_time) for im in r["images"]]
    scene.adaptive_details = r
    return calc_velocity_from_homo_heteros(tof[:n], tof[n:], exposure_time, w_g), r["metric"], r["count"]


def run_scene_velocity_map_adaptive(scene, spp, max_passes, tol_mps, offsets=(0.0, 0.25), base_passes=1, **integrator_kwargs):
    """velocity_map_adaptive under run_scene_velocity_map's integrator dictionary: passes of `spp` samples with seeds 0, 1, ..., the first `base_passes` of them dense.
    Returns (velocity map from calc_velocity_from_homo_heteros, its standard-error map, count)."""
    integrator_kwargs = dict(integrator_kwargs)
    integrator_kwargs.pop("hetero_offset", None)
    integrator_kwargs.pop("hetero_frequency", None)
    scene.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, **integrator_kwargs))
    exposure_time, w_g = integrator_kwargs.get("exposure_time", 0.0015), integrator_kwargs.get("w_g", 30)
    return velocity_map_adaptive(scene, spp, max_passes, tol_mps, offsets, base_passes=base_passes, exposure_time=exposure_time, w_g=w_g)


def run_scene_velocity(scene, total_spp=1024, output_file=None):
    single, _ = _passes(total_spp)
    img = render_multi_pass(scene, load_dict({"type": "velocity"}), total_spp, single)
    if output_file:
        write_npy(output_file, img)
    return img


def run_scene_radiance(scene, total_spp=1024, max_depth=4, output_file=None):
    single, _ = _passes(total_spp)
    img = render_multi_pass(scene, load_dict({"type": "path", "max_depth": max_depth}), total_spp, single)
    if output_file:
        write_npy(output_file, img)
    return img


def _velocity_from_ratio(ratio, exposure_time, w_g_mhz):
    """ratio = heterodyne / homodyne = dw T / (dw T - 1)  =>  dw = ratio / (T (ratio - 1)); v = -(c / 2) dw / w_g"""
    ratio = np.clip(ratio, -1.0, 0.999)
    delta_w = ratio * (1.0 / exposure_time) / (ratio - 1.0)
    return -(0.5 * delta_w * 3e8 / (w_g_mhz * 1e6))


def calc_velocity_from_homo_hetero(homodyne, heterodyne, exposure_time=0.0015, w_g=30):
    """image_utils.py:140-168 -- per-pixel ratio (0 where the homodyne image vanishes), then the closed form above."""
    homodyne, heterodyne = np.asarray(homodyne, np.float64), np.asarray(heterodyne, np.float64)
    ratio = np.divide(heterodyne, homodyne, out=np.zeros_like(homodyne), where=np.abs(homodyne) > 0)
    return _velocity_from_ratio(ratio, exposure_time, w_g)


def calc_velocity_from_homo_heteros(homodynes, heterodynes, exposure_time=0.0015, w_g=30):
    """image_utils.py:170-199 -- confidence-weighted (|homodyne| + 1e-5 T) mean of the ratios of several offset pairs."""
    num = den = 0.0
    for homodyne, heterodyne in zip(homodynes, heterodynes):
        homodyne, heterodyne = np.asarray(homodyne, np.float64), np.asarray(heterodyne, np.float64)
        ratio = np.divide(heterodyne, homodyne, out=np.zeros_like(homodyne), where=np.abs(homodyne) > 0)
        conf = np.abs(homodyne) + 1e-5 * 0.0015
        num, den = num + ratio * conf, den + conf
    return _velocity_from_ratio(num / den, exposure_time, w_g)


# ------------------------------------------------------------------------------------------------ depth map (the host route of Scene.render_depth_map)
_TWO_PI = 6.283185307179586


def _fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product of two float32 is exact in double; the double sum is rounded to ODD (its error term from the two-sum
    decides), so that the second rounding, to float32, sees what it would have seen of the exact value"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        return _fma32_quiet(a, b, c)


def _fma32_quiet(a, b, c):
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _atan2f(y, x):
    """atan2_ of csrc/dtof_math.h on float32 arrays, operation for operation (every float32 operation rounded once)"""
    f = np.float32
    y, x = np.asarray(y, f), np.asarray(x, f)
    with np.errstate(all="ignore"):
        return _atan2f_quiet(y, x, f)


def _atan2f_quiet(y, x, f):
    xa, ya = np.abs(x), np.abs(y)
    mn, mx = np.where(ya < xa, ya, xa), np.where(xa > ya, xa, ya)
    scale = mn / mx
    z = scale * scale
    z2 = z * z
    z4 = z2 * z2
    p01, p23 = _fma32(z, f(-0.33326497518773606976), f(0.99999934166683966009)), _fma32(z, f(-0.13486708938456973185), f(0.19881342388439013552))
    p45, p6 = _fma32(z, f(-0.37006525670417265220e-1), f(0.83863120428809689910e-1)), f(0.78613793713198150252e-2)
    poly = _fma32(z4, _fma32(z2, p6, p45), _fma32(z2, p23, p01))
    t = scale * poly
    pi = f(3.14159265358979323846)
    t = np.where(ya > xa, f(0.5) * pi - t, t)
    t = np.where(x < 0, pi - t, t)
    r = np.where(y < 0, -t, t)
    return np.where(mx != 0, r, f(0)).astype(f)


def calc_depth_from_homodynes(i_images, q_images, frequencies, max_path_length, _atan2=_atan2f):
    """The depth map of include/dtof.h ("depth map") in numpy, from the float32 ToF images of the homodyne films at hetero_offset 0 (i_images[j]) and 0.25
    (q_images[j]) rendered at frequencies[j] MHz: the wrapped phase atan2(-Q, I) of every frequency and, with two or more, the wrap counts -- tried for the first
    frequency up to max_path_length -- on which the frequencies agree best.  Returns a dict: "depth" (half the path length, metres), "residual" float64, "wraps"
    (F, ...) int32, "amplitude" (F, ...) float64, "phase" (F, ...) float32.  Scene.render_depth_map computes the same words on the device."""
    I = [np.ascontiguousarray(a, np.float32) for a in i_images]
    Q = [np.ascontiguousarray(a, np.float32) for a in q_images]
    n_freq = len(frequencies)
    if not 1 <= n_freq <= 4 or len(I) != n_freq or len(Q) != n_freq:
        raise ValueError("between 1 and 4 frequencies, each with an I and a Q image")
    shape = I[0].shape
    with np.errstate(all="ignore"):
        L = [300.0 / float(f) for f in frequencies]
        ph = [np.asarray(_atan2(-Q[j], I[j]), np.float32).reshape(shape) for j in range(n_freq)]
        w, amp = [], []
        for j in range(n_freq):
            p = ph[j].astype(np.float64)
            p = np.where(p < 0, p + _TWO_PI, p)
            w.append((p / _TWO_PI) * L[j])
            i64, q64 = I[j].astype(np.float64), Q[j].astype(np.float64)
            amp.append(np.sqrt(i64 * i64 + q64 * q64))
        if n_freq == 1:
            return {"depth": 0.5 * w[0], "residual": np.zeros(shape), "wraps": np.zeros((1,) + shape, np.int32), "amplitude": np.stack(amp), "phase": np.stack(ph)}
        n_cand = np.floor(max_path_length / L[0])
        if not 0 <= n_cand <= 4095:
            raise ValueError("max_path_length must give between 1 and 4096 wrap candidates of the first frequency")
        won = np.zeros(shape, bool)
        best_err, best_c = np.zeros(shape), np.zeros(shape)
        best_e, best_m = [np.zeros(shape) for _ in range(n_freq)], [np.zeros(shape) for _ in range(n_freq)]
        for n in range(int(n_cand) + 1):
            c = w[0] + float(n) * L[0]
            err, e, m = np.zeros(shape), [None], [np.full(shape, float(n))]
            for j in range(1, n_freq):
                mj = np.rint((c - w[j]) / L[j])
                mj = np.where(mj < 0, 0.0, mj)
                ej = w[j] + mj * L[j]
                r = ej - c
                err = err + r * r
                e.append(ej); m.append(mj)
            take = np.where(won, err < best_err, err == err)      # the first wins on ties, a NaN never
            won = won | take
            best_err, best_c = np.where(take, err, best_err), np.where(take, c, best_c)
            for j in range(n_freq):
                best_m[j] = np.where(take, m[j], best_m[j])
                if j:
                    best_e[j] = np.where(take, e[j], best_e[j])
        S, num = amp[0], amp[0] * best_c
        for j in range(1, n_freq):
            S, num = S + amp[j], num + amp[j] * best_e[j]
        path = np.where(S > 0, num / S, 0.0)
        nan = np.float64("nan")
        return {"depth": np.where(won, 0.5 * path, nan), "residual": np.where(won, np.sqrt(best_err), nan),
                "wraps": np.stack([np.where(won, best_m[j], -1.0).astype(np.int32) for j in range(n_freq)]),
                "amplitude": np.stack([np.where(won, amp[j], nan) for j in range(n_freq)]),
                "phase": np.stack([np.where(won, ph[j], np.float32("nan")).astype(np.float32) for j in range(n_freq)])}


def _depth_setup(scene, frequencies, max_path_length, integrator_kwargs):
    from ._scene import default_max_path_length
    integrator_kwargs = dict(integrator_kwargs)
    for k in ("hetero_offset", "hetero_frequency", "w_g"):
        integrator_kwargs.pop(k, None)
    freq = [float(np.float32(f)) for f in frequencies]
    scene.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, w_g=freq[0], **integrator_kwargs))
    return freq, default_max_path_length(freq) if max_path_length is None else float(max_path_length), integrator_kwargs.get("exposure_time", 0.0015)


def run_scene_depth_map(scene, total_spp=1024, frequencies=(30.0, 40.0), max_path_length=None, film="float32", **integrator_kwargs):
    """The depth map on the host from ONE traversal per pass and pair of frequencies: the I / Q films of every frequency are (0, 0, f) and (0, 0.25, f) variants of the
    same paths (Scene.render(variants=triples)), averaged over the passes, turned into ToF images and handed to calc_depth_from_homodynes.  Returns its dict with
    "tof", the (2 F, H, W) ToF images in the order of depth_map_variants, added."""
    from ._scene import depth_map_variants
    freq, max_path_length, exposure_time = _depth_setup(scene, frequencies, max_path_length, integrator_kwargs)
    single, n_pass = _passes(total_spp)
    triples = [tuple(float(x) for x in v) for v in depth_map_variants(freq)]
    images, stats = [], []
    for g in range(0, len(triples), 4):
        acc = None
        for i in range(n_pass):
            img = scene.render(seed=i, spp=single, variants=triples[g:g + 4], film=film).astype(np.float32)
            stats.append(scene.last_stats)
            acc = img if acc is None else acc + img
        images += list(acc / np.float32(n_pass))
    scene.pass_stats = stats
    tof = [to_tof_image(im, exposure_time) for im in images]
    out = calc_depth_from_homodynes(tof[0::2], tof[1::2], freq, max_path_length)
    out["tof"] = np.stack(tof)
    return out


def run_scene_depth_map_device(scene, total_spp=1024, frequencies=(30.0, 40.0), max_path_length=None, film="float32", **integrator_kwargs):
    """run_scene_depth_map with everything behind the film splat on the GPU (Scene.render_depth_map): the same integrator, passes, seeds and traversals; the same dict,
    word for word."""
    freq, max_path_length, exposure_time = _depth_setup(scene, frequencies, max_path_length, integrator_kwargs)
    single, n_pass = _passes(total_spp)
    return scene.render_depth_map(n_pass, single, freq, exposure_time, max_path_length, film=film)
