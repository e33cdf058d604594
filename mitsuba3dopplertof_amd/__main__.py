"""Command line front end mirroring `mitsuba scene.xml -D key=value -o out` (src/mitsuba/mitsuba.cpp:150-423) for the
plugins this library implements:

    python -m mitsuba3dopplertof_amd scene.xml [-D key=value ...] [-o out.exr|.npy|.pfm] [--spp N] [--seed S]
                                               [--offsets 0,0.25,0.5,0.75] [--film float64] [-v]
    python -m mitsuba3dopplertof_amd scene.xml --velocity-map 0,0.25 [--w-g 30 --exposure-time 0.0015] [--spp N] [-o out.npy]
        the radial-velocity map of the scene's dopplertofpath integrator (float64 .npy), reconstructed on the GPU: passes of min(1024, N) samples, seeds 0, 1, ...
    python -m mitsuba3dopplertof_amd scene.xml --depth-map 30,40 [--max-path-length M] [--exposure-time 0.0015] [--film float64] [--spp N] [-o out.npy]
        the depth map (metres, float64 .npy) from the homodyne I / Q films at the given modulation frequencies (MHz), two frequencies per traversal, reconstructed and
        unwrapped on the GPU (Scene.render_depth_map); the wrap counts and the residual go to the output's _wraps and _residual siblings
    python -m mitsuba3dopplertof_amd scene.xml --variants 0:0:30,0:0.25:30,0:0:40,0:0.25:40 [--spp N] [-o out.exr]
        one image per hetero_frequency:hetero_offset:w_g triple, every four of them from one traversal (<out>_variant_<k>)
    python -m mitsuba3dopplertof_amd scene.xml --moments [--variants 0:0,1:0] [--passes N] [--spp N] [-o out.npz]
        the per-pixel moment film of one traversal per pass (weight, mean, m2, cross: Scene.render_moments), written with np.savez
    python -m mitsuba3dopplertof_amd scene.xml --aovs dd:depth,nn:sh_normal [--passes N] [--spp N] [-o out.npz]
        the geometry channels of the reference's `aov` integrator along the scene integrator's camera rays (Scene.render_aovs), written with np.savez
    python -m mitsuba3dopplertof_amd scene.xml --denoise [--denoise-route host|device] [--denoise-levels 5] [--denoise-sigma n,x,l] [--velocity-map 0,0.25] [--spp N] [-o out.exr|.npy]
        the image (or, with --velocity-map and two offsets, the velocity map) with the joint variance-guided a-trous denoiser behind the films (Denoiser): the
        denoised result goes to the output file, the noisy one to its _noisy sibling
    python -m mitsuba3dopplertof_amd scene.xml --adaptive TOL [--adaptive-mode image|velocity] [--base-passes 1] [--max-passes 4] [--variants ...] [--velocity-map 0,0.25]
        adaptive sampling (Scene.render_adaptive): dense base passes, then passes over the pixels whose estimated error is still above TOL -- the relative standard
        error of the image, or with --adaptive-mode velocity and --velocity-map the standard error of the map in m/s; the count map goes to the output's _count sibling
    python -m torch.distributed.run --nproc-per-node G --master-addr 127.0.0.1 -m mitsuba3dopplertof_amd scene.xml ...
        one process per GPU: the pixel rows are sharded across the G ranks, rank 0 gathers and writes the image
"""
import argparse
import os
import sys
import time

import numpy as np


def parser():
    ap = argparse.ArgumentParser(prog="python -m mitsuba3dopplertof_amd", description=__doc__.split("\n\n")[0])
    ap.add_argument("scene")
    ap.add_argument("-D", "--define", action="append", default=[], metavar="key=value",
                    help="define a constant that scene files reference as $key (mitsuba.cpp:241-248)")
    ap.add_argument("-o", "--output", default=None, help="output file (.exr, .npy or .pfm); default: <scene>.exr")
    ap.add_argument("--spp", type=int, default=0, help="samples per pixel (0 = the sampler's sample_count)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--offsets", default=None, help="comma separated hetero_offset values evaluated in ONE traversal")
    ap.add_argument("--stripes", type=int, default=0, metavar="ROWS",
                    help="multi-GPU runs: interleave stripes of ROWS pixel rows across the ranks (load balance) instead of one contiguous band per rank")
    ap.add_argument("-m", "--mode", default="hip_rgb", help="accepted for command-line compatibility (only hip_rgb exists)")
    ap.add_argument("--velocity-map", default=None, metavar="OFFSETS",
                    help="comma separated hetero_offset values: write the radial-velocity map of their homodyne / heterodyne films (float64 .npy) instead of an image")
    ap.add_argument("--depth-map", default=None, metavar="MHZ",
                    help="comma separated modulation frequencies in MHz (1 .. 4, distinct): write the depth map of their homodyne I / Q films (float64 .npy, metres) "
                         "instead of an image; wrap counts and residual go to the _wraps and _residual siblings")
    ap.add_argument("--max-path-length", type=float, default=None, metavar="M",
                    help="--depth-map: the longest path (metres) the unwrapping tries; default 300 / gcd of whole-MHz frequencies")
    ap.add_argument("--w-g", type=float, default=30.0, help="--velocity-map: illumination frequency in MHz")
    ap.add_argument("--exposure-time", type=float, default=0.0015, help="--velocity-map, --depth-map: exposure time in seconds")
    ap.add_argument("--film", default="float32", choices=("float32", "float64"),
                    help="the film's accumulator: float64 sums the splat in double on the GPU (order-independent images and velocity maps; single GPU)")
    ap.add_argument("--moments", action="store_true",
                    help="write the per-pixel moment film (sample mean, second moments and the variants' cross moments, float64 .npz) instead of an image")
    ap.add_argument("--variants", default=None, metavar="F:O,F:O",
                    help="--moments: up to four hetero_frequency:hetero_offset pairs evaluated in ONE traversal (default: the integrator's own pair); alone: "
                         "hetero_frequency:hetero_offset:w_g triples, one image each at its own illumination frequency (MHz)")
    ap.add_argument("--passes", type=int, default=1, help="--moments, --aovs: passes with seeds --seed, --seed + 1, ... that accumulate into one film")
    ap.add_argument("--aovs", default=None, metavar="NAME:TYPE,...",
                    help="write the geometry channels under each pixel (depth, position, uv, geo_normal, sh_normal, dp_du, dp_dv, prim_index, shape_index; float64 "
                         ".npz) instead of an image: the `aovs` string of the reference's aov integrator")
    ap.add_argument("--denoise", action="store_true",
                    help="denoise the image, or the four films of a --velocity-map of two offsets, guided by the moment film's variance and the aov film's position and "
                         "shading normal (three traversals); the noisy result is written to the output's _noisy sibling")
    ap.add_argument("--denoise-levels", type=int, default=None, metavar="L", help="--denoise: a-trous levels, 1 .. 6 (default 5)")
    ap.add_argument("--denoise-route", default="host", choices=("host", "device"),
                    help="--denoise: host renders the images, the moment film and the aov film in three traversals and forms the denoiser's arguments with numpy; "
                         "device renders the three films in ONE traversal and keeps everything up to the result on the GPU (the float64 film's images)")
    ap.add_argument("--denoise-sigma", default=None, metavar="N,X,L",
                    help="--denoise: sigma_normal,sigma_position,sigma_luminance (default 0.1, 1 %% of the scene's extent, 4)")
    ap.add_argument("--adaptive", type=float, default=None, metavar="TOL",
                    help="adaptive sampling: after the dense base passes, render only the pixels whose estimated error is still above TOL (slightly biased: pixels "
                         "that look converged by chance stop early); the per-pixel sample counts are written next to the output (_count.npy)")
    ap.add_argument("--adaptive-mode", default="image", choices=("image", "velocity"),
                    help="--adaptive: TOL is a relative standard error of the image, or (with --velocity-map) the standard error of the velocity map in m/s")
    ap.add_argument("--base-passes", type=int, default=1, help="--adaptive: dense passes before the first selection")
    ap.add_argument("--max-passes", type=int, default=4, help="--adaptive: passes at most, the base passes included")
    ap.add_argument("-v", "--verbose", action="store_true")
    return ap


def check_adaptive_args(ap, args):
    """what --adaptive cannot be combined with, refused before the scene is loaded"""
    if args.moments or args.aovs is not None or args.denoise:
        ap.error("--adaptive renders an image or a velocity map: do not combine it with --moments, --aovs or --denoise")
    if args.stripes > 0 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--adaptive is a single-GPU feature: it cannot be combined with --stripes or a multi-GPU launch")
    if args.offsets is not None:
        ap.error("--adaptive takes --variants (hetero_frequency:hetero_offset pairs) or --velocity-map, not --offsets")
    if not args.adaptive == args.adaptive or args.adaptive < 0:
        ap.error("--adaptive expects a tolerance >= 0")
    if args.base_passes < 1 or args.max_passes < args.base_passes:
        ap.error("--base-passes must be at least 1 and --max-passes at least --base-passes")
    if (args.adaptive_mode == "velocity") != (args.velocity_map is not None):
        ap.error("--adaptive-mode velocity and --velocity-map go together: the tolerance of a velocity map is its standard error in m/s")
    if args.velocity_map is not None:
        if args.variants is not None:
            ap.error("--adaptive with --velocity-map renders the map's own variants: --variants does not apply")
        if not 1 <= len(args.velocity_map.split(",")) <= 2:
            ap.error("--adaptive with --velocity-map takes one or two offsets: the films of one traversal")
    elif args.variants is not None:
        try:
            n = len(parse_variants(args.variants))
        except ValueError:
            ap.error("--variants expects comma separated hetero_frequency:hetero_offset pairs")
        if not 1 <= n <= 4:
            ap.error("--variants takes between 1 and 4 pairs")


def _count_sibling(path):
    return os.path.splitext(path)[0] + "_count.npy"


def adaptive(args, scene):
    """--adaptive: Scene.render_adaptive (image mode: the images of the variants) or harness.velocity_map_adaptive (--velocity-map); the count map beside the output"""
    from mitsuba3dopplertof_amd.io import write_image
    t0 = time.time()
    if args.velocity_map is not None:
        from mitsuba3dopplertof_amd.harness import velocity_map_adaptive
        out = args.output or os.path.splitext(args.scene)[0] + "_velocity.npy"
        v, se, count = velocity_map_adaptive(scene, args.spp, args.max_passes, args.adaptive, [float(x) for x in args.velocity_map.split(",")],
                                             base_passes=args.base_passes, exposure_time=args.exposure_time, w_g=args.w_g)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        np.save(out, v)
        np.save(os.path.splitext(out)[0] + "_stderr.npy", se)
    else:
        out = args.output or os.path.splitext(args.scene)[0] + ".exr"
        variants = parse_variants(args.variants) if args.variants else None
        r = scene.render_adaptive(seed=args.seed, spp=args.spp, base_passes=args.base_passes, max_passes=args.max_passes, variants=variants, mode="image", tol=args.adaptive)
        count = r["count"]
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        if variants is None:
            write_image(out, r["images"][0])
        else:
            base, ext = os.path.splitext(out)
            for k in range(len(variants)):
                write_image("%s_variant_%d%s" % (base, k, ext), r["images"][k])
    np.save(_count_sibling(out), count)
    if args.verbose:
        print("Adaptive render finished. (took %.1f ms, samples per pixel %d .. %d, mean %.1f, %s)"
              % ((time.time() - t0) * 1e3, count.min(), count.max(), count.mean(), scene.last_stats))
    return 0


def check_denoise_args(ap, args):
    """what --denoise cannot be combined with, refused before the scene is loaded -> the keyword arguments of Denoiser"""
    if args.moments or args.aovs is not None:
        ap.error("--denoise filters an image or a velocity map: --moments and --aovs write the films it is guided by, run them separately")
    if args.stripes > 0 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--denoise is a single-GPU feature: it cannot be combined with --stripes or a multi-GPU launch")
    if args.film == "float64" and args.denoise_route == "device":
        ap.error("--denoise-route device renders the float64 film already: do not combine it with --film float64")
    if args.film == "float64":
        ap.error("--denoise reads the float32 images: do not combine it with --film float64")
    if args.offsets is not None:
        ap.error("--denoise takes the integrator's own image or a --velocity-map, not --offsets")
    kw = {}
    if args.denoise_levels is not None:
        if not 1 <= args.denoise_levels <= 6:
            ap.error("--denoise-levels must be between 1 and 6")
        kw["levels"] = args.denoise_levels
    if args.denoise_sigma is not None:
        try:
            sn, sx, sl = (float(x) for x in args.denoise_sigma.split(","))
        except ValueError:
            ap.error("--denoise-sigma expects three comma separated numbers: normal,position,luminance")
        if not all(np.isfinite(v) and v > 0 for v in (sn, sx, sl)):
            ap.error("--denoise-sigma: every sigma must be finite and > 0")
        kw.update(sigma_normal=sn, sigma_position=sx, sigma_luminance=sl)
    if args.velocity_map is not None and len(args.velocity_map.split(",")) != 2:
        ap.error("--denoise with --velocity-map takes two offsets: the four films of one traversal share their weights")
    return kw


def _noisy_sibling(path):
    base, ext = os.path.splitext(path)
    return base + "_noisy" + ext


def check_film_args(ap, args):
    """what --film float64 cannot be combined with, refused before the scene is loaded: the multi-GPU film exchange (and dtof-render --gpus) is float32"""
    if args.film == "float64" and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.stripes > 0):
        ap.error("--film float64 is a single-GPU feature: the sharded and striped multi-GPU renders (and dtof-render --gpus) keep the float32 film")


def check_velocity_map_args(ap, args):
    """what --velocity-map cannot be combined with, refused before the scene is loaded"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--velocity-map is a single-GPU feature")
    if args.offsets is not None:
        ap.error("--velocity-map takes its own offsets: do not combine it with --offsets")
    if args.seed != 0:
        ap.error("--velocity-map renders the seeds 0, 1, ... of its passes: --seed does not apply")
    if args.output is not None and not args.output.lower().endswith(".npy"):
        ap.error("--velocity-map writes a float64 .npy file")
    try:
        [float(x) for x in args.velocity_map.split(",")]
    except ValueError:
        ap.error("--velocity-map expects comma separated numbers")


def parse_variants(text, triples=False):
    """'f:o,f:o,...' -> [(hetero_frequency, hetero_offset), ...]; triples=True: 'f:o:w_g,...' -> [(hetero_frequency, hetero_offset, w_g_mhz), ...].  Anything else,
    a mixture of the two included, is a ValueError."""
    out = []
    for item in text.split(","):
        parts = item.split(":")
        if len(parts) != (3 if triples else 2):
            raise ValueError("--variants expects hetero_frequency:hetero_offset%s items" % (":w_g" if triples else ""))
        out.append(tuple(float(x) for x in parts))
    return out


def check_variant_triples(ap, args):
    """--variants without --moments / --adaptive: hetero_frequency:hetero_offset:w_g triples of a plain render, refused before the scene is loaded"""
    try:
        parse_variants(args.variants, triples=True)
    except ValueError:
        ap.error("--variants and --passes belong to --moments; alone, --variants takes hetero_frequency:hetero_offset:w_g triples (all of them triples)")
    if args.offsets is not None:
        ap.error("--variants replaces --offsets: do not combine them")
    if args.stripes > 0 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--variants is a single-GPU feature: it cannot be combined with --stripes or a multi-GPU launch")
    if args.velocity_map is not None or args.denoise:
        ap.error("--variants triples make plain images: do not combine them with --velocity-map or --denoise")


def check_depth_map_args(ap, args):
    """what --depth-map cannot be combined with, refused before the scene is loaded"""
    if args.velocity_map is not None or args.moments or args.aovs is not None or args.adaptive is not None or args.denoise:
        ap.error("--depth-map is an output of its own: do not combine it with --velocity-map, --moments, --aovs, --adaptive or --denoise")
    if args.stripes > 0 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--depth-map is a single-GPU feature")
    if args.offsets is not None or args.variants is not None:
        ap.error("--depth-map renders its own films: do not combine it with --offsets or --variants")
    if args.seed != 0:
        ap.error("--depth-map renders the seeds 0, 1, ... of its passes: --seed does not apply")
    if args.output is not None and not args.output.lower().endswith(".npy"):
        ap.error("--depth-map writes a float64 .npy file")
    try:
        f = [float(x) for x in args.depth_map.split(",")]
    except ValueError:
        ap.error("--depth-map expects comma separated numbers")
    if not 1 <= len(f) <= 4 or len(set(np.float32(x) for x in f)) != len(f) or not all(np.isfinite(x) and x > 0 for x in f):
        ap.error("--depth-map takes between 1 and 4 distinct frequencies, each finite and > 0")
    if args.max_path_length is None and any(x != int(x) for x in f):
        ap.error("--depth-map: --max-path-length is required unless every frequency is a whole number of MHz")
    if args.max_path_length is not None and not (np.isfinite(args.max_path_length) and args.max_path_length >= 0):
        ap.error("--max-path-length must be finite and >= 0")


def check_moments_args(ap, args):
    """what --moments cannot be combined with, refused before the scene is loaded"""
    if args.velocity_map is not None:
        ap.error("--moments and --velocity-map are two outputs: run them separately")
    if args.stripes > 0 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--moments is a single-GPU feature: it cannot be combined with --stripes or a multi-GPU launch")
    if args.film == "float64":
        ap.error("--moments accumulates in double already: do not combine it with --film float64")
    if args.offsets is not None:
        ap.error("--moments takes --variants (hetero_frequency:hetero_offset pairs), not --offsets")
    if args.passes < 1:
        ap.error("--passes must be at least 1")
    if args.output is not None and not args.output.lower().endswith(".npz"):
        ap.error("--moments writes a float64 .npz file")
    if args.variants is not None:
        try:
            n = len(parse_variants(args.variants))
        except ValueError:
            ap.error("--variants expects comma separated hetero_frequency:hetero_offset pairs")
        if not 1 <= n <= 4:
            ap.error("--variants takes between 1 and 4 pairs")


def check_aovs_args(ap, args):
    """what --aovs cannot be combined with, refused before the scene is loaded"""
    if args.moments:
        ap.error("--aovs and --moments are two outputs: run them separately")
    if args.velocity_map is not None:
        ap.error("--aovs and --velocity-map are two outputs: run them separately")
    if args.stripes > 0 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--aovs is a single-GPU feature: it cannot be combined with --stripes or a multi-GPU launch")
    if args.film == "float64":
        ap.error("--aovs accumulates in double already: do not combine it with --film float64")
    if args.offsets is not None or args.variants is not None:
        ap.error("--aovs records geometry, which no modulation changes: --offsets and --variants do not apply")
    if args.passes < 1:
        ap.error("--passes must be at least 1")
    if args.output is not None and not args.output.lower().endswith(".npz"):
        ap.error("--aovs writes a float64 .npz file")
    import mitsuba3dopplertof_amd as mi
    try:
        if not mi.aov_channels(args.aovs):
            ap.error("--aovs names no channel")
    except mi.DtofError as e:
        ap.error("--aovs: %s" % e)


def aovs(args, scene):
    """--aovs: Scene.render_aovs of --passes passes, the dict written with np.savez"""
    out = args.output or os.path.splitext(args.scene)[0] + "_aovs.npz"
    t0 = time.time()
    m = scene.render_aovs(args.aovs, seed=args.seed, spp=args.spp, n_passes=args.passes)
    dt = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **m)
    if args.verbose:
        print("AOV film finished. (took %.1f ms, %d passes, %s)" % (dt * 1e3, args.passes, scene.last_stats))
    return 0


def moments(args, scene):
    """--moments: Scene.render_moments of --passes passes, the dict written with np.savez"""
    out = args.output or os.path.splitext(args.scene)[0] + "_moments.npz"
    t0 = time.time()
    m = scene.render_moments(seed=args.seed, spp=args.spp, n_passes=args.passes, variants=parse_variants(args.variants) if args.variants else None)
    dt = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **m)
    if args.verbose:
        print("Moment film finished. (took %.1f ms, %d passes, %s)" % (dt * 1e3, args.passes, scene.last_stats))
    return 0


def _sibling(path, tag):
    base, ext = os.path.splitext(path)
    return base + "_" + tag + ext


def depth_map(args, scene):
    """--depth-map: the passes of harness._passes, one traversal per two frequencies and pass, everything behind the film splat on the GPU (Scene.render_depth_map)"""
    from mitsuba3dopplertof_amd.harness import _passes
    frequencies = [float(x) for x in args.depth_map.split(",")]
    out = args.output or os.path.splitext(args.scene)[0] + "_depth.npy"
    single, n_pass = _passes(args.spp or scene.info()["sample_count"])
    t0 = time.time()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    d = scene.render_depth_map(n_pass, single, frequencies, exposure_time=args.exposure_time, max_path_length=args.max_path_length, film=args.film,
                               outputs=("depth", "wraps", "residual"))
    dt = time.time() - t0
    np.save(out, d["depth"])
    np.save(_sibling(out, "wraps"), d["wraps"])
    np.save(_sibling(out, "residual"), d["residual"])
    if args.verbose:
        print("Depth map finished. (took %.1f ms, %d passes of %d spp, %s)" % (dt * 1e3, n_pass, single, scene.last_stats))
    return 0


def velocity_map(args, scene):
    """--velocity-map: the passes of harness._passes (the sampler's sample count when --spp is 0), one traversal per two offsets and pass, everything behind the film
    splat on the GPU (Scene.render_velocity_map)"""
    from mitsuba3dopplertof_amd.harness import _passes
    offsets = [float(x) for x in args.velocity_map.split(",")]
    out = args.output or os.path.splitext(args.scene)[0] + "_velocity.npy"
    single, n_pass = _passes(args.spp or scene.info()["sample_count"])
    t0 = time.time()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if args.denoise and args.denoise_route == "device":   # one traversal per pass, the films, the denoiser and both maps on the GPU
        noisy, v = scene.render_velocity_map_denoised(n_pass, single, offsets, exposure_time=args.exposure_time, w_g=args.w_g, **args.denoise_kw)
        np.save(_noisy_sibling(out), noisy)
    elif args.denoise:   # the host route: three traversals per pass, the films reach the denoiser through numpy
        from mitsuba3dopplertof_amd.harness import velocity_map_denoised
        noisy, v = velocity_map_denoised(scene, n_pass, single, offsets, exposure_time=args.exposure_time, w_g=args.w_g, **args.denoise_kw)
        np.save(_noisy_sibling(out), noisy)
    else:
        v, _films = scene.render_velocity_map(n_pass, single, offsets, exposure_time=args.exposure_time, w_g=args.w_g, film=args.film)
    dt = time.time() - t0
    np.save(out, v)
    if args.verbose:
        st = scene.last_stats
        print("Velocity map finished. (took %.1f ms, %d passes of %d spp, %s)" % (dt * 1e3, n_pass, single, st))
    return 0


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    check_film_args(ap, args)
    if args.aovs is not None:
        check_aovs_args(ap, args)
    elif args.moments:
        check_moments_args(ap, args)
    elif args.passes != 1:
        ap.error("--variants and --passes belong to --moments")
    elif args.variants is not None and args.adaptive is None and args.depth_map is None:
        check_variant_triples(ap, args)
    if args.depth_map is not None:
        check_depth_map_args(ap, args)
    elif args.max_path_length is not None:
        ap.error("--max-path-length belongs to --depth-map")
    if args.velocity_map is not None:
        check_velocity_map_args(ap, args)
    if args.denoise:
        args.denoise_kw = check_denoise_args(ap, args)
    elif args.denoise_levels is not None or args.denoise_sigma is not None or args.denoise_route != "host":
        ap.error("--denoise-levels, --denoise-sigma and --denoise-route belong to --denoise")
    if args.adaptive is not None:
        check_adaptive_args(ap, args)
    elif args.adaptive_mode != "image" or args.base_passes != 1 or args.max_passes != 4:
        ap.error("--adaptive-mode, --base-passes and --max-passes belong to --adaptive")
    import mitsuba3dopplertof_amd as mi
    from mitsuba3dopplertof_amd.io import write_image
    defines = {}
    for d in args.define:
        if "=" not in d:
            ap.error("-D expects key=value")
        k, v = d.split("=", 1)
        defines[k] = v
    try:
        scene = mi.load_file(args.scene, **defines)
        if args.adaptive is not None:
            return adaptive(args, scene)
        if args.depth_map is not None:
            return depth_map(args, scene)
        if args.velocity_map is not None:
            return velocity_map(args, scene)
        if args.moments:
            return moments(args, scene)
        if args.aovs is not None:
            return aovs(args, scene)
        t0 = time.time()
        offsets = [float(x) for x in args.offsets.split(",")] if args.offsets else None
        triples = parse_variants(args.variants, triples=True) if args.variants else None      # a plain render's --variants (check_variant_triples)
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world > 1:   # launched by torch.distributed.run: shard the rows, one film gather (distributed.py)
            import torch
            import torch.distributed as dist
            from mitsuba3dopplertof_amd import distributed as D
            if offsets is not None:
                ap.error("--offsets is a single-GPU feature")
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            dist.init_process_group("nccl")
            img = (D.render_striped(scene, seed=args.seed, spp=args.spp, stripe_rows=args.stripes) if args.stripes > 0
                   else D.render_sharded(scene, seed=args.seed, spp=args.spp))
            dist.barrier()
            dist.destroy_process_group()
            if img is None:
                return 0
        elif args.denoise:
            render = scene.render_denoised_device if args.denoise_route == "device" else scene.render_denoised
            d = render(seed=args.seed, spp=args.spp, **args.denoise_kw)
            img, noisy = d["denoised"], d["image"]
        else:
            img = scene.render(seed=args.seed, spp=args.spp, offsets=offsets, variants=triples, film=args.film)
        dt = time.time() - t0
    except mi.DtofError as e:
        print("Error: %s" % e, file=sys.stderr)
        return 1
    out = args.output or os.path.splitext(args.scene)[0] + ".exr"
    if args.denoise:
        if out.lower().endswith(".npy"):      # the denoiser's float64 survives in a .npy file only
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            np.save(out, img)
        else:
            write_image(out, img.astype(np.float32))
        write_image(_noisy_sibling(out), noisy)
    elif triples is not None:
        base, ext = os.path.splitext(out)
        for k in range(len(triples)):
            write_image("%s_variant_%d%s" % (base, k, ext), img[k])
    elif offsets is None:
        write_image(out, img)
    else:
        base, ext = os.path.splitext(out)
        for k, off in enumerate(offsets):
            write_image("%s_offset_%.3f%s" % (base, off, ext), img[k])
    if args.verbose:
        st = scene.last_stats
        print("Rendering finished. (took %.1f ms, %.0f Mpaths/s on the GPU: %s)" % (dt * 1e3, st["n_paths"] / max(st["ms_total"], 1e-9) / 1e3, st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
