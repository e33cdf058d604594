#!/usr/bin/env python3
"""The velocity map by its two routes, timed side by side: harness.run_scene_velocity_map (films developed on the device, copied to the host, averaged and
reconstructed by numpy) and harness.run_scene_velocity_map_device (developed, averaged and reconstructed by two kernels; only the results are copied).

    python tools/time_velocity_map.py [--reps 20] [--out profiles/velocity_map_device.txt] [--shapes c2,domino]

Both routes run in one process, alternating, after a warm-up of each; every repetition is a host clock around work that ends in a device synchronise (the host
route ends with its numpy arithmetic).  Reported: median, quartiles and extremes of each route, the frame's GPU time from the library's events, the host route's
renders alone (what is left of it is its tail: copies and numpy), and the GPU time of the two reconstruction kernels from HIP events around each.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
import make_scenes  # noqa: E402

make_scenes.ensure()
import mitsuba3dopplertof_amd as mi  # noqa: E402
from mitsuba3dopplertof_amd import harness  # noqa: E402

# name: (scene file, -D parameters, total spp): one pass each (total <= 1024), two offsets = the four films of one traversal
SHAPES = {"c2": ("cornell_wall.xml", dict(resx=512, resy=512), 64),
          "domino": ("domino.xml", dict(resx=1024, resy=1024), 128)}
OFFSETS = (0.0, 0.25)


def spread(ms):
    a = np.sort(np.asarray(ms))
    return "median %8.3f ms   quartiles %8.3f .. %8.3f   min %8.3f   max %8.3f   (n = %d)" % (np.median(a), np.percentile(a, 25), np.percentile(a, 75), a[0], a[-1], len(a))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_times(sc, reps):
    """GPU milliseconds of the develop-accumulate (k_develop<float, false> of dtof_develop.hip: the four films of one pass, stored as on a first pass) and k_velocity_map (two pairs, ToF images and per-pair maps written), HIP events on the
    stream the library enqueues on"""
    import torch
    w, h = sc.size
    n = w * h
    stream = torch.cuda.Stream()
    sc.set_stream(stream.cuda_stream)
    t_acc, t_map = [], []
    try:
        with torch.cuda.stream(stream):
            film = torch.zeros((4, n, 4), dtype=torch.float32, device="cuda")
            d_sum = torch.zeros((4, n, 3), dtype=torch.float32, device="cuda")
            d_tof = torch.zeros((4, n), dtype=torch.float32, device="cuda")
            d_pairs = torch.zeros((2, n), dtype=torch.float64, device="cuda")
            d_v = torch.zeros((n,), dtype=torch.float64, device="cuda")
            variants = [(0.0, o) for o in OFFSETS] + [(1.0, o) for o in OFFSETS]
            sc.render_rows_async(film.data_ptr(), 0, 16, 0, h, variants=variants)      # a real film, so that the divisions see real operands
            for i in range(reps + 3):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record(stream)
                sc.develop_accumulate_async(film.data_ptr(), 4, d_sum.data_ptr(), n, first=True)
                e[1].record(stream)
                e[2].record(stream)
                sc.velocity_map_async(d_sum.data_ptr(), (0, 1), (2, 3), 1, n, d_v.data_ptr(), d_tof_ptr=d_tof.data_ptr(), d_velocity_pairs_ptr=d_pairs.data_ptr())
                e[3].record(stream)
                stream.synchronize()
                if i >= 3:
                    t_acc.append(e[0].elapsed_time(e[1])); t_map.append(e[2].elapsed_time(e[3]))
        sc.collect()
    finally:
        torch.cuda.synchronize()
        sc.set_stream(None)
    return t_acc, t_map


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "velocity_map_device.txt"))
    ap.add_argument("--shapes", default="c2,domino")
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() == 0:
        sys.exit("time_velocity_map.py: no HIP device -- times are only taken on the GPU")
    lines = ["velocity map, host route vs device route (tools/time_velocity_map.py, %d alternating repetitions after a warm-up of each; %s)" % (args.reps, torch.cuda.get_device_name(0)),
             "host clock around each call, which ends in a device synchronise; GPU times from HIP events", ""]
    for name in args.shapes.split(","):
        xml, params, spp = SHAPES[name]
        sc = mi.load_file(os.path.join(ROOT, "scenes", xml), **params)
        w, h = sc.size
        variants = [(0.0, o) for o in OFFSETS] + [(1.0, o) for o in OFFSETS]
        host = lambda: harness.run_scene_velocity_map(sc, total_spp=spp, offsets=OFFSETS)              # noqa: E731
        device = lambda: harness.run_scene_velocity_map_device(sc, total_spp=spp, offsets=OFFSETS)     # noqa: E731
        renders = lambda: harness.run_scene_doppler_tof_variants(sc, variants, spp)                    # noqa: E731
        for _ in range(3):
            v_host, _ = host()
            v_dev, films = device()
            renders()
        with np.errstate(all="ignore"):
            own = harness.calc_velocity_from_homo_heteros(films["homodyne"], films["heterodyne"])
        same = bool(np.array_equal(v_dev.view(np.uint64)[~np.isnan(own)], own.view(np.uint64)[~np.isnan(own)]) and np.isnan(v_dev[np.isnan(own)]).all())
        t_host, t_dev, t_renders, gpu_host, gpu_dev = [], [], [], [], []
        for _ in range(args.reps):
            t, _ = clock(host); t_host.append(t); gpu_host.append(sc.pass_stats[-1]["ms_total"])
            t, _ = clock(device); t_dev.append(t); gpu_dev.append(sc.last_stats["ms_total"])
            t, _ = clock(renders); t_renders.append(t)
        t_acc, t_map = kernel_times(sc, args.reps)
        film_mb = 4 * w * h * 3 * 4 / 1e6
        lines += ["%s: %s %d x %d, %d spp, 1 pass, offsets %s (4 films of one traversal; the host route copies %.1f MB of developed films)" % (name, xml, w, h, spp, OFFSETS, film_mb),
                  "  host route   run_scene_velocity_map          %s" % spread(t_host),
                  "  device route run_scene_velocity_map_device   %s" % spread(t_dev),
                  "  host route's renders alone (run_scene_doppler_tof_variants: traversal, develop, copy, float32 mean)",
                  "                                               %s" % spread(t_renders),
                  "  host tail beyond its renders (ToF images + calc_velocity_from_homo_heteros in numpy): median %.3f ms" % (np.median(t_host) - np.median(t_renders)),
                  "  GPU time of the traversal (library events)   host route median %.3f ms, device route median %.3f ms" % (np.median(gpu_host), np.median(gpu_dev)),
                  "  develop-accumulate (4 films)                 %s" % spread(t_acc),
                  "  k_velocity_map (2 pairs, all outputs)        %s" % spread(t_map),
                  "  device route / host route (medians): %.3f; device map bit-equal to numpy on its own ToF images: %s" % (np.median(t_dev) / np.median(t_host), same), ""]
        print("\n".join(lines[-11:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("written to", args.out)


if __name__ == "__main__":
    main()
