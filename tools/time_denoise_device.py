#!/usr/bin/env python3
"""The denoised renders: the host route against the device route, and the default route against a build of the parent commit.

    python tools/time_denoise_device.py [--reps 20] [--parent-lib tools/ab/parent.so] [--bench-rounds 4] [--out profiles/denoise_device_ab.txt]

  1. cornell_wall 512 x 512, K = 4, one pass, at 16 spp and at 64 spp, both modes.  The HOST route (Scene.render_denoised, harness.velocity_map_denoised: three
     traversals, numpy between the films and the denoiser) is the yardstick; the DEVICE route (Scene.render_denoised_device, Scene.render_velocity_map_denoised: one
     traversal, everything up to the result on the GPU) is measured against it, never against itself.  One process, a warm-up, then --reps repetitions that alternate
     between the two routes; wall-clock around the calls (the host overhead is what goes), and beside it the library's HIP-event time of the device route's
     traversals (last_stats["ms_total"]) -- what is left of the wall-clock is the tail (inputs, extent, denoiser, map), the copies and the host's part.
     Condition: the device route's median lies below the host route's by more than the sum of the two interquartile ranges.
  2. --parent-lib: `bench.py --gpus 1` (the headline workload, which runs none of the new code) with this tree's library and with the given build of the parent
     commit (DTOF_LIB), --bench-rounds fresh processes each, alternating.

Needs a GPU."""
import argparse
import json
import os
import subprocess
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

W = H = 512
VARIANTS = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]


def stats_of(a):
    q1, med, q3 = np.percentile(np.asarray(a, np.float64), [25, 50, 75])
    return med, q1, q3


def show(a):
    med, q1, q3 = stats_of(a)
    return "median %8.3f ms   quartiles %8.3f .. %8.3f   (n = %d)" % (med, q1, q3, len(a))


def time_routes(reps):
    sc = mi.load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml"), resx=W, resy=H)
    lines, ok = [], True
    for spp in (16, 64):
        pairs = {"IMAGE (4 variants)": (lambda: sc.render_denoised(seed=0, spp=spp, variants=VARIANTS),
                                        lambda: sc.render_denoised_device(seed=0, spp=spp, variants=VARIANTS)),
                 "TOF (velocity map)": (lambda: harness.velocity_map_denoised(sc, 1, spp),
                                        lambda: sc.render_velocity_map_denoised(1, spp))}
        for mode, (host, device) in pairs.items():
            for f in (host, device, host, device):      # warm-up: code objects, workspaces, the buffers of both routes
                f()
            ms = {"host": [], "device": []}
            gpu = []
            for _ in range(reps):
                for name, f in (("host", host), ("device", device)):
                    t0 = time.perf_counter()
                    f()
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                    if name == "device":
                        gpu.append(sc.last_stats["ms_total"])
            (mh, h1, h3), (md, d1, d3) = stats_of(ms["host"]), stats_of(ms["device"])
            met = mh - md > (h3 - h1) + (d3 - d1)
            ok = ok and met
            lines += ["   %s, %d spp, 1 pass" % (mode, spp),
                      "     host route    %s" % show(ms["host"]),
                      "     device route  %s" % show(ms["device"]),
                      "     device route, HIP events around its traversal (one frame: k_generate, k_aov, the bounce loop, three splats): %s" % show(gpu),
                      "     host - device, medians: %.3f ms (%.2fx); sum of the interquartile ranges %.3f ms; condition (difference > that sum): %s"
                      % (mh - md, mh / md, (h3 - h1) + (d3 - d1), "met" if met else "NOT MET"),
                      "     device route above its traversal's GPU time (the tail's kernels, the copies of the results, the host): %.3f ms" % (md - float(np.median(gpu)))]
    return lines, ok


def bench_rounds(parent_lib, rounds, steps, warmup):
    """bench.py in fresh processes, this tree's library and the other build alternating"""
    libs = {"this tree": None, "parent build (%s)" % os.path.relpath(parent_lib, ROOT): os.path.abspath(parent_lib)}
    res = {name: [] for name in libs}
    for _ in range(rounds):
        for name, lib in libs.items():
            env = dict(os.environ)
            env.pop("DTOF_LIB", None)
            if lib:
                env["DTOF_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                               capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                sys.exit("time_denoise_device.py: bench.py failed with %s: %s" % (name, r.stderr[-2000:]))
            out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append((out["value"], out["ms_per_step_median"], out["config"]["image_checksum"]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="a libdtof.so of the parent commit: bench.py is run with it and with this tree's library")
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_device_ab.txt"))
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() == 0:
        sys.exit("time_denoise_device.py: no HIP device -- times are only taken on the GPU")
    lines = ["denoised renders, host route against device route (tools/time_denoise_device.py; one process, %d alternating repetitions after a warm-up; %s)"
             % (args.reps, torch.cuda.get_device_name(0)), "",
             "1. cornell_wall.xml %d x %d, max_depth as loaded, K = 4; wall-clock around the calls, copies to the host included" % (W, H)]
    part, ok = time_routes(args.reps)
    lines += part + ["   condition met in every case: %s" % ok, ""]
    print("\n".join(lines), flush=True)
    if args.parent_lib:
        res = bench_rounds(args.parent_lib, args.bench_rounds, args.bench_steps, 5)
        part = ["2. default route: bench.py --gpus 1 --steps %d --warmup 5, %d fresh processes per build, alternating" % (args.bench_steps, args.bench_rounds)]
        for name, rows in res.items():
            v = np.asarray([r[0] for r in rows])
            part.append("   %-40s Mpaths/s %s   median %.2f, spread %.2f .. %.2f   ms_per_step_median %s   image checksum %s"
                        % (name, " ".join("%.2f" % x for x in v), np.median(v), v.min(), v.max(), " ".join("%.4f" % r[1] for r in rows), sorted({r[2] for r in rows})))
        x, y = list(res)
        mine, parent = np.asarray([r[0] for r in res[x]]), np.asarray([r[0] for r in res[y]])
        part.append("   this tree / parent, medians: %.4fx; this tree's median inside the parent's own spread: %s"
                    % (np.median(mine) / np.median(parent), bool(parent.min() <= np.median(mine) <= parent.max())))
        part.append("")
        print("\n".join(part), flush=True)
        lines += part
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("written to", args.out)


if __name__ == "__main__":
    main()
