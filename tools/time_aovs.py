#!/usr/bin/env python3
"""The aov film against the moment film, timed side by side, and the default route against another build of the library.

    python tools/time_aovs.py [--reps 20] [--parent-lib tools/ab/parent.so] [--bench-rounds 4] [--out profiles/aov_ab.txt]

  1. cornell_wall 512 x 512 x 64 spp: Scene.render_aovs("p:position,n:sh_normal") -- k_generate, then k_aov: one closest hit per lane and the splat of 6 channels
     and the weight -- against Scene.render_moments at K = 1 -- the whole path, then k_splat_moments_f64: 6 moments and the weight.  Both issue the same number of
     atomics per cell (7), through the same run reduction, into the same 32-double cells.  The yardstick is the moment film, which is the older of the two.
     One process, a warm-up of each route, then --reps repetitions that alternate between the routes; median and quartiles of the library's HIP events around the
     frame (generate .. splat), and of the stages the two routes differ in.
  2. --parent-lib: `bench.py --gpus 1` (the headline workload, which runs no aov code) with this tree's library and with the given build of another commit
     (DTOF_LIB), --bench-rounds processes each, alternating; the headline value and the median frame time of every process.

Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
import make_scenes  # noqa: E402

make_scenes.ensure()
import mitsuba3dopplertof_amd as mi  # noqa: E402

SPEC = "p:position,n:sh_normal"


def quartiles(a):
    q1, med, q3 = np.percentile(np.asarray(a, np.float64), [25, 50, 75])
    return "median %8.3f ms   quartiles %8.3f .. %8.3f   (n = %d)" % (med, q1, q3, len(a))


def time_routes(sc, spp, reps):
    routes = {"moment film, K = 1 (path + k_splat_moments_f64)": lambda: sc.render_moments(0, spp, raw=True),
              "aov film, 6 channels (k_aov)": lambda: sc.render_aovs(SPEC, 0, spp, raw=True)}
    for call in routes.values():      # warm-up: code objects, workspace, the film
        for _ in range(3):
            call()
    keys = ("ms_total", "ms_generate", "ms_trace", "ms_shade", "ms_splat")
    ms = {name: {k: [] for k in keys} for name in routes}
    for _ in range(reps):
        for name, call in routes.items():
            call()
            assert sc.last_stats["n_fused_splat_launches"] == 0
            for k in keys:
                ms[name][k].append(sc.last_stats[k])
    return ms


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
                sys.exit("time_aovs.py: bench.py failed with %s: %s" % (name, r.stderr[-2000:]))
            out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append((out["value"], out["ms_per_step_median"], out["config"]["image_checksum"]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="a libdtof.so of another commit: bench.py is run with it and with this tree's library")
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_ab.txt"))
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() == 0:
        sys.exit("time_aovs.py: no HIP device -- times are only taken on the GPU")
    lines = ["aov film against moment film (tools/time_aovs.py; one process, %d alternating repetitions per route after a warm-up; %s)" % (args.reps, torch.cuda.get_device_name(0)),
             "times are the library's HIP events: frame = generate .. splat; the develop kernel and the copy to the host lie outside", "",
             "cornell_wall.xml 512 x 512, 64 spp; both routes add 7 sums per cell of their footprints"]
    sc = mi.load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml"), resx=512, resy=512)
    ms = time_routes(sc, 64, args.reps)
    for name, m in ms.items():
        lines.append("  %s" % name)
        lines.append("    frame                 %s" % quartiles(m["ms_total"]))
        lines.append("    generate              %s" % quartiles(m["ms_generate"]))
        lines.append("    trace (aov: k_aov)    %s" % quartiles(m["ms_trace"]))
        lines.append("    shade                 %s" % quartiles(m["ms_shade"]))
        lines.append("    splat                 %s" % quartiles(m["ms_splat"]))
    a, b = list(ms)
    lines.append("  aov / moment, medians of the frame: %.3fx" % (np.median(ms[b]["ms_total"]) / np.median(ms[a]["ms_total"])))
    lines.append("  k_aov / k_splat_moments_f64, medians (the closest hit and the splat of 7 sums against the splat of 7 sums alone): %.3fx"
                 % (np.median(ms[b]["ms_trace"]) / np.median(ms[a]["ms_splat"])))
    lines.append("")
    print("\n".join(lines), flush=True)
    if args.parent_lib:
        res = bench_rounds(args.parent_lib, args.bench_rounds, args.bench_steps, 5)
        part = ["default route: bench.py --gpus 1 --steps %d --warmup 5, %d fresh processes per build, alternating" % (args.bench_steps, args.bench_rounds)]
        for name, rows in res.items():
            v = np.asarray([r[0] for r in rows])
            part.append("  %-40s Mpaths/s %s   median %.2f, spread %.2f .. %.2f   ms_per_step_median %s   image checksum %s"
                        % (name, " ".join("%.2f" % x for x in v), np.median(v), v.min(), v.max(), " ".join("%.4f" % r[1] for r in rows), sorted({r[2] for r in rows})))
        x, y = list(res)
        part.append("  this tree / parent, medians: %.4fx" % (np.median([r[0] for r in res[x]]) / np.median([r[0] for r in res[y]])))
        part.append("")
        print("\n".join(part), flush=True)
        lines += part
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("written to", args.out)


if __name__ == "__main__":
    main()
