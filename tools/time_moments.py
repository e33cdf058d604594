#!/usr/bin/env python3
"""The moment film against the float64 film, timed side by side.

    python tools/time_moments.py [--reps 10] [--out profiles/moments_ab.txt]

  cornell_wall 512 x 512 x 64 spp, K = 1 (the integrator's own pair) and K = 4 variants of one traversal: frame time and splat stage time of
  Scene.render_film64 (k_splat_f64: 1 + 3 K sums per cell) and of Scene.render_moments (k_splat_moments_f64: 1 + 6 K + K (K - 1) / 2 sums per cell)

The two routes run in one process, alternating frame by frame, in three rounds of --reps frames after a warm-up of each; a round's figure is the median of its
frames, the reported figure the median of the three rounds (their extremes beside it).  Times are the library's HIP events around the frame (generate .. splat) and
around the splat stage; the develop kernels and the copies to the host lie outside both.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
import make_scenes  # noqa: E402

make_scenes.ensure()
import mitsuba3dopplertof_amd as mi  # noqa: E402

ROUNDS = 3
K4 = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]


def three(rounds):
    a = np.sort(np.asarray(rounds))
    return "%8.3f ms (rounds %.3f .. %.3f)" % (np.median(a), a[0], a[-1])


def time_routes(sc, spp, variants, reps):
    routes = {"float64 film (k_splat_f64)": lambda: sc.render_film64(0, spp, variants=variants),
              "moment film (k_splat_moments_f64)": lambda: sc.render_moments(0, spp, variants=variants, raw=True)}
    for call in routes.values():      # warm-up: code objects, workspace, both films
        for _ in range(3):
            call()
    out = {name: ([], []) for name in routes}
    for _ in range(ROUNDS):
        ms = {name: ([], []) for name in routes}
        for _ in range(reps):
            for name, call in routes.items():
                call()
                assert sc.last_stats["n_fused_splat_launches"] == 0
                ms[name][0].append(sc.last_stats["ms_total"]); ms[name][1].append(sc.last_stats["ms_splat"])
        for name in routes:
            out[name][0].append(float(np.median(ms[name][0]))); out[name][1].append(float(np.median(ms[name][1])))
    return out


def report(K, res):
    sums = {"float64 film (k_splat_f64)": 1 + 3 * K, "moment film (k_splat_moments_f64)": mi.MOMENT_PLANES(K)}
    lines = ["K = %d: cornell_wall.xml 512 x 512, 64 spp" % K]
    for name, (frames, splats) in res.items():
        lines.append("  %-36s frame %s   splat stage %s   sums (atomics of a run) per cell %d" % (name, three(frames), three(splats), sums[name]))
    a, b = list(res)
    lines.append("  moment / float64 (medians): splat stage %.2fx, frame %.3fx; sums per cell %.2fx"
                 % (np.median(res[b][1]) / np.median(res[a][1]), np.median(res[b][0]) / np.median(res[a][0]), sums[b] / sums[a]))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moments_ab.txt"))
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() == 0:
        sys.exit("time_moments.py: no HIP device -- times are only taken on the GPU")
    lines = ["moment film against float64 film (tools/time_moments.py; %d rounds of %d alternating frames per route after a warm-up; %s)" % (ROUNDS, args.reps, torch.cuda.get_device_name(0)),
             "frame = the library's HIP events around generate .. splat; a round's figure is the median of its frames, the figure given the median of the rounds", ""]
    sc = mi.load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml"), resx=512, resy=512)
    for K, variants in ((1, None), (4, K4)):
        part = report(K, time_routes(sc, 64, variants, args.reps)) + [""]
        print("\n".join(part), flush=True)
        lines += part
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("written to", args.out)


if __name__ == "__main__":
    main()
