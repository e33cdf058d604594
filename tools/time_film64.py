#!/usr/bin/env python3
"""The float64 film against the float32 film, timed side by side and held against the oracle's exact film.

    python tools/time_film64.py [--reps 10] [--out profiles/film64_ab.txt] [--parent-lib PATH/libdtof.so]

  C2        cornell_wall 512 x 512 x 64 spp: frame time and splat stage time of the float32 default (the first-bounce kernel splats), of float32 with DTOF_FUSE_SPLAT=0
            (the separate float32 splat kernel: the like-for-like partner) and of the float64 film
  C5-like   domino.xml 512 x 512 x 64 spp, trapezoidal, K = 4 films of one traversal: float32 against float64
  accuracy  rel_linf_px (tests/test_gpu_parity.py) of both routes against orc_render_exact on cornell_sphere_light 64 x 64 x 64 spp
  headline  with --parent-lib: `python bench.py --gpus 1` of this tree against the same bench.py on the parent commit's library (DTOF_LIB), alternating

All routes of a shape run in one process, alternating frame by frame, in three rounds of --reps frames after a warm-up of each; a round's figure is the median of its
frames, the reported figure the median of the three rounds (their extremes beside it).  Times are the library's HIP events around the frame (generate .. splat) and
around the splat stage.  Needs a GPU."""
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

ROUNDS = 3
K4 = [(1.0, 0.0), (1.0, 0.25), (1.0, 0.5), (1.0, 0.75)]


def rel_linf_px(a, ref, eps=1e-3):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    floor = eps * max(np.abs(ref).max(), 1e-30)
    return float((np.abs(a - ref) / np.maximum(np.abs(ref), floor)).max())


def three(rounds):
    a = np.sort(np.asarray(rounds))
    return "%8.3f ms (rounds %.3f .. %.3f)" % (np.median(a), a[0], a[-1])


def time_routes(sc, routes, spp, variants, reps):
    """routes: name -> (environment, film); -> name -> ([frame ms of the rounds], [splat ms of the rounds], fused splat launches per frame)"""
    def frame(env, film):
        for k, v in env.items():
            os.environ[k] = v
        try:
            sc.render(seed=0, spp=spp, variants=variants, film=film)
        finally:
            for k in env:
                del os.environ[k]
        return sc.last_stats
    for env, film in routes.values():      # warm-up: code objects, workspace, both films
        for _ in range(3):
            frame(env, film)
    out = {name: ([], [], 0) for name in routes}
    for _ in range(ROUNDS):
        ms = {name: ([], []) for name in routes}
        for _ in range(reps):
            for name, (env, film) in routes.items():
                st = frame(env, film)
                ms[name][0].append(st["ms_total"]); ms[name][1].append(st["ms_splat"])
                out[name] = (out[name][0], out[name][1], st["n_fused_splat_launches"])
        for name in routes:
            out[name][0].append(float(np.median(ms[name][0]))); out[name][1].append(float(np.median(ms[name][1])))
    return out


def report(title, res, pair):
    lines = [title]
    for name, (frames, splats, fused) in res.items():
        lines.append("  %-44s frame %s   splat stage %s   fused splat launches %d" % (name, three(frames), three(splats), fused))
    a, b = pair
    lines.append("  float64 / float32 separate splat (like for like, medians): splat stage %.2fx, frame %.3fx (+%.1f %%)"
                 % (np.median(res[b][1]) / np.median(res[a][1]), np.median(res[b][0]) / np.median(res[a][0]), 100 * (np.median(res[b][0]) / np.median(res[a][0]) - 1)))
    return lines


def accuracy():
    """the exact image comes from tests/film64_exact.py in a process of its own: the oracle is test infrastructure and is not imported outside tests/"""
    import tempfile
    path, spp, seed = os.path.join(ROOT, "scenes", "cornell_sphere_light.xml"), 64, 3
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "exact.npy")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "film64_exact.py"), path, "64", "64", str(spp), str(seed), out])
        exact = np.load(out)
    sc = mi.load_file(path, resx=64, resy=64)
    f32, f64 = sc.render(seed=seed, spp=spp), sc.render(seed=seed, spp=spp, film="float64")
    diff = int((f64.view(np.uint32) != exact.view(np.uint32)).sum())
    return ["accuracy: cornell_sphere_light 64 x 64 x 64 spp, seed 3, rel_linf_px against orc_render_exact",
            "  float32 film %.3g   float64 film %.3g (%d of %d floats differ from the exact image; one float32 ulp is %.3g)" % (rel_linf_px(f32, exact), rel_linf_px(f64, exact), diff, f64.size, 2.0 ** -23)]


def headline(parent_lib, rounds=ROUNDS):
    """bench.py --gpus 1 (its default steps and warm-up) on this tree's library and on the parent's, alternating"""
    ms = {"parent": [], "this commit": []}
    for _ in range(rounds):
        for name, lib in (("parent", parent_lib), ("this commit", None)):
            env = dict(os.environ)
            env.pop("DTOF_LIB", None)
            if lib:
                env["DTOF_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit("bench.py failed (%s): %s" % (name, r.stderr[-2000:]))
            ms[name].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["ms_per_step"])
    lines = ["headline: python bench.py --gpus 1 (C2, default steps), ms per step of %d alternating runs each" % rounds]
    for name, v in ms.items():
        lines.append("  %-12s %s   median %.4f   spread %.4f" % (name, "  ".join("%.4f" % x for x in v), np.median(v), max(v) - min(v)))
    d = np.median(ms["this commit"]) - np.median(ms["parent"])
    lines.append("  difference of the medians %+.4f ms: %s the parent's own run-to-run spread" % (d, "within" if abs(d) <= max(ms["parent"]) - min(ms["parent"]) else "OUTSIDE"))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "film64_ab.txt"))
    ap.add_argument("--parent-lib", default=None, help="libdtof.so of the parent commit: also run the C2 headline of bench.py on both")
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() == 0:
        sys.exit("time_film64.py: no HIP device -- times are only taken on the GPU")
    lines = ["float64 film against float32 film (tools/time_film64.py; %d rounds of %d alternating frames per route after a warm-up; %s)" % (ROUNDS, args.reps, torch.cuda.get_device_name(0)),
             "frame = the library's HIP events around generate .. splat; a round's figure is the median of its frames, the figure given the median of the rounds", ""]
    sc = mi.load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml"), resx=512, resy=512)
    routes = {"float32, default (k_shade splats)": ({}, "float32"), "float32, DTOF_FUSE_SPLAT=0 (separate splat)": ({"DTOF_FUSE_SPLAT": "0"}, "float32"),
              "float64 (k_splat_f64)": ({}, "float64")}
    res = time_routes(sc, routes, 64, None, args.reps)
    lines += report("C2: cornell_wall.xml 512 x 512, 64 spp, one film", res, ("float32, DTOF_FUSE_SPLAT=0 (separate splat)", "float64 (k_splat_f64)"))
    d = np.median(res["float64 (k_splat_f64)"][0]) / np.median(res["float32, default (k_shade splats)"][0])
    lines += ["  float64 / float32 default (what a user who turns it on pays): frame %.3fx (+%.1f %%)" % (d, 100 * (d - 1)), ""]
    print("\n".join(lines), flush=True)
    sc = mi.load_file(os.path.join(ROOT, "scenes", "domino.xml"), resx=512, resy=512, wave_function_type="trapezoidal")
    routes = {"float32 (separate splat)": ({}, "float32"), "float64 (k_splat_f64)": ({}, "float64")}
    part = report("C5-like: domino.xml 512 x 512, 64 spp, trapezoidal, K = 4 films of one traversal", time_routes(sc, routes, 64, K4, max(args.reps // 2, 3)), tuple(routes)) + [""]
    part += accuracy() + [""]
    print("\n".join(part), flush=True)
    lines += part
    if args.parent_lib:
        part = headline(os.path.abspath(args.parent_lib))
        print("\n".join(part), flush=True)
        lines += part + [""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("written to", args.out)


if __name__ == "__main__":
    main()
