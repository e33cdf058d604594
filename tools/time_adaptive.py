#!/usr/bin/env python3
"""What adaptive sampling costs and buys, measured on the GPU: writes profiles/adaptive_ab.txt.  Interleaved rounds, medians, the spread beside every figure.

  (a) the headline bench.py line of this build against the parent commit's library (--parent-lib: a libdtof.so built from the parent with the same compiler), alternating,
      each in its own process; the margin is the parent's own round-to-round spread in this session
  (b) a sparse pass with the FULL list against the dense pass of the same frame through the generic kernels (DTOF_PLAN_FACTS=0): the price of the table lookup; and
      sparse passes at 50 %, 10 % and 1 % list density, scattered pixels and one compact block (wave coherence differs)
  (c) the selection's launches and the 4-byte read-back per pass (mi.adaptive_select round trips are NOT that: the driver's per-pass cost is timed through
      Scene.render_adaptive with max_passes against base_passes at a tolerance nothing reaches), per frame size
  (d) end to end on the moving-wall velocity map: wall-clock time and paths the adaptive loop needs to bring the map's standard error under a tolerance on 95 % of its
      valid pixels (the first pass budget at which its estimate says so), against the uniform passes needed for the same; the tolerance is the 95th percentile of a
      UNIFORM run's own standard error at a stated budget; then both are held to an estimate the selection cannot bias: the spread of the map over repetitions

    python tools/time_adaptive.py [--parent-lib PATH] [--parts abcd] [--rounds 5] [--out profiles/adaptive_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "scenes")
K4 = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]


def med(v):
    v = np.asarray(v, float)
    return "%.3f (min %.3f, max %.3f, n %d)" % (np.median(v), v.min(), v.max(), len(v))


def part_a(args, out):
    libs = {"this": os.path.join(ROOT, "mitsuba3dopplertof_amd", "libdtof.so")}
    if args.parent_lib:
        libs["parent"] = args.parent_lib
    res = {k: [] for k in libs}
    for _ in range(args.rounds):
        for name, lib in libs.items():
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "300", "--warmup", "20"], capture_output=True, text=True,
                               env=dict(os.environ, DTOF_LIB=lib), timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                raise SystemExit("bench.py failed with %s: %s" % (name, r.stderr[-500:]))
            res[name].append(json.loads(line[-1])["value"])
    out.append("(a) headline bench.py --gpus 1 --steps 300 --warmup 20, Mpaths/s, %d interleaved rounds" % args.rounds)
    for name, v in res.items():
        out.append("    %-7s median %s  rounds %s" % (name, med(v), " ".join("%.1f" % x for x in v)))
    if "parent" in res:
        spread = (max(res["parent"]) - min(res["parent"])) / np.median(res["parent"])
        diff = np.median(res["this"]) / np.median(res["parent"]) - 1
        out.append("    this / parent - 1 = %+.2f %%; the parent's own spread (max - min) / median = %.2f %%" % (100 * diff, 100 * spread))


def _time_calls(fn, rounds, reps):
    fn()
    t = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        t.append((time.perf_counter() - t0) / reps * 1e3)
    return t


def part_b(args, out, mi):
    frames = [("cornell_wall 512x512x64", "cornell_wall.xml", dict(resx=512, resy=512), 64), ("domino 1024x1024x128 K=1", "domino.xml", dict(resx=1024, resy=1024), 128)]
    for title, scene, params, spp in frames:
        sc = mi.load_file(os.path.join(SCENES, scene), **params)
        w, h = sc.size
        n = w * h
        rng = np.random.default_rng(1)
        lists = {"full": np.arange(n)}
        for frac in (0.5, 0.1, 0.01):
            m = int(n * frac)
            lists["%g %% scattered" % (100 * frac)] = np.sort(rng.permutation(n)[:m])
            side = int(np.sqrt(m))
            ys, xs = np.mgrid[0:side, 0:side]
            lists["%g %% block" % (100 * frac)] = np.sort(((ys + (h - side) // 2) * w + xs + (w - side) // 2).reshape(-1))
        variants = None

        def dense_generic():
            os.environ["DTOF_PLAN_FACTS"] = "0"
            try:
                sc.render_moments(0, spp, variants=variants, raw=True)
            finally:
                del os.environ["DTOF_PLAN_FACTS"]
            return sc.last_stats["ms_total"]

        def dense_default():
            sc.render_moments(0, spp, variants=variants, raw=True)
            return sc.last_stats["ms_total"]

        rows = {"dense, default kernels": [], "dense, generic kernels": []}
        rows.update({"list " + k: [] for k in lists})
        for f in (dense_default, dense_generic):
            f()
        for k, v in lists.items():
            sc.render_pixels(v, 0, spp, raw=True)
        for _ in range(args.rounds):
            rows["dense, default kernels"].append(dense_default())
            rows["dense, generic kernels"].append(dense_generic())
            for k, v in lists.items():
                sc.render_pixels(v, 0, spp, raw=True)
                rows["list " + k].append(sc.last_stats["ms_total"])
        out.append("(b) %s: one pass into the moment film, ms of the frame's own HIP events (upload of the list and read-back of the planes not included), %d interleaved rounds"
                   % (title, args.rounds))
        for k, v in rows.items():
            out.append("    %-24s median %s" % (k, med(v)))
        out.append("    full list / dense generic = %.3f" % (np.median(rows["list full"]) / np.median(rows["dense, generic kernels"])))


def part_c(args, out, mi):
    out.append("(c) the selection per pass: Scene.render_adaptive with 1 base pass and max_passes 1 against max_passes 2 at a tolerance nothing reaches (the second pass is the "
               "selection's launches, the 4-byte read-back and an empty list); wall clock, ms, %d interleaved rounds" % args.rounds)
    for res in (256, 512, 1024, 2048):
        sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=res, resy=res)
        one = lambda: sc.render_adaptive(seed=0, spp=4, base_passes=1, max_passes=1, mode="image", tol=1e30)
        two = lambda: sc.render_adaptive(seed=0, spp=4, base_passes=1, max_passes=2, mode="image", tol=1e30)
        a, b = [], []
        one(); two()
        for _ in range(args.rounds):
            a += _time_calls(one, 1, 3)
            b += _time_calls(two, 1, 3)
        out.append("    %4d x %-4d without %s   with %s   difference of the medians %.3f ms" % (res, res, med(a), med(b), np.median(b) - np.median(a)))


def part_d(args, out, mi):
    from mitsuba3dopplertof_amd import harness
    spp, budget, res, reps = 64, 8, 256, 16
    sc = mi.load_file(os.path.join(SCENES, "cornell_wall.xml"), resx=res, resy=res)
    pairs, offsets = [(0, 2), (1, 3)], (0.0, 0.25)

    def uniform(passes):
        t0 = time.perf_counter()
        m = sc.render_moments(0, spp, n_passes=passes, variants=K4)
        se = np.fmax(harness.velocity_standard_error(m, 0, 2, passes * spp), harness.velocity_standard_error(m, 1, 3, passes * spp))
        return se, (time.perf_counter() - t0) * 1e3, sc.last_stats["n_paths"]

    def adaptive(max_passes, seed=0):
        t0 = time.perf_counter()
        r = sc.render_adaptive(seed=seed, spp=spp, base_passes=1, max_passes=max_passes, variants=K4, mode="velocity", tol=tol, pairs=pairs)
        return r, (time.perf_counter() - t0) * 1e3, sc.last_stats["n_paths"]

    def uniform_map(passes, seed):
        acc = None
        for p in range(passes):
            img = sc.render(seed=seed + p, spp=spp, variants=K4, film="float64").astype(np.float64)
            acc = img if acc is None else acc + img
        tof = [harness.to_tof_image(im, 0.0015) for im in acc / passes]
        return harness.calc_velocity_from_homo_heteros(tof[:2], tof[2:], 0.0015, 30)

    se_u, _, _ = uniform(budget)
    valid = np.isfinite(se_u)
    tol = float(np.percentile(se_u[valid], 95))
    out.append("(d) moving-wall velocity map, cornell_wall %d x %d, passes of %d spp, pairs %s.  Tolerance %.4g m/s = the 95th percentile of the standard error of a UNIFORM "
               "run of %d passes (%d valid pixels of %d)" % (res, res, spp, pairs, tol, budget, valid.sum(), valid.size))
    need = None
    for passes in range(1, 4 * budget + 1):
        se, ms, paths = uniform(passes)
        share = np.mean(se[valid] <= tol)
        if share >= 0.95:
            need = (passes, paths, share)
            break
    reach = None
    for most in range(1, 4 * budget + 1):      # the first pass budget at which the loop's own estimate has 95 % of the pixels under the tolerance
        r, ms, paths = adaptive(most)
        share = np.mean(r["metric"][valid] <= tol)
        if share >= 0.95:
            reach = (most, paths, share, list(r["pass_pixels"]))
            break
    t_u, t_a = [], []
    for _ in range(args.rounds):
        t_u.append(uniform(need[0])[1])
        t_a.append(adaptive(reach[0])[1])
    out.append("    uniform : %d passes reach %.1f %% of the valid pixels under the tolerance (moment estimate); %d paths; wall clock ms median %s" % (need[0], 100 * need[2], need[1], med(t_u)))
    out.append("    adaptive: stopped at the first budget, %d passes (%s pixels), at which its own estimate has %.1f %% of those pixels under the tolerance; %d paths; wall "
               "clock ms median %s" % (reach[0], " ".join(str(x) for x in reach[3]), 100 * reach[2], reach[1], med(t_a)))
    out.append("    paths adaptive / uniform = %.3f, time adaptive / uniform = %.3f (interleaved rounds)" % (reach[1] / need[1], np.median(t_a) / np.median(t_u)))
    # an estimate independent of the selection: the spread of the MAP itself over repetitions with other seeds, the same for both
    maps_u = np.stack([uniform_map(need[0], 1000 * (i + 1)) for i in range(reps)])
    maps_a = np.stack([harness.velocity_map_adaptive(sc, spp, reach[0], tol, offsets, base_passes=1, seed=1000 * (i + 1))[0] for i in range(reps)])
    sd_u, sd_a = maps_u.std(axis=0, ddof=1), maps_a.std(axis=0, ddof=1)
    out.append("    independent check, %d repetitions of each with other seeds: pixels whose map's empirical standard deviation is under the tolerance: uniform %.1f %%, "
               "adaptive %.1f %%; median deviation uniform %.4g, adaptive %.4g m/s; |mean adaptive map - mean uniform map|, median over the pixels, %.4g m/s (the standard "
               "error of that difference is about %.4g)" % (reps, 100 * np.mean(sd_u[valid] <= tol), 100 * np.mean(sd_a[valid] <= tol), np.median(sd_u), np.median(sd_a),
                                                       np.median(np.abs(maps_a.mean(axis=0) - maps_u.mean(axis=0))), np.median(np.sqrt((sd_u ** 2 + sd_a ** 2) / reps))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_ab.txt"))
    args = ap.parse_args()
    import mitsuba3dopplertof_amd as mi
    out = ["adaptive sampling: measurements of tools/time_adaptive.py (%s)" % mi._lib().dtof_version().decode()]
    for part, fn in (("a", lambda: part_a(args, out)), ("b", lambda: part_b(args, out, mi)), ("c", lambda: part_c(args, out, mi)), ("d", lambda: part_d(args, out, mi))):
        if part in args.parts:
            fn()
            print("\n".join(out[-12:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
