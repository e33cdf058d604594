#!/usr/bin/env python3
"""The denoiser's level kernels, tiled against one lane per pixel, and what the denoise stage adds to the calls that end in it.

    make -C mitsuba3dopplertof_amd/csrc variant NAME=denoise_naive DEFS=-DDTOF_DENOISE_NAIVE      # tools/ab/denoise_naive.so: the one-lane-per-pixel build
    python tools/time_denoise.py [--reps 20] [--naive-lib tools/ab/denoise_naive.so] [--parent-lib tools/ab/parent.so] [--bench-rounds 4]
                                 [--out profiles/denoise_ab.txt] [--wall-out profiles/denoise_wall.txt]

  1. 512 x 512, K = 4, normals, positions and variances, on the device through dtof_denoise_async: the whole call (the pack kernel and L level kernels) for
     L = 1 .. 6, with the LDS-tiled level kernel of this tree's library and, with --naive-lib, with the one-lane-per-pixel form of a build with
     -DDTOF_DENOISE_NAIVE (the same arithmetic: the two results are compared bit for bit first).  One process that holds both libraries, a warm-up, then --reps
     repetitions that alternate between the two forms and walk through the L; medians and quartiles of HIP events around the call.  The increment from L - 1 to L is the cost
     of the level of step 2^(L - 1); next to it the level's compulsory bytes -- every input and output word once -- and the bandwidth that would be.
  2. cornell_wall 512 x 512: Scene.render_denoised against the three renders it starts with, and harness.run_scene_velocity_map_denoised against the same calls
     without the denoiser; wall-clock around the calls, which all end in a copy to the host.
  3. the moving wall of cornell_wall.xml (-10 m/s): harness.run_scene_velocity_map_denoised at 64 x 64 and 256 x 256, 512 and 16 spp, with the default
     sigma_position (1 % of the extent) and with ten times that; RMS error, mean error and standard deviation of the noisy and of the denoised map over the pixels
     whose aov shape_index is the wall's -> --wall-out.
  4. --parent-lib: `bench.py --gpus 1` (the headline workload, which runs no denoiser code) with this tree's library and with the given build of another commit
     (DTOF_LIB), --bench-rounds processes each, alternating.

Needs a GPU."""
import argparse
import ctypes as C
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
K = 4
TILED, NAIVE = "tiled (LDS tile on the level's lattice)", "naive (one lane per pixel, every tap from memory)"
VARIANTS = [(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]


def quartiles(a):
    q1, med, q3 = np.percentile(np.asarray(a, np.float64), [25, 50, 75])
    return "median %8.3f ms   quartiles %8.3f .. %8.3f   (n = %d)" % (med, q1, q3, len(a))


def synthetic(torch):
    """a plausible film: two planes meeting in an edge, noise of a tenth of the signal, the variance of that noise"""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W]
    side = xx + yy > W
    normal = np.where(side[..., None], [0.0, 0.6, 0.8], [1.0, 0.0, 0.0]).astype(np.float32)
    position = np.stack([xx / W, yy / H, np.where(side, 0.5, 0.2 + 0.3 * xx / W)], axis=2).astype(np.float32)
    signal = np.where(side, 2.0, 0.5)[None, :, :, None] * np.array([1.0, -0.5, 0.25, 2.0])[:, None, None, None] * np.ones(3)
    colour = (signal * (1.0 + 0.1 * rng.standard_normal((K, H, W, 3)))).astype(np.float32)
    variance = (0.1 * np.abs(signal[..., 0])) ** 2 / 3.0
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (colour, variance, normal, position)]


def open_library(path, torch):
    """(library, scene handle on torch's current stream) of this tree's build (path None) or of another build of it, loaded beside it"""
    vp = C.c_void_p
    if path is None:
        L = mi._lib()
    else:
        L = C.CDLL(os.path.abspath(path))
        L.dtof_last_error.restype = C.c_char_p
        L.dtof_scene_load_file.argtypes = [C.c_char_p, vp, vp, C.c_int, C.POINTER(vp)]
        L.dtof_scene_set_stream.argtypes = [vp, vp]
        L.dtof_scene_destroy.argtypes = [vp]
        L.dtof_denoise_async.argtypes = [vp, vp, C.c_int, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
    h = vp()
    names, values = (C.c_char_p * 2)(b"resx", b"resy"), (C.c_char_p * 2)(b"8", b"8")
    assert L.dtof_scene_load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml").encode(), names, values, 2, C.byref(h)) == 0, L.dtof_last_error()
    assert L.dtof_scene_set_stream(h, torch.cuda.current_stream().cuda_stream) == 0, L.dtof_last_error()
    return L, h


def time_levels(torch, reps, naive_lib):
    libs = {TILED: open_library(None, torch)}
    if naive_lib:
        libs[NAIVE] = open_library(naive_lib, torch)
    colour, variance, normal, position = synthetic(torch)
    out = {name: torch.zeros((K, H, W, 3), dtype=torch.float64, device="cuda") for name in libs}
    out_var = {name: torch.zeros((K, H, W), dtype=torch.float64, device="cuda") for name in libs}

    def call(name, levels):
        L, h = libs[name]
        prm = mi._DenoiseParams(levels, 0.1, 0.05, 4.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.dtof_denoise_async(h, colour.data_ptr(), K, W, H, variance.data_ptr(), normal.data_ptr(), position.data_ptr(), C.byref(prm), out[name].data_ptr(),
                                  out_var[name].data_ptr())
        e1.record()
        assert rc == 0, L.dtof_last_error()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {name: {lv: [] for lv in range(1, 7)} for name in libs}
    try:
        for name in libs:      # warm-up: code objects, the scratch
            for lv in range(1, 7):
                call(name, lv)
        same = None
        if naive_lib:
            same = bool(torch.equal(out[TILED].view(torch.int64), out[NAIVE].view(torch.int64)) and torch.equal(out_var[TILED].view(torch.int64), out_var[NAIVE].view(torch.int64)))
        for _ in range(reps):
            for lv in range(1, 7):
                for name in libs:
                    ms[name][lv].append(call(name, lv))
    finally:
        torch.cuda.synchronize()
        for L, h in libs.values():
            L.dtof_scene_destroy(h)
    return ms, same


def wall_errors():
    """section 3: the lines of --wall-out"""
    lines = []
    for res in (64, 256):
        sc = mi.load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml"), resx=res, resy=res)
        index = sc.render_aovs("s:shape_index", seed=0, spp=64)["s"]
        wall = np.abs(index - np.round(index[res // 2, res // 2])) < 1e-6      # every sample of the footprint met the wall
        for spp in (512, 16):
            sigma = None
            for label in ("sigma_position 1 % of the extent (the default)", "sigma_position 10 % of the extent"):
                noisy, den = harness.run_scene_velocity_map_denoised(sc, spp, max_depth=2, denoiser={} if sigma is None else dict(sigma_position=10 * sigma))
                if sigma is None:
                    sigma = sc.denoise_details["denoiser"].last_sigma_position

                def err(m):
                    return float(np.sqrt(np.mean((m[wall] + 10) ** 2))), float(np.mean(m[wall] + 10)), float(np.std(m[wall]))
                lines.append("%3d x %3d, %3d spp, 1 pass, max_depth 2, %5d wall pixels, %-46s   noisy: RMS %.5f (mean error %+.5f, std %.5f)   denoised: RMS %.5f (mean error %+.5f, std %.5f)"
                             % ((res, res, spp, int(wall.sum()), label + ":") + err(noisy) + err(den)))
    return lines


def time_calls(reps):
    """wall-clock of the calls with and without their denoise stage"""
    sc = mi.load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml"), resx=W, resy=H)

    def three_renders():
        sc.render(seed=0, spp=16, variants=VARIANTS)
        sc.render_moments(seed=0, spp=16, variants=VARIANTS)
        sc.render_aovs("p:position,n:sh_normal", seed=0, spp=16)

    def map_alone():
        harness.run_scene_velocity_map(sc, 64, max_depth=2)
        sc.render_moments(seed=0, spp=64, variants=VARIANTS)
        sc.render_aovs("p:position,n:sh_normal", seed=0, spp=64)

    routes = {"render + render_moments + render_aovs, 4 variants, 16 spp": three_renders,
              "Scene.render_denoised, 4 variants, 16 spp": lambda: sc.render_denoised(seed=0, spp=16, variants=VARIANTS),
              "run_scene_velocity_map + render_moments + render_aovs, 64 spp": map_alone,
              "run_scene_velocity_map_denoised, 64 spp": lambda: harness.run_scene_velocity_map_denoised(sc, 64, max_depth=2)}
    for f in routes.values():
        f()
    ms = {name: [] for name in routes}
    for _ in range(reps):
        for name, f in routes.items():
            t0 = time.perf_counter()
            f()
            ms[name].append((time.perf_counter() - t0) * 1e3)
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
                sys.exit("time_denoise.py: bench.py failed with %s: %s" % (name, r.stderr[-2000:]))
            out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append((out["value"], out["ms_per_step_median"], out["config"]["image_checksum"]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--naive-lib", default=None, help="a libdtof.so built with -DDTOF_DENOISE_NAIVE: the one-lane-per-pixel level kernel, timed against this tree's")
    ap.add_argument("--wall-out", default=os.path.join(ROOT, "profiles", "denoise_wall.txt"))
    ap.add_argument("--parent-lib", default=None, help="a libdtof.so of another commit: bench.py is run with it and with this tree's library")
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_ab.txt"))
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() == 0:
        sys.exit("time_denoise.py: no HIP device -- times are only taken on the GPU")
    n = W * H
    level_bytes = n * (32 + 8 * K * 5) + n * 8 * K * 5      # read: the guide record, 3 K colour, K variance, K luminance doubles; written: the same planes
    lines = ["denoiser (tools/time_denoise.py; one process, %d alternating repetitions after a warm-up; %s)" % (args.reps, torch.cuda.get_device_name(0)), "",
             "1. dtof_denoise_async, %d x %d, K = %d, normals + positions + variances; HIP events around the call (k_denoise_pack and L launches of k_denoise_level)" % (W, H, K),
             "   compulsory traffic of one level: %.1f MB (%d B per pixel read, %d written); at 8 TB/s that is %.4f ms" % (level_bytes / 1e6, 32 + 40 * K, 40 * K, level_bytes / 8e12 * 1e3)]
    ms, same = time_levels(torch, args.reps, args.naive_lib)
    med = {name: {lv: float(np.median(v)) for lv, v in m.items()} for name, m in ms.items()}
    for name, m in ms.items():
        lines.append("   %s" % name)
        for lv in range(1, 7):
            inc = med[name][lv] - (med[name][lv - 1] if lv > 1 else 0.0)
            lines.append("     L = %d  %s   %s %8.3f ms%s" % (lv, quartiles(m[lv]), "pack + level of step 1:" if lv == 1 else "level of step %2d adds:   " % (1 << (lv - 1)), inc,
                                                             "" if lv == 1 else "  = %6.2f TB/s of its compulsory bytes" % (level_bytes / (inc * 1e-3) / 1e12 if inc > 0 else float("nan"))))
    if args.naive_lib:
        lines.append("   the two forms' results at L = 6 are bit for bit the same: %s" % same)
        lines.append("   naive / tiled, medians: " + "  ".join("L = %d: %.3fx" % (lv, med[NAIVE][lv] / med[TILED][lv]) for lv in range(1, 7)))
    lines.append("")
    print("\n".join(lines), flush=True)
    part = ["2. cornell_wall.xml %d x %d, max_depth as loaded (render_denoised) and 2 (velocity map); wall-clock around the calls, copies to the host included" % (W, H)]
    calls = time_calls(max(args.reps // 2, 3))
    for name, v in calls.items():
        part.append("   %-64s %s" % (name, quartiles(v)))
    names = list(calls)
    part.append("   the denoise stage adds (medians): %.3f ms to render_denoised, %.3f ms to the velocity map"
                % (np.median(calls[names[1]]) - np.median(calls[names[0]]), np.median(calls[names[3]]) - np.median(calls[names[2]])))
    part.append("")
    print("\n".join(part), flush=True)
    lines += part
    wall = ["denoised against noisy velocity map on the moving wall (tools/time_denoise.py, section 3: harness.run_scene_velocity_map_denoised; scenes/cornell_wall.xml, back wall at",
            "-10 m/s; %s); pixels: those whose aov shape_index is the back wall's up to rounding; errors against the analytic -10 m/s" % torch.cuda.get_device_name(0),
            "the first line is the configuration of tests/test_denoise_gpu.py::test_denoised_velocity_map_is_closer_to_the_walls_velocity", ""] + wall_errors() + [""]
    print("\n".join(wall), flush=True)
    with open(args.wall_out, "w") as f:
        f.write("\n".join(wall))
    if args.parent_lib:
        res = bench_rounds(args.parent_lib, args.bench_rounds, args.bench_steps, 5)
        part = ["4. default route: bench.py --gpus 1 --steps %d --warmup 5, %d fresh processes per build, alternating" % (args.bench_steps, args.bench_rounds)]
        for name, rows in res.items():
            v = np.asarray([r[0] for r in rows])
            part.append("   %-40s Mpaths/s %s   median %.2f, spread %.2f .. %.2f   ms_per_step_median %s   image checksum %s"
                        % (name, " ".join("%.2f" % x for x in v), np.median(v), v.min(), v.max(), " ".join("%.4f" % r[1] for r in rows), sorted({r[2] for r in rows})))
        x, y = list(res)
        part.append("   this tree / parent, medians: %.4fx" % (np.median([r[0] for r in res[x]]) / np.median([r[0] for r in res[y]])))
        part.append("")
        print("\n".join(part), flush=True)
        lines += part
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("written to", args.out)


if __name__ == "__main__":
    main()
