#!/usr/bin/env python3
"""The denoiser's temporal stage against its compulsory bytes, and the default route against a build of another commit.

    python tools/time_temporal.py [--reps 20] [--parent-lib tools/ab/parent.so] [--bench-rounds 4] [--out profiles/temporal_ab.txt]

  1. 512 x 512, K = 4, variance, normals and ids, a history of every buffer, on the device through dtof_denoise_temporal_async (one launch of k_temporal), with
     o_colour_f32: a warm-up, then --reps repetitions that walk through three flow fields (zero; a constant fractional shift; a smooth field of up to +-3 pixels);
     medians and quartiles of HIP events around the call.  Next to it the launch's compulsory bytes -- every input, history and output word once -- and the bandwidth
     that would be.  The method is that of tools/time_denoise.py.
  2. Scene.render_flow against Scene.render_aovs of two channels ("u:uv": the same traversal, splat and develop without the flow arithmetic) on cornell_wall
     512 x 512 x 16 spp and on domino 512 x 512 x 16 spp: wall-clock around the calls, which end in a copy to the host, alternating.
  3. --parent-lib: `bench.py --gpus 1` (the headline workload, which runs no temporal code) with this tree's library and with the given build of another commit
     (DTOF_LIB), --bench-rounds fresh processes each, alternating.

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

W = H = 512
K = 4
BUFFERS = [n for n, _ in mi._TemporalBuffers._fields_]


def quartiles(a):
    q1, med, q3 = np.percentile(np.asarray(a, np.float64), [25, 50, 75])
    return "median %8.4f ms   quartiles %8.4f .. %8.4f   (n = %d)" % (med, q1, q3, len(a))


def synthetic(torch):
    """two surfaces meeting in an edge, noise of a tenth of the signal; the history is the noiseless signal with lengths 1 .. 8"""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W]
    side = xx + yy > W
    normal = np.where(side[..., None], [0.0, 0.6, 0.8], [1.0, 0.0, 0.0]).astype(np.float32)
    ids = (1 + side).astype(np.float32)
    signal = np.where(side, 2.0, 0.5)[None, :, :, None] * np.array([1.0, -0.5, 0.25, 2.0])[:, None, None, None] * np.ones(3)
    colour = (signal * (1.0 + 0.1 * rng.standard_normal((K, H, W, 3)))).astype(np.float32)
    variance = (0.1 * np.abs(signal[..., 0])) ** 2 / 3.0
    length = rng.integers(1, 9, (H, W)).astype(np.float32)
    flows = {"zero flow": np.zeros((H, W, 2), np.float32), "constant (0.25, -1.5)": np.broadcast_to(np.array([0.25, -1.5], np.float32), (H, W, 2)).copy(),
             "smooth, up to 3 pixels": np.stack([3 * np.sin(xx / 40.0) * np.cos(yy / 55.0), 3 * np.cos(xx / 70.0)], axis=2).astype(np.float32)}
    dev = {"colour": colour, "variance": variance, "normal": normal, "ids": ids, "h_colour": signal, "h_variance": variance / length[None], "h_normal": normal,
           "h_ids": ids, "h_length": length}
    dev = {n: torch.from_numpy(np.ascontiguousarray(a)).cuda() for n, a in dev.items()}
    return dev, {n: torch.from_numpy(f).cuda() for n, f in flows.items()}


def time_launch(torch, reps):
    sc = mi.load_file(os.path.join(ROOT, "scenes", "cornell_wall.xml"), resx=8, resy=8)
    sc.set_stream(torch.cuda.current_stream().cuda_stream)
    dev, flows = synthetic(torch)
    out = {"o_colour": torch.zeros((K, H, W, 3), dtype=torch.float64, device="cuda"), "o_variance": torch.zeros((K, H, W), dtype=torch.float64, device="cuda"),
           "o_length": torch.zeros((H, W), dtype=torch.float32, device="cuda"), "o_colour_f32": torch.zeros((K, H, W, 3), dtype=torch.float32, device="cuda")}
    prm = mi._TemporalParams(0.2, 32.0, 0.25)
    L = mi._lib()

    def call(flow):
        tensors = dict(dev, flow=flows[flow], **out)
        buf = mi._TemporalBuffers(*(tensors[n].data_ptr() for n in BUFFERS))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = L.dtof_denoise_temporal_async(sc._h, C.byref(buf), K, W, H, C.byref(prm))
        e1.record()
        assert rc == 0, L.dtof_last_error()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {name: [] for name in flows}
    try:
        for name in flows:
            call(name)
        for _ in range(reps):
            for name in flows:
                ms[name].append(call(name))
        blended = float((out["o_length"] > 1).float().mean())
    finally:
        torch.cuda.synchronize()
        sc.set_stream(None)
    return ms, blended


def time_flow(reps):
    ms = {}
    for name in ("cornell_wall.xml", "domino.xml"):
        sc = mi.load_file(os.path.join(ROOT, "scenes", name), resx=W, resy=H)
        routes = {"render_aovs, 2 channels": lambda: sc.render_aovs("u:uv", seed=0, spp=16), "render_flow": lambda: sc.render_flow(seed=0, spp=16)}
        for f in routes.values():
            f()
        for label in routes:
            ms[(name, label)] = []
        for _ in range(reps):
            for label, f in routes.items():
                t0 = time.perf_counter()
                f()
                ms[(name, label)].append((time.perf_counter() - t0) * 1e3)
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
                sys.exit("time_temporal.py: bench.py failed with %s: %s" % (name, r.stderr[-2000:]))
            out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            res[name].append((out["value"], out["ms_per_step_median"], out["config"]["image_checksum"]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="a libdtof.so of another commit: bench.py is run with it and with this tree's library")
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_ab.txt"))
    args = ap.parse_args()
    import torch
    if torch.cuda.device_count() == 0:
        sys.exit("time_temporal.py: no HIP device -- times are only taken on the GPU")
    n = W * H
    # read: colour 12 K, variance 8 K, normal 12, ids 4, flow 8; history: colour 24 K, variance 8 K, normal 12, ids 4, length 4; written: colour 24 K, variance 8 K,
    # length 4, colour_f32 12 K
    read, written = 12 * K + 8 * K + 12 + 4 + 8 + 24 * K + 8 * K + 12 + 4 + 4, 24 * K + 8 * K + 4 + 12 * K
    total = n * (read + written)
    lines = ["temporal stage (tools/time_temporal.py; one process, %d repetitions walking through the flow fields after a warm-up; %s)" % (args.reps, torch.cuda.get_device_name(0)), "",
             "1. dtof_denoise_temporal_async, %d x %d, K = %d, variance + normals + ids, a full history, o_colour_f32 written; HIP events around the call (one launch of k_temporal)" % (W, H, K),
             "   compulsory traffic: %.1f MB (%d B per pixel read, %d written); at 8 TB/s that is %.4f ms" % (total / 1e6, read, written, total / 8e12 * 1e3)]
    ms, blended = time_launch(torch, args.reps)
    for name, v in ms.items():
        med = float(np.median(v))
        lines.append("   %-24s %s   = %6.2f TB/s of the compulsory bytes" % (name, quartiles(v), total / (med * 1e-3) / 1e12))
    lines.append("   pixels that took a history under the last flow field: %.1f %%" % (100 * blended))
    lines.append("")
    print("\n".join(lines), flush=True)
    part = ["2. the flow film against an aov film of two channels, %d x %d x 16 spp; wall-clock around the calls, copies to the host included" % (W, H)]
    flow_ms = time_flow(args.reps)
    for (name, label), v in flow_ms.items():
        part.append("   %-18s %-26s %s" % (name, label, quartiles(v)))
    for name in ("cornell_wall.xml", "domino.xml"):
        part.append("   %s: render_flow / render_aovs, medians: %.4fx" % (name, np.median(flow_ms[(name, "render_flow")]) / np.median(flow_ms[(name, "render_aovs, 2 channels")])))
    part.append("")
    print("\n".join(part), flush=True)
    lines += part
    if args.parent_lib:
        res = bench_rounds(args.parent_lib, args.bench_rounds, args.bench_steps, 5)
        part = ["3. default route: bench.py --gpus 1 --steps %d --warmup 5, %d fresh processes per build, alternating" % (args.bench_steps, args.bench_rounds)]
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
