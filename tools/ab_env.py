#!/usr/bin/env python3
"""A/B timing on one GPU box of several (library, environment) variants of the same workload, interleaved over several rounds.
usage: ab_env.py scene.xml [spp] -- name=[LIB.so][,ENV=VAL ...] ...   e.g.  ab_env.py cornell_wall.xml -- base=tools/ab/base.so new= memo0=,DTOF_INSTANCE_MEMO=0
Two pseudo-variables shape the workload of a variant instead of its environment: D:name=value is a -D parameter of the scene file (D:resx=1024), and
FILMS=offsets | variants renders four films per traversal -- hetero_offset 0, 0.25, 0.5, 0.75 (dtof_render_offsets), or the homodyne / heterodyne pairs
(0, 0), (0, 0.25), (1, 0), (1, 0.25) (dtof_render_variants) -- over 12 frames instead of 30.
AB_ROUNDS (default 3) and AB_FRAMES (default 30, of which the first 5 are dropped; 12 and 3 with FILMS) in the environment size the comparison.
Prints min / median of ms_total, ms_first (first-bounce kernel) and of the bounce-kernel launches (HIP events of the library)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]; k = args.index("--"); scene = args[0]; spp = int(args[1]) if k > 1 else 0
variants = []
for v in args[k + 1:]:
    name, rest = v.split("=", 1); parts = rest.split(",")
    env = dict(p.split("=", 1) for p in parts[1:] if p and not p.startswith("D:"))
    env["AB_PARAMS"] = repr(dict(p[2:].split("=", 1) for p in parts[1:] if p.startswith("D:")))
    env["AB_FILMS"] = env.pop("FILMS", "")
    if parts[0]: env["DTOF_LIB"] = os.path.join(ROOT, parts[0])
    variants.append((name, env))
code = ("import sys, numpy as np; sys.path.insert(0, %r); import mitsuba3dopplertof_amd as mi\n"
        "import os; films = os.environ.get('AB_FILMS', ''); sc = mi.load_file(%r, **eval(os.environ.get('AB_PARAMS', '{}')))\n"
        "kw = dict(offsets=[0.0, 0.25, 0.5, 0.75]) if films == 'offsets' else dict(variants=[(0.0, 0.0), (0.0, 0.25), (1.0, 0.0), (1.0, 0.25)]) if films == 'variants' else {}\n"
        "T = []\n"
        "for i in range(int(os.environ.get('AB_FRAMES', 0)) or (12 if films else 30)):\n"
        "    sc.render(seed=0, spp=%d, **kw); s = sc.last_stats; T.append((s['ms_total'], s['ms_first'], (s['ms_shade'] - s['ms_first']) / max(s['n_launches_shade'] - s['n_launches_first'], 1), s['ms_trace'], s['ms_shadow'], s['ms_splat']))\n"
        "T = np.array(T[3 if films else 5:]); print(' '.join('%%.3f/%%.3f' %% (T[:, j].min(), np.median(T[:, j])) for j in range(6)))\n" % (ROOT, os.path.join(ROOT, "scenes", scene), spp))
res = {n: [] for n, _ in variants}
for r in range(int(os.environ.get("AB_ROUNDS", 3))):
    for n, env in variants:
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)   # a round is seconds
        if out.returncode != 0:   # a child that failed ends the comparison: nothing more is started on that GPU
            sys.exit("%s, round %d: exit status %d\n%s" % (n, r, out.returncode, out.stderr[-2000:]))
        res[n].append(out.stdout.strip() or out.stderr[-300:])
print("variant: per round min/median of  total | first | bounce launch | trace | shadow | splat  (ms)")
for n, _ in variants:
    for r in res[n]: print("%-14s %s" % (n, r))
