#!/usr/bin/env python3
"""The time of a two-frequency depth map -- I and Q at 30 and 40 MHz, ONE traversal per pass (Scene.render_depth_map) -- against the two traversals per pass it
replaces (an integrator per frequency, two films each) and against the four films of the same traversal brought to the host; one process, the routes alternating
over three rounds, medians of the library's HIP events and of the wall time of the call -> profiles/multifreq_ab.txt (c).  usage: python tools/time_depth_map.py"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mitsuba3dopplertof_amd as mi
from mitsuba3dopplertof_amd.harness import doppler_integrator_dict
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for scene, params, spp in (("cornell_wall.xml", dict(resx=512, resy=512), 64), ("domino.xml", dict(resx=1024, resy=1024), 64)):
    sc = mi.load_file(os.path.join(ROOT, "scenes", scene), **params)
    kw = dict(time_sampling_method="antithetic", path_correlation_depth=16, max_depth=4)
    sc.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, w_g=30.0, **kw))
    def one():
        t0 = time.perf_counter(); sc.render_depth_map(1, spp, (30.0, 40.0), outputs=("depth",)); wall = time.perf_counter() - t0
        return sc.last_stats["ms_total"], wall * 1e3
    def four():
        t0 = time.perf_counter(); sc.render(seed=0, spp=spp, variants=[(0, 0, 30), (0, .25, 30), (0, 0, 40), (0, .25, 40)]); wall = time.perf_counter() - t0
        return sc.last_stats["ms_total"], wall * 1e3
    def two():
        ms, t0 = 0.0, time.perf_counter()
        for g in (30.0, 40.0):   # what a caller had to do before: an integrator per frequency, I and Q of each in one traversal
            sc.set_integrator(doppler_integrator_dict(hetero_frequency=0.0, hetero_offset=0.0, w_g=g, **kw))
            sc.render(seed=0, spp=spp, variants=[(0.0, 0.0), (0.0, 0.25)]); ms += sc.last_stats["ms_total"]
        return ms, (time.perf_counter() - t0) * 1e3
    for f in (one, four, two): f(); f()
    rows = {"depth_map_one_traversal": [], "render_four_films_one_traversal": [], "render_two_traversals_of_two_films": []}
    for r in range(3):
        for name, f in zip(rows, (one, four, two)):
            t = np.array([f() for _ in range(8)]); rows[name].append((np.median(t[:, 0]), np.median(t[:, 1])))
    print("%s %s %d spp: per round median of  GPU ms of the traversals (HIP events) | wall ms of the call" % (scene, params, spp))
    for name, rr in rows.items():
        print("  %-36s %s" % (name, "   ".join("%.3f | %.3f" % x for x in rr)))
