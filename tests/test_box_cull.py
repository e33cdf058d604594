"""The slab test of the TLAS / BLAS walks (mitsuba3dopplertof_amd/csrc/dtof_box_cull.h) is conservative: tests/box_cull_check.cpp compiles slab_ray and box_hit for the
host and runs them over the rays of families B (box rims), F (far origins) and E (small direction components) of tests/tree_sweep.py with the padded bounds, as floats and
as half floats, of the triangles and meshes those rays hit -- with the reciprocal as 1.f / x and moved one ulp either way, since v_rcp_f32 is a one-ulp reciprocal.  No ray
that passes through the unpadded box may be culled.  The check also counts what the test as it was before (exact zeros nudged only, tn <= tf) culls of them: far origins
and small components, the two defects the contract was written for.  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tree_sweep as ts

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba3dopplertof_amd", "csrc")
SCENES = ("slab_small", "slab_unit", "blobs", "ties")


@pytest.fixture(scope="module")
def records(orc, tmp_path_factory):
    out = {}
    for name in SCENES:
        sw = ts.Sweep(name, orc, tmp_path_factory.mktemp(name))
        out[name] = ts.cull_records(sw)
    out["issue"] = ts.issue_records()
    return out


@pytest.mark.parametrize("ulps", (0, 1, -1))
def test_no_ray_through_the_unpadded_box_is_culled(records, tmp_path, ulps):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "box_cull_check")
    # -ffp-contract=off: a multiply-add happens exactly where fmaf() is written, as in the kernels
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC] + (["-DDTOF_SLAB_RCP_ULPS=%d" % ulps] if ulps else []) +
                          [os.path.join(HERE, "box_cull_check.cpp"), "-o", exe])
    parent_culled = {}
    for name, rec in records.items():
        path = str(tmp_path / (name + ".f32"))
        np.ascontiguousarray(rec, np.float32).tofile(path)
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        r = {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()}
        print(name, "reciprocal %+d ulp:" % ulps, r)
        assert r["records"] == len(rec) and r["records"] > 0
        # not vacuous: most of these rays do pass through their boxes (they hit a triangle inside them)
        assert r["through"] * 2 >= r["records"], (name, r)
        assert r["culled_float"] == 0 and r["culled_half"] == 0, (name, r, out.stderr[-2000:])
        parent_culled[name] = r["parent_culled_float"]
    # the test as it was is caught by these very records: small components (the issue's box) and far origins (the small slab from 1e3 and 1e4 extents away)
    assert parent_culled["issue"] > 0 and parent_culled["slab_small"] > 0, parent_culled
