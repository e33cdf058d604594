"""trace_flat's certain-miss test (mitsuba3dopplertof_amd/csrc/dtof_flat_cull.h) is sound: over 10^8 random and adversarial inputs -- any bit pattern, +-0, denormals,
infinities, NaN, zy near 0, maxt = the largest float, quotients within ulps of 0 and of maxt, u and v within an ulp of +-1 -- it never settles a rectangle test whose
t lies in [0, maxt], let alone one that hits.  The rectangle test it is checked against is the kernel's arithmetic, restated in tests/flat_cull_check.cpp.  CPU only."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "mitsuba3dopplertof_amd", "csrc")


def test_flat_cull_never_settles_a_hit(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "flat_cull_check")
    # -ffp-contract=off: a multiply-add happens exactly where fmaf() is written, as in the kernels
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC, os.path.join(HERE, "flat_cull_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "100000000", "7"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = {}
    for ln in out.stdout.splitlines():
        k, *v = ln.split()
        r[k] = [int(x) for x in v]
    print(out.stdout)
    assert r["inputs"][0] >= 100_000_000
    assert r["unsound_range"][0] == 0, out.stderr[-2000:]
    assert r["unsound_hit"][0] == 0
    assert r["room_unsound"][0] == 0
    # the checks are not vacuous: every kind of input both hits and gets culled somewhere
    assert r["culled"][0] > 0 and r["hits"][0] > 0 and r["in_range"][0] > 0
    for k in range(6):
        n, culled, in_range, bad = r["kind%d" % k]
        assert n > 0 and culled > 0 and in_range > 0 and bad == 0, (k, r["kind%d" % k])
    frac = r["room_culled"][0] / r["room_tests"][0]
    print("C2-like shadow rays: %.4f of the wall tests settled by the z row" % frac)
    assert frac > 0.99
