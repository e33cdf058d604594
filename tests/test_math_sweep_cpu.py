"""The float32 building blocks of dtof_math.h, host leg (no GPU): `math_sweep --cpu` runs the HOST compilation of every case of tests/math_sweep.hip against the
same references the device leg uses (tests/test_math_sweep_gpu.py) over a thinned index space -- 2^28 of the 2^32 bit patterns of the exhaustive cases, 2^26 of
the others; every element keeps its high bits, even ones have zero low bits (so +-0, the infinities, the quiet NaN, powers of two stay in), odd ones random low
bits.  This tests the references, the generators and the class counters on any machine, and it is the host <-> oracle leg of "host, device and the oracle produce
the same bits": under --cpu the restated transcendentals (exp_, log_, tan_, erf_, erfinv_, acos_, cos_, sincos_, atan2_) take the oracle's orc_* export as their
reference, 2^26 inputs each, special values among them.

test_accuracy_against_float64 is the one check that can see an error product and oracle SHARE (both restate the same polynomials): the largest error of each
restated function against float64 libm (erfinv: Newton on erf in float64) over its documented range.  The bounds: where the suite already asserts one
(test_sincos_matches_libm: 2.5e-7 absolute on [-20, 20]; test_emitters.py: 4e-7 absolute for acos) the same bound on at least as many points; everywhere else the
ORACLE's own measured error, rounded up to the next whole ulp.  erf_'s tail (|x| >= 1) is Abramowitz & Stegun 7.1.26, an ABSOLUTE 1.5e-7 approximation: it is
bounded absolutely (the oracle's absolute error rounded up to a whole ulp of 1), not in ulps of 1 - erf.  The table is printed; profiles/math_sweep_accuracy.txt
and DESIGN.md §3 hold a copy.  About 100 s on 8 threads for the whole module."""
import math

import pytest

import sweep_tool as T


@pytest.fixture(scope="module")
def sweep():
    T.build()
    return T


@pytest.mark.parametrize("case", list(T.CASES))
def test_host_compilation_matches_the_reference(sweep, case):
    rc, r, log = T.run(case, ["--cpu", "--oracle", T.ORACLE], timeout=280)
    print(log)
    assert rc == 0, log
    assert r["mode"] == ["cpu"]
    n = len(T.fdiv_divisors()) << 16 if case == "fdiv" else T.CASES[case][1]
    if case == "fdiv":
        assert r["divisors"][0] == len(T.fdiv_divisors())
    T.check(case, r, n, log, thinned_to=n)


def test_cpu_mode_never_touches_the_hip_runtime(sweep):
    """--cpu with no device visible to the child: every HIP call of the program is checked and ends it with a non-zero status, so a run that ends well made none"""
    import os
    import subprocess
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([T.EXE, "signf", "--cpu"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and "mismatches 0" in out.stdout and "mode cpu" in out.stdout, out.stdout + out.stderr


def test_accuracy_against_float64(sweep, capsys):
    rc, r, log = T.run("accuracy", ["--oracle", T.ORACLE], timeout=280)
    assert rc == 0, log
    rows = {}
    with capsys.disabled():
        print("\n%-8s %-18s %14s %14s %10s | %9s %11s | %9s %11s | bound" % ("function", "range", "from", "to", "points", "ulp", "abs", "oracle ulp", "oracle abs"))
        for v in r["acc"]:
            fn, what, lo, hi, n = v[0], v[1], float(v[2]), float(v[3]), int(v[4])
            d_ulp, d_abs, o_ulp, o_abs = float(v[6]), float(v[8]), float(v[10]), float(v[12])
            absolute = (fn, what) == ("erf_", "tail")
            bound = math.ceil(o_abs / 2.0 ** -24) * 2.0 ** -24 if absolute else float(math.ceil(o_ulp))
            rows[(fn, what)] = (d_ulp, d_abs, n)
            print("%-8s %-18s %14.8g %14.8g %10d | %9.3f %11.4g | %9.3f %11.4g | %s" % (fn, what, lo, hi, n, d_ulp, d_abs, o_ulp, o_abs,
                                                                                          "%.4g absolute" % bound if absolute else "%d ulp" % bound))
            assert (d_abs if absolute else d_ulp) <= bound, (fn, what, d_ulp, d_abs, bound)
    assert len(rows) == 13
    # the bounds the suite already asserts, on >= 2^24 points instead of 8 001 / 4 001
    for fn in ("sin_", "cos_"):
        assert rows[(fn, "pm20")][1] < 2.5e-7 and rows[(fn, "pm20")][2] >= 1 << 24
    assert rows[("acos_", "domain")][1] < 4e-7 and rows[("acos_", "domain")][2] >= 1 << 24
    assert rows[("erf_", "tail")][1] < 1.5e-7 + 2.0 ** -24          # A&S 7.1.26's stated error plus one rounding of the result
