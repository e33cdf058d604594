"""Shared by tests/test_math_sweep_gpu.py and tests/test_math_sweep_cpu.py: builds tests/math_sweep.hip on first use (the `sweep` target of the kernels' Makefile, so
that it gets exactly $(HIPFLAGS)), runs one case in a child process and parses its "key value..." lines; and the figures a case promises, computed here and not
read from the program: element counts, the size of every exclusion class, the divisor set of fdiv."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "mitsuba3dopplertof_amd")
CSRC = os.path.join(PKG, "csrc")
EXE = os.path.join(PKG, "math_sweep")
EXE_CANDIDATE = os.path.join(PKG, "math_sweep_candidate")
ORACLE = os.path.join(ROOT, "oracle", "libdtof_oracle.so")

# case -> (elements on the device, elements of the thinned host run)
CASES = {
    "rcp": (1 << 32, 1 << 28), "sqrtf": (1 << 32, 1 << 28), "rsqrt_": (1 << 32, 1 << 28), "safe_sqrt": (1 << 32, 1 << 28), "signf": (1 << 32, 1 << 28),
    "truncf": (1 << 32, 1 << 28), "floorf": (1 << 32, 1 << 28), "float_to_int32": (1 << 32, 1 << 28), "int32_to_float": (1 << 32, 1 << 28),
    "uint32_to_float": (1 << 32, 1 << 28), "div": (1 << 32, 1 << 28),
    "fmaf": (1 << 30, 1 << 26), "lerp_": (1 << 30, 1 << 26), "dot": (1 << 30, 1 << 26), "cross": (1 << 30, 1 << 26),
    "fmod_pos_2pi": (1 << 32, 1 << 28), "fmod_pos_xy": (1 << 30, 1 << 26),
    "fdiv": None,                       # divisors x 2^32 / divisors x 2^16, see fdiv_divisors()
    "pcg_jump6": (1 << 30, 1 << 26), "pcg_output_f32": (1 << 30, 1 << 26),
    "permute_kensler": (64 * (257 * 258 // 2 + 1000 + 4096 + 65537),) * 2,
    "mulsign": (8 << 32, 8 << 25), "mulsign_neg": (8 << 32, 8 << 25),
    "exp_": (1 << 32, 1 << 26), "log_": (1 << 32, 1 << 26), "tan_": (1 << 32, 1 << 26), "erf_": (1 << 32, 1 << 26), "erfinv_": (1 << 32, 1 << 26),
    "acos_": (1 << 32, 1 << 26), "cos_": (1 << 32, 1 << 26), "sincos_": (1 << 32, 1 << 26), "atan2_": (1 << 32, 1 << 26),
    "f64_div_sqrt": (1 << 24, 1 << 24),
}
KINDS = {"div": 8, "fmaf": 4, "lerp_": 4, "dot": 4, "cross": 4, "fmod_pos_xy": 4, "atan2_": 8}


def octant_threshold():
    """bit pattern of the smallest positive float x whose x * fl(4 / pi), rounded to float, reaches 2^31: from there on (infinities and NaNs included) the
    (int32_t) conversion of sincos_ / cos_ / tan_ is undefined"""
    c = np.float32(1.2732395447351626862)
    lo, hi = 0, 0x7f800000                      # the product is monotone in x
    while lo < hi:
        mid = (lo + hi) // 2
        if np.array([mid], np.uint32).view(np.float32)[0] * c >= np.float32(2147483648.0):
            hi = mid
        else:
            lo = mid + 1
    return lo


def excluded_bit_patterns(case):
    """the bit-pattern set [first, 0x7fffffff] (either sign) a case excludes, as its first pattern; None when the case excludes nothing"""
    if case == "float_to_int32":
        return 0x4f000000                       # |x| >= 2^31, inf, NaN
    if case in ("tan_", "cos_", "sincos_"):
        return octant_threshold()
    if case in ("exp_", "erf_"):
        return 0x7f800001                       # NaN
    return None


def expected_excluded(case, thinned_to=None):
    """(count, slack): exact over all 2^32 patterns.  A thinned run of 2^k elements visits (i << (32 - k)) | low bits, low bits zero for even i and random for odd i:
    whether an element is in the class is settled by its high k bits except for the one element per sign whose high bits equal the boundary's"""
    first = excluded_bit_patterns(case)
    if first is None:
        return 0, 0
    if thinned_to is None:
        return 2 * (0x80000000 - first), 0
    sh = 32 - thinned_to.bit_length() + 1
    return 2 * ((0x80000000 >> sh) - ((first + (1 << sh) - 1) >> sh)), 2


def config_divisors():
    """every divisor the five BASELINE configurations and the parity CONFIGS put into d_spp, d_w, d_tcn, d_pcn, d_stratum, d_sample_count, d_lanes_per_row and
    d_stripe_rows (dtof_render.hip: spp, crop width, time / path correlate number, sample_count / tcn, width x spp, the stripe heights the suite uses)"""
    from conftest import CONFIGS
    sets = [(256, 16, {}), (512, 64, {}), (512, 256, {}), (1024, 128, {}), (1024, 512, {})]           # BASELINE.json: width, spp
    sets += [(params.get("resx", 256), spp, params) for _, _, params, spp in CONFIGS]
    out = {3, 4}                                                                                      # stripe_rows of the striped renders in the suite
    for w, spp, params in sets:
        for tcn in {int(params.get("time_correlate_number", 2)), 1, 2, 4}:
            out |= {spp, w, w * spp, tcn, int(params.get("path_correlate_number", tcn)), max(spp // tcn, 1)}
    return sorted(out)


PRIMES = [4099, 4999, 7919, 10007, 65521, 65537, 99991, 1000003, 16777213, 16777259, 100000007, 1000000007, 2147483629, 2147483647, 2147483659, 3000000019,
          4294967279, 4294967291]


def fdiv_divisors():
    d = set(range(1, 4097)) | {0xffffffff} | set(PRIMES) | set(config_divisors())
    for k in range(1, 32):
        d |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    return sorted(d)


def build():
    subprocess.check_call(["make", "-C", CSRC, "-j2", "ARCH=gfx950", "sweep"], stdout=subprocess.DEVNULL)
    if not os.path.exists(ORACLE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)


def parse(stdout):
    r, mism = {}, []
    for ln in stdout.splitlines():
        if not ln or ln.startswith("#"):
            continue
        k, *v = ln.split()
        if k == "mismatch":
            mism.append(ln)
        elif k == "acc":
            r.setdefault("acc", []).append(v)
        else:
            r[k] = [int(x) if x.lstrip("-").isdigit() else x for x in v]
    r["mismatch_lines"] = mism
    return r


def run(case, args=(), timeout=600, exe=EXE):
    """one child process; returns (exit status, parsed lines, stdout)"""
    extra = ["--extra", ",".join(str(d) for d in config_divisors())] if case == "fdiv" else []
    out = subprocess.run([exe, case, *extra, *args], capture_output=True, text=True, timeout=timeout)
    return out.returncode, parse(out.stdout), out.stdout + out.stderr[-2000:]


def check(case, r, n_expected, log, thinned_to=None):
    """what both legs assert of a finished run"""
    assert r["mismatches"][0] == 0, "%s: %d mismatches\n%s" % (case, r["mismatches"][0], "\n".join(r["mismatch_lines"]))
    assert r["inputs"][0] == n_expected, (case, r["inputs"], n_expected)
    if "gen_mismatches" in r:
        assert r["gen_mismatches"][0] == 0, "%s: device and host generated different operands\n%s" % (case, log)
        want, slack = expected_excluded(case, thinned_to)
        assert abs(r["excluded"][0] - want) <= slack, (case, r["excluded"], want)
        assert r["compared"][0] == n_expected - r["excluded"][0]
    if "not_permutation" in r:
        assert r["not_permutation"][0] == 0, log
    classes = {k: v[0] for k, v in r.items() if k.startswith("class_")}
    assert all(v > 0 for v in classes.values()), "%s: an empty class makes the check vacuous: %s" % (case, classes)
    for k in range(KINDS.get(case, 0)):
        n, bad = r["kind%d" % k]
        assert n > 0 and bad == 0, (case, k, n, bad)
