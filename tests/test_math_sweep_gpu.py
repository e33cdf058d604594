"""The float32 building blocks of dtof_math.h on the device, against exact references (tests/math_sweep.hip, compiled with exactly the kernels' $(HIPFLAGS)).

DESIGN.md §3 rests the lane parity of product and oracle on "fused multiply-adds only where fmaf is written, IEEE `/` and sqrt on both".  The parity tests check
the consequence on the lanes of the committed configurations; this module checks the sentence, one parametrised test per case so that a failure names the
function, and the program names the operand:
  A. what the device makes of 1 / x, sqrtf, sqrtf(1 / x), safe_sqrt, signf, truncf, floorf, (int32_t) x, (float) int32, (float) uint32 -- all 2^32 bit patterns
     each -- and of a / b on 2^32 pairs (every exponent pair, boundary quotients, near-ties, 1 / det-like, random), against double precision rounded once
     (53 >= 2 * 24 + 2 bits: the second rounding is harmless); fmaf against the C library's, lerp_ / dot / cross against the host compilation, 2^30 each,
     random and cancellation-heavy;
  B. fmod_pos(x, 2 pi) against fmodf for all 2^32 x and fmod_pos(x, y, 1 / y) on 2^30 pairs; fdiv(n, make_fastdiv(d)) against the definition of the quotient
     for all 2^32 n and 4 171 divisors (compared on the device); pcg_jump6 / pcg_output_f32 on 2^30 states; permute_kensler is a permutation and equals the
     host's for 260 sizes x 64 seeds; mulsign / mulsign_neg for all 2^32 a and 8 special b;
  C. exp_, log_, tan_, erf_, erfinv_, acos_, cos_, sincos_ on all 2^32 inputs and atan2_ on 2^32 pairs: the device against the host compilation of the same
     function (tests/test_math_sweep_cpu.py holds the host against the oracle and against float64).
Nothing is thinned: every case runs the element count sweep_tool.CASES promises.  The only inputs left out of a comparison are those whose float -> int
conversion inside the function is undefined in C++ (|x| 4 / pi >= 2^31 or NaN in sincos_ / cos_ / tan_, NaN in exp_ / erf_, |x| >= 2^31 in the conversion
itself); the program prints how many each exclusion removed and the test holds that against the size of the class computed in sweep_tool.py.

Every case asserts: the child ended with status 0, `mismatches == 0`, the operands the device generated are the ones the host compared (`gen_mismatches`),
`inputs` is what the case promises, and every class count the case prints (denormal in / out, overflow, NaN in, exact, rounded up / down, tie where the
operation has ties, every generator kind) is non-zero.  After a child that ended abnormally no further GPU process is started: every later case fails at once.

Time: the host reference is the cost.  Each child's timeout is three times what the host leg measured for the case (seconds per element on 8 threads,
HOST_SECONDS below, from tests/test_math_sweep_cpu.py's runs), scaled to the case's element count on 16 threads, plus two minutes for start-up and transfers.
Wall times seen on an MI355X host (16 threads) are in WALL_ON_MI355X: 0.3 s (permute_kensler) to 20 s (fmod_pos_2pi: libm's fmodf of huge arguments), 8 s for
the 1.8e13 fdiv checks, 134 s for the whole module.

The candidate slot (test_division_candidate_class_table): the `div` case carries tests/candidates/div_unscaled.h, the unscaled reciprocal + multiply-add chain
of DESIGN §8.3.  Its mismatches are reported per operand class (profiles/math_sweep_div_candidate.txt holds the table), not asserted -- except inside the
exponent window the candidate's header claims to be safe, where there must be none."""
import pytest

import sweep_tool as T

# seconds the host leg took per case on 8 threads for its thinned element count (sweep_tool.CASES[case][1])
HOST_SECONDS = {"rcp": 1.5, "sqrtf": 1.9, "rsqrt_": 2.0, "safe_sqrt": 1.5, "signf": 0.4, "truncf": 1.8, "floorf": 1.5, "float_to_int32": 1.1, "int32_to_float": 1.6,
                "uint32_to_float": 2.2, "div": 2.7, "fmaf": 0.6, "lerp_": 0.4, "dot": 0.7, "cross": 0.9, "fmod_pos_2pi": 13.9, "fmod_pos_xy": 1.6, "fdiv": 0.5,
                "pcg_jump6": 0.1, "pcg_output_f32": 0.1, "permute_kensler": 0.3, "mulsign": 0.6, "mulsign_neg": 0.6, "exp_": 1.3, "log_": 0.6, "tan_": 0.5, "erf_": 3.1,
                "erfinv_": 0.9, "acos_": 1.6, "cos_": 3.6, "sincos_": 3.3, "atan2_": 1.3, "f64_div_sqrt": 0.1}
# seconds per case on the device leg as measured on an MI355X host with 16 compare threads (profiles/math_sweep_gpu.txt); the whole module: 134 s
WALL_ON_MI355X = {"rcp": 2.45, "sqrtf": 1.71, "rsqrt_": 1.90, "safe_sqrt": 1.61, "signf": 0.92, "truncf": 1.16, "floorf": 1.18, "float_to_int32": 0.98,
                  "int32_to_float": 1.55, "uint32_to_float": 1.60, "div": 7.11, "fmaf": 1.73, "lerp_": 1.43, "dot": 2.00, "cross": 2.09, "fmod_pos_2pi": 20.09,
                  "fmod_pos_xy": 4.28, "fdiv": 8.08, "pcg_jump6": 0.61, "pcg_output_f32": 0.55, "permute_kensler": 0.31, "mulsign": 7.67, "mulsign_neg": 7.94,
                  "exp_": 2.90, "log_": 3.07, "tan_": 2.17, "erf_": 3.30, "erfinv_": 5.99, "acos_": 3.61, "cos_": 3.74, "sincos_": 5.01, "atan2_": 6.37,
                  "f64_div_sqrt": 0.34}

_ended_abnormally = []


def _timeout(case, n_gpu):
    n_cpu = len(T.fdiv_divisors()) << 16 if case == "fdiv" else T.CASES[case][1]
    if case == "fdiv":
        return 600          # integer work compared on the device: no host reference to scale; 4 171 launches over 2^32 n each
    return int(min(850, 120 + 3 * HOST_SECONDS[case] * (n_gpu / n_cpu) * 8 / 16))


@pytest.fixture(scope="module")
def sweep():
    T.build()
    return T


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(T.CASES))
def test_device_matches_the_reference(sweep, case):
    if _ended_abnormally:
        pytest.fail("no GPU process is started after one that ended abnormally: %s" % _ended_abnormally[0])
    n = len(T.fdiv_divisors()) << 32 if case == "fdiv" else T.CASES[case][0]
    try:
        rc, r, log = T.run(case, timeout=_timeout(case, n))
    except Exception as e:   # a timeout of the child included
        _ended_abnormally.append("%s: %r" % (case, e))
        raise
    print(log)
    if rc != 0:
        _ended_abnormally.append("%s: exit status %d" % (case, rc))
    assert rc == 0, log
    assert r["mode"] == ["gpu"]
    if case == "fdiv":
        divisors = T.fdiv_divisors()
        assert r["divisors"][0] == len(divisors)
        assert r["class_multiples"][0] == sum(0xffffffff // d + 1 for d in divisors)      # the multiples of d among all n, 0 included
    T.check(case, r, n, log)
    print("%s: %d inputs, 0 mismatches, wall %s s" % (case, n, r["wall_s"][0]))


@pytest.mark.gpu
def test_division_candidate_class_table(sweep, capsys):
    if _ended_abnormally:
        pytest.fail("no GPU process is started after one that ended abnormally: %s" % _ended_abnormally[0])
    try:
        rc, r, log = T.run("div", ["--candidate"], timeout=_timeout("div", 1 << 32), exe=T.EXE_CANDIDATE)
    except Exception as e:
        _ended_abnormally.append("div --candidate: %r" % (e,))
        raise
    if rc != 0:
        _ended_abnormally.append("div --candidate: exit status %d" % rc)
    assert rc == 0, log
    with capsys.disabled():
        print("\nunscaled reciprocal + multiply-add chain for a / b against the correctly rounded quotient (operand class: inputs, mismatches)")
        for k in ("normal", "denormal_operand", "denormal_result", "near_overflow_or_underflow", "special", "safe_window"):
            print("  %-28s %12d %12d" % (k, *r["cand_" + k]))
        print("normal operands that break exactly one condition of the window (unbiased exponents ea, eb): inputs, mismatches, range of that exponent over the mismatches")
        for k, what in (("b_above_125", "eb > 125"), ("b_below_m125", "eb < -125"), ("a_below_m100", "ea < -100"), ("a_minus_b_below_m100", "ea - eb < -100"),
                        ("a_minus_b_above_125", "ea - eb > 125")):
            n, bad, lo, hi = r["cand_only_" + k]
            print("  %-28s %12d %12d   %s" % (what, n, bad, "%d .. %d" % (lo, hi) if bad else "-"))
    assert r["mode"] == ["candidate"] and r["inputs"][0] == 1 << 32 and r["gen_mismatches"][0] == 0
    inside, bad = r["cand_safe_window"]
    assert inside > 1 << 30, "the window the candidate claims to be safe holds too few of the operands to mean anything: %d" % inside
    assert bad == 0, log
    assert all(r["cand_" + k][0] > 0 for k in ("normal", "denormal_operand", "denormal_result", "near_overflow_or_underflow", "special"))
