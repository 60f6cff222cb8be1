"""CPU: the host-callable 64-bit arithmetic of alchemy_amd/csrc/modarith.hpp against unsigned __int128 arithmetic, in a stand-alone
program (tests/sanitize/word64_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer, at every modulus the GPU tests
of the 64-bit word path use (tests/test_gpu_word64_edges.py, the 62-bit rows of tests/test_gpu_decrypt.py) and CFG2_Q60: make_modp and
h_shoup_const; mont_mul_lazy and shoup_mul_lazy on a corner grid and 10^6 random pairs per modulus; bfly_fwd_st over the four stages
of a radix-16 pass with its [0,4q) / [0,2q) ranges checked as 128-bit values; both inverse butterflies and the generic forward one;
csub, add_mod and sub_mod on the corner grid; the digit-entry expressions of k_ks_accum<u64>, balanced and not.
A second invocation is the negative control: with an odd q just above 2^62 the program's own "4q fits the word" expectation fails."""
import os
import subprocess

import pytest

from conftest import CFG2_Q60, ROOT


def gpu_test_moduli():
    import test_gpu_decrypt as TD
    import test_gpu_word64_edges as TW
    qs = set(TW.ALL_MODULI) | {CFG2_Q60}
    for m, L, bits, balanced in TD.lift_ring_cases():
        if bits == 62:
            qs |= set(TD.moduli(m, L, bits, balanced))
    qs |= set(TD.moduli(420, 2, 62, True))
    return sorted(qs)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("word64") / "word64_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "word64_harness.cpp"), "-o", exe], check=True)
    return exe


ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_word64_arithmetic_is_exact_and_clean_under_asan_and_ubsan(harness):
    qs = gpu_test_moduli()
    assert max(qs) < 1 << 62 and sum(q > 1 << 61 for q in qs) >= 20 and 2148728833 in qs and 65537 in qs
    out = subprocess.run([harness] + [str(q) for q in qs], capture_output=True, text=True, env=ENV, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-2] == f"checked {len(qs)} moduli" and lines[-1] == "OK: 0 failed expectation(s)"
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_the_range_expectations_can_fail(harness):
    """Negative control: q = 2^62 + 1 + 2^16 (odd, just outside the accepted range) -- 4q no longer fits the word."""
    q = (1 << 62) + (1 << 16) + 1
    out = subprocess.run([harness, "--negative", str(q)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 1, out.stdout[-3000:] + out.stderr[-3000:]
    assert "q4 < WORD" in out.stdout and f"(q = {q})" in out.stdout
    last = out.stdout.strip().splitlines()[-1]
    assert last.startswith("NEGATIVE CONTROL: ") and int(last.split()[2]) > 0
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    # and the same expectations hold for the largest accepted modulus
    ok = subprocess.run([harness, "--negative", "4611686018427387329"], capture_output=True, text=True, env=ENV, timeout=120)
    assert ok.returncode == 0 and ok.stdout.strip().endswith("NEGATIVE CONTROL: 0 failed expectation(s)")
