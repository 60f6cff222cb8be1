"""CPU: the forward butterflies of 32-bit rings with the difference leg written as an absolute difference plus xx (gfx950: v_sad_u32;
alchemy_amd/csrc/modarith.hpp, bfly_fwd(u32...) and bfly_fwd4) against the subtract-and-add formulas they replaced, word for word, in
a stand-alone program (tests/sanitize/bfly_sad_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  Per modulus
(the headline's four, the first of which is the largest prime below 2^31 that is 1 mod 2^16, and 1073479681, the largest of the
benchmark's primes below 2^30; bfly_fwd4 on the latter): x, y in {0, 1, q-1, q, q+1, 2q-1} (bfly_fwd4: x up to 4q-1, y also 2^32-1),
w in {0, 1, q-1, R mod q}, and 10^5 random triples.  t = 0 (y = 0 or w = 0), where the leg returns xx + q (xx + 2q), is counted and
must occur.  The kernels' use of the butterflies is checked on the device by tests/test_gpu_bfly_sad.py."""
import os
import subprocess

from conftest import ROOT


def test_sad_butterflies_give_the_same_words_and_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "bfly_sad_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "bfly_sad_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
