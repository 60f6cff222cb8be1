"""CPU: stage01_signed (alchemy_amd/csrc/modarith.hpp) -- stages 0-1 of the key-switch kernel's pass G as one signed sum over four
centred digits -- against __int128 arithmetic, in a stand-alone program (tests/sanitize/stage01_signed_harness.cpp) built with
AddressSanitizer and UndefinedBehaviorSanitizer.  Per modulus (the headline's four, 2^31 - 1, one below 2^30, two small ones), per
digit range (the modulus itself, 2^31 - 1, 65537), per half, per sign and per twiddle pair: all 6^4 tuples of the extreme digits
{0, 1, -1, (q-1)/2, -(q-1)/2, (q-3)/2} and 500 random ones.  It asserts the helper's preconditions, 0 < S +- T < q 2^32, that nothing
wraps in 64 bits, the residues and the range [0, 2q).  The kernel's own use of the helper is checked on the device by
tests/test_gpu_ks_signed_stage01.py."""
import os
import subprocess

from conftest import ROOT


def test_signed_stage01_is_exact_and_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "stage01_signed_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "stage01_signed_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "OK: 0 failed expectation(s)" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
