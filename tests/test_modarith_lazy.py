"""CPU: the lazy accumulator arithmetic of the key-switch kernel against unsigned __int128 arithmetic, in a stand-alone program
(tests/sanitize/modarith_lazy_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer: the corner grid
{0, 1, q-1, q, q+1, 2q-2, 2q-1}^2 and 10^6 random pairs per modulus, x in {0, 2q-1, 2^32-1}, every modulus the GPU tests of the
kernel use and 12289.  sub_lazy, csub and mont_mul_lazy come from alchemy_amd/csrc/modarith.hpp, the header the kernel includes; the
accumulate step and the negated stage 0 are restated in the program from kernel_ks_half.hpp (the kernel's own expressions are
checked on the device by tests/test_gpu_ks_lazy_acc.py)."""
import os
import subprocess

from conftest import ROOT


def test_lazy_arithmetic_is_exact_and_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "modarith_lazy_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "modarith_lazy_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
