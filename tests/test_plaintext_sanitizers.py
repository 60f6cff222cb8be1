"""CPU: AddressSanitizer + UndefinedBehaviorSanitizer over the new host-only arithmetic of the plaintext-side entry points --
the 128-bit coefficient bound behind alch_pt_bound and the test Q / 2 > bound (alchemy_amd/csrc/plain_host.hpp) -- in a stand-alone
program (tests/sanitize/plain_bound_harness.cpp): extreme indices, moduli and term counts, and lifting rings whose full modulus
product would not fit 128 bits.  The library includes the same header, so this is the code the entry points run."""
import os
import subprocess

from conftest import ROOT

CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


def test_bound_arithmetic_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "plain_bound_harness")
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,unsigned-integer-overflow",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "sanitize", "plain_bound_harness.cpp"), "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    src = open(os.path.join(ROOT, "alchemy_amd", "csrc", "alchemy_hip.hip")).read()
    assert '#include "plain_host.hpp"' in src and "pt_bound_value(" in src and "pt_q_exceeds(" in src
