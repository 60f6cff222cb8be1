"""CPU: the three-instruction Plantard product (alchemy_amd/csrc/modarith.hpp: plant_mul3 = two partial products and the closing step
hi32(t1 q + q)) and the butterflies built on it -- the 7-instruction forward butterfly and the 8- / 12-instruction inverse pair on
values kept in [0, q] -- in a stand-alone program (tests/sanitize/plant3_harness.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer.  Per modulus (the headline's four and 1073479681): plant_mul3 against the exact a c mod q and word for
word against the four-instruction plant_mul for a in {0, 1, q-1, q, q+1, 2q-1, 2q, 2^32-1}, c in {0, 1, q-1, R mod q} and 10^5 random
pairs; the closing step alone at t1 = 2^32 - 1, which must give q; the forward butterfly against the Montgomery one (congruent,
outputs below 2q, t = q forced through the closing step); the inverse pair against bfly_inv (entry form on [0,2q), steady form on
[0, q] with both inputs equal to q; outputs at most q).  The kernels' use of them is checked on the device by
tests/test_gpu_plant3.py."""
import os
import subprocess

from conftest import ROOT


def test_plant3_product_and_butterflies_are_exact_and_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "plant3_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "plant3_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "t = q cases: 30" in out.stdout
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
