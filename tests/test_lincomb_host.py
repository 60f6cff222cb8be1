"""CPU: the weighted sums of alch_ct_automorph_lincomb against unsigned __int128 arithmetic, in a stand-alone program
(tests/sanitize/lincomb_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  lincomb_step / lincomb_close
(alchemy_amd/csrc/modarith.hpp, the expressions k_hoist_lincomb evaluates) on the primes at both ends of every class
floor((2^32 - 1) / q) = 2 .. 11 and the product-at-a-time form on the two largest primes below 2^62, group lengths on either side of K
and beyond 2 K with every operand q - 1; the row-block walk of do_lincomb (kernel_lincomb.hpp: lincomb_blocks, lincomb_block_rows)
covers rows 0 .. n_out - 1 exactly once for n_out up to 3 ROWS + 1.  The kernel on the device: tests/test_gpu_automorph_lincomb.py."""
import os
import re
import subprocess

from conftest import ROOT


def test_weighted_sums_and_row_walk_are_exact_and_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lincomb_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "lincomb_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    # the program walked the ROWS the kernel is built with
    src = open(os.path.join(ROOT, "alchemy_amd", "csrc", "kernel_lincomb.hpp")).read()
    rows, tile = (int(re.search(rf"constexpr int LINCOMB_{k} = (\d+);", src).group(1)) for k in ("ROWS", "TILE"))
    assert f"ROWS {rows} TILE {tile}" in out.stdout


def test_the_trivgad_digits_of_minus_one_are_minus_one(oracle_lib):
    """What tests/test_gpu_automorph_lincomb.py's closed form rests on, on the C restatement: the constant -1 (q - 1 in every CRT
    slot) decomposes into TrivGad digits that are the constant -1 again in every limb, on a two-power and on a general index."""
    import numpy as np
    from helpers import primes_1_mod
    for m in (64, 45):
        qs = primes_1_mod(m, 2, 1 << 28)
        ring = oracle_lib.Ring(32, qs) if m == 64 else oracle_lib.GenRing(m, qs)
        minus_one = np.zeros((ring.n, 2), dtype=np.int64)
        minus_one[0] = [q - 1 for q in qs]
        assert np.array_equal(ring.crt(minus_one), np.broadcast_to(np.array(qs) - 1, (ring.n, 2)))
        digits = ring.decompose_triv(minus_one)
        assert len(digits) == 2 and all(np.array_equal(d, minus_one) for d in digits)
