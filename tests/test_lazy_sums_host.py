"""CPU: the lazy 64-bit sums of the 32-bit word path against unsigned __int128 arithmetic, in a stand-alone program
(tests/sanitize/lazy_sums_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  lazy_group (the group size of
k_tunnel_mac_e, k_tun2_mac<u32> and k_pt_mac<u32>) at every odd modulus within 2^16 of 2^32 / k, k = 3 .. 12; the group chain
(K products of (q-1)^2 on top of the carried sum, three groups) at the largest odd modulus of every class; dense_level at both of
its constants; dense_row<R, LVL> for every R and level the general-index passes instantiate, at the largest modulus of each level.
lazy_group, mont_red_lazy, dense_level and dense_row come from alchemy_amd/csrc/modarith.hpp, the header the kernels include; the
kernels on the device are checked at the same thresholds by tests/test_gpu_word32_thresholds.py."""
import os
import subprocess

from conftest import ROOT


def test_lazy_sums_hold_their_bounds_and_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "lazy_sums_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "lazy_sums_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_the_threshold_moduli_sit_next_to_their_thresholds():
    """Every modulus tests/test_gpu_word32_thresholds.py takes from helpers.group_class_primes / level_edge_primes lies within 2^18
    of the threshold it is meant for, in the intended class; the rings of several limbs stay inside their class."""
    import test_gpu_word32_thresholds as TW
    from helpers import DENSE_LEVEL1_BELOW, DENSE_LEVEL2_BELOW, dense_level, group_class_primes, lazy_group, level_edge_primes
    near, u32 = 1 << 18, (1 << 32) - 1
    assert TW.CLASSES == list(range(3, 12))
    for m in TW.TP_MODULI + TW.GEN_MODULI + TW.PT_MODULI:
        for kmax in TW.CLASSES:
            top, bottom = group_class_primes(m, kmax)
            assert top % m == 1 and bottom % m == 1
            assert 0 <= u32 // kmax - top < near and 0 < bottom - u32 // (kmax + 1) < near, (m, kmax)
            assert u32 // top == kmax == u32 // bottom
            want = 0 if kmax < 4 else min(8, kmax - 2)
            assert lazy_group(top) == lazy_group(bottom) == want == TW.CLASS_K[kmax]
            assert u32 // (top + m) < kmax or not _is_prime(top + m)      # nothing of the class above `top`
    for kmax, d_rel, L in TW.TP_CASES:
        for end in ("top", "bottom"):
            qs = TW.class_ring(max(TW.TP_PAIRS[d_rel]), kmax, L, end)
            assert len(set(qs)) == L
    for kmax, d_rel, L in TW.GEN_CASES:
        rp, sp = TW.GEN_PAIRS[d_rel]
        for end in ("top", "bottom"):
            qs = TW.class_ring(rp * sp // 20 if d_rel == 2 else rp * sp // 21, kmax, L, end)
            assert len(set(qs)) == L and qs[0] % rp == 1 and qs[0] % sp == 1
    for m in TW.LEVEL_M + (315,):
        e = level_edge_primes(m)
        assert all(len(v) == 2 and all(q % m == 1 for q in v) for v in e.values())
        assert all(0 < DENSE_LEVEL2_BELOW - q < near and dense_level([q]) == 2 for q in e["below2"])
        assert all(0 <= q - DENSE_LEVEL2_BELOW < near and dense_level([q]) == 1 for q in e["above2"])
        assert all(0 < DENSE_LEVEL1_BELOW - q < near and dense_level([q]) == 1 for q in e["below1"])
        assert all(0 <= q - DENSE_LEVEL1_BELOW < near and dense_level([q]) == 0 for q in e["above1"])
        assert all(0 < (1 << 31) - q < near and dense_level([q]) == 0 for q in e["top"])
        assert 6 * max(e["below2"]) < 1 << 32 and 6 * max(e["below1"]) ** 2 < 1 << 64 <= 6 * min(e["above1"]) ** 2
    for m in TW.LEVEL_M:
        for name, (_, level) in TW.LEVEL_RINGS.items():
            assert dense_level(TW.level_ring(m, name)) == level


def _is_prime(q):
    from oracle.model import is_prime
    return is_prime(q)
