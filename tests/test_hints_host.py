"""CPU: the gadget bookkeeping the hint kernel shares with the host (alchemy_amd/csrc/hint_gadget.hpp: the digit -> (limb, exponent)
map of both gadgets and the counter of a uniform word) in a stand-alone program (tests/sanitize/hints_harness.cpp) built with
AddressSanitizer and UndefinedBehaviorSanitizer.  The program checks every entry against a plain nested loop, for L = 1 .. 6 at 17-,
31-, 32- and 62-bit moduli; what it prints is compared here with Python integers."""
import os
import subprocess

import pytest

from conftest import ROOT

ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hints") / "hints_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "hints_harness.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    got = out.stdout.strip().splitlines()
    assert got[-1] == "OK"
    return got[:-1]


def test_layouts_equal_python_integers(lines):
    rows = [l[2:].split("|") for l in lines if l.startswith("G ")]
    assert len(rows) == 4 * 6 * 2
    seen = set()
    for head, qs, first in rows:
        bits, L, gadget, D = (int(v) for v in head.split())
        qs, first = [int(v) for v in qs.split()], [int(v) for v in first.split()]
        assert len(qs) == L and len(first) == L + 1 and all(q.bit_length() == bits for q in qs)
        per = [(q - 1).bit_length() if gadget else 1 for q in qs]                  # ceil(log2 q)
        assert first == [sum(per[:i]) for i in range(L + 1)] and D == sum(per)
        assert all((1 << (k - 1)) < q for k, q in zip(per, qs))                   # the largest gadget scalar stays below its modulus
        seen.add((bits, L, gadget))
    assert seen == {(b, L, g) for b in (17, 31, 32, 62) for L in range(1, 7) for g in (0, 1)}


def test_counters_equal_python_integers(lines):
    rows = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("P ")]
    assert len(rows) == 8 * 6 * 5
    for pair, L, j, n, k, pos in rows:
        assert pos == (((2 * pair + 1) * L + j) * n + k) % (1 << 64), (pair, L, n)
    assert any(((2 * pair + 1) * L + j) * n + k >= 1 << 64 for pair, L, j, n, k, _ in rows)      # some of them wrap
