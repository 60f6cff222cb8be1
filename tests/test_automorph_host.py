"""CPU: the slot tables of the Galois automorphisms (alchemy_amd/csrc/automorph_host.hpp) in a stand-alone program
(tests/sanitize/automorph_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  For every index
2^a 3^b 5^c 7^d 11^e 13^f with phi <= 384 and every unit j: the table is a permutation of [0, phi) that sends slot k to the slot whose
unit is u(k) j, table(1) is the identity, j and j + m agree, the group law holds, and for a two-power index the table equals the
closed form the radix-16 kernel evaluates per lane -- the same expression, shared through the header -- up to n = 2^16, where an
aligned group of four destination slots also reads one aligned group of four source slots.  The header is compiled alone by the host
compiler: it includes standard headers only."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

PHI_MAX = 384


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("automorph") / "automorph_harness")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")             # the default of alchemy_amd/csrc/Makefile
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", f"-DPHI_MAX={PHI_MAX}", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "sanitize", "automorph_harness.cpp"), "-o", exe], check=True)
    return exe


def test_every_small_index_and_unit_builds_a_consistent_table(harness):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([harness], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "OK: 0 failed expectation(s)", "\n".join(lines[-25:])
    found = re.fullmatch(r"walked (\d+) indices with phi <= (\d+): (\d+) tables, (\d+) units, (\d+) closed-form comparisons", lines[-2])
    assert found, lines[-2]
    indices, bound, tables, units, closed = map(int, found.groups())
    assert bound == PHI_MAX and indices > 150 and tables == units > 10000 and closed > 500


def test_the_header_needs_no_other_header_of_the_library():
    text = open(os.path.join(ROOT, "alchemy_amd", "csrc", "automorph_host.hpp")).read()
    assert re.findall(r'#include\s+"', text) == []
    kernel = open(os.path.join(ROOT, "alchemy_amd", "csrc", "kernel_automorph.hpp")).read()
    assert '#include "automorph_host.hpp"' in kernel and "automorph::pow2_src(" in kernel
