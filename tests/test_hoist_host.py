"""CPU: where the hoisted inner product reads (alchemy_amd/csrc/kernel_hoist.hpp through automorph::pow2_pack of automorph_host.hpp), in a
stand-alone program (tests/sanitize/hoist_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly.
For every two-power n from 16 to 2^16, every unit and VL in {2, 4}: the pack address and the picks of the closed form reproduce the
slot table, and each aligned destination pack reads exactly one aligned source pack.  For the general indices 9, 45, 21 and 11648: the
table entries one load of a piece brings are the ones the one-word form reads."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hoist") / "hoist_harness")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")             # the default of alchemy_amd/csrc/Makefile
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-g", "-pthread", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "sanitize", "hoist_harness.cpp"), "-o", exe], check=True)
    return exe


def test_packs_and_picks_reproduce_the_table_for_every_unit(harness):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([harness], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "OK: 0 failed expectation(s)", "\n".join(lines[-25:])
    found = re.fullmatch(r"swept (\d+) units of 13 two-power sizes on (\d+) thread\(s\), (\d+) tables against build_table; (\d+) general units, "
                         r"(\d+) pieces", lines[-2])
    assert found, lines[-2]
    units, threads, cross, gen_units, pieces = map(int, found.groups())
    assert units == sum(1 << logn for logn in range(4, 17))              # every unit of every size
    assert 1 <= threads <= 8 and cross > 1000
    # 9: 6 units (VL = 2 only: n = 6), 45: 24, 21: 12, 11648: the first 64
    assert gen_units == 6 + 24 + 12 + 64
    assert pieces == 6 * 3 + 24 * (6 + 12) + 12 * (3 + 6) + 64 * (4608 // 4 + 4608 // 2)


def test_the_kernel_evaluates_the_shared_expression():
    kernel = open(os.path.join(ROOT, "alchemy_amd", "csrc", "kernel_hoist.hpp")).read()
    assert '#include "automorph_host.hpp"' in kernel and "automorph::pow2_pack<VW>(" in kernel
    host = open(os.path.join(ROOT, "alchemy_amd", "csrc", "automorph_host.hpp")).read()
    assert re.findall(r'#include\s+"', host) == []
