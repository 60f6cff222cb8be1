"""CPU: the scratch planning of the chunked walks (alchemy_amd/csrc/scratch_plan.hpp) where it needs no GPU.

scratch_chunk and fused_chunk against the formulas the walks spelled out one by one before the header owned them, their bounds, that
no product wraps for items up to 2^40 bytes, and the carve cursor, in a stand-alone program (tests/sanitize/scratch_plan_harness.cpp)
built with AddressSanitizer and UndefinedBehaviorSanitizer; and that the header stays host-only."""
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "alchemy_amd", "csrc", "scratch_plan.hpp")


def test_chunk_rules_and_carve_cursor_are_exact_and_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "scratch_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "scratch_plan_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_the_header_is_host_only_and_the_library_includes_it():
    text = open(HEADER).read()
    assert not re.search(r"#include\s*[<\"][^>\"]*hip", text) and "__global__" not in text and "__device__" not in text
    lib = open(os.path.join(ROOT, "alchemy_amd", "csrc", "alchemy_hip.hip")).read()
    assert '#include "scratch_plan.hpp"' in lib
    # one definition of the rule: no walk spells it out again
    assert not re.search(r"std::max<size_t>\(1, \(\w+->scratch_mib << 20\)", lib)
