"""GPU: examples/arithmetic_replay --steps -- the product of examples/Arithmetic.hs run one SHE operation at a time through the host
mirror's batch forms (ctMulBatch, keySwitchQuadBatch, modSwitchDegBatch over alch_ct_mul, alch_ct_key_switch_quad and
alch_ct_mod_switch_deg), checked inside the program bit for bit against the fused batch path, with the error rate of every step
printed as the reference's writeErrorRates prints them.  The source has no --steps flag before the feature (it reads the word as an
index and fails), so the first test fails on the parent commit."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

STEP_LINE = re.compile(r"^(mul_|keySwitchQuad_|modSwitch_) error rate: (\S+)$", re.M)


@pytest.fixture(scope="module")
def replay_binary():
    exe = os.path.join(ROOT, "examples", "arithmetic_replay")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "examples", "arithmetic_replay.cpp"),
                    "-L" + os.path.join(ROOT, "alchemy_amd", "lib"), "-lalchemy_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "alchemy_amd", "lib")], check=True)
    return exe


@pytest.mark.parametrize("index", ["512", "32"])
def test_steps_flag_prints_the_three_rates_and_pass(replay_binary, index):
    out = subprocess.run([replay_binary, index, "--steps"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = STEP_LINE.findall(out.stdout)
    assert [name for name, _ in lines] == ["mul_", "keySwitchQuad_", "modSwitch_"], out.stdout
    rates = [float(v) for _, v in lines]
    assert all(0.0 < r < 0.5 for r in rates), rates                  # a valid ciphertext: the error is below half the modulus
    assert "step path == fused path: yes" in out.stdout
    assert "fused path == per-op path: yes" in out.stdout
    assert out.stdout.strip().endswith("PASS")


def test_without_the_flag_no_step_lines(replay_binary):
    out = subprocess.run([replay_binary, "32"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert not STEP_LINE.search(out.stdout) and "step path" not in out.stdout
    assert out.stdout.strip().endswith("PASS")
