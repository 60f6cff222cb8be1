"""GPU: the host mirror's plaintext batches (alchemy_amd/host/cycgen.hpp: PtBatch and the batch forms of mul, addScalar, div2 and
evalLin over alch_pt_mul, alch_buf_add_bcast, alch_pt_rescale, alch_pt_eval_lin) inside the HomomRLWR replay: with
--device-plaintext the plaintext side of examples/homomrlwr_replay.cpp is computed on resident batches, and the replay prints the
same PASS, the same "decrypted results equal" line and the same STATS line as with the per-element host computation on the same seed
-- and the same per-stage lines, which compare ciphertext 0's decryption with the plaintext stage.

The flag does not exist before the feature: the parent's replay takes "--device-plaintext" for a batch size of 0."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replay_pt") / "homomrlwr_replay")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "examples", "homomrlwr_replay.cpp"),
                    "-L" + os.path.join(ROOT, "alchemy_amd", "lib"), "-lalchemy_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "alchemy_amd", "lib")], check=True)
    return exe


def test_device_plaintext_prints_pass_and_the_same_lines(replay_exe):
    runs = []
    for extra in ([], ["--device-plaintext"]):
        out = subprocess.run([replay_exe, "64", "--seed", "77"] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("PASS"), out.stdout
        runs.append(out.stdout)
    pick = lambda text, pat: re.findall(pat, text, flags=re.M)
    for pat in (r"^STATS .*$", r"^decrypted results equal to the plaintext results: .*$"):
        host, dev = pick(runs[0], pat), pick(runs[1], pat)
        assert len(host) == 1 and host == dev, (host, dev)
    assert "decrypted results equal to the plaintext results: 64 of 64" in runs[1]
    stage = r"^  .*decrypts to the plaintext stage: .*$"
    assert len(pick(runs[0], stage)) >= 7 and pick(runs[0], stage) == pick(runs[1], stage)
    assert all("every div2 operand even: yes" in r for r in runs)
    # everything but the timings is the same text
    strip = lambda text: re.sub(r"\d+\.\d+ s", "T s", text)
    assert strip(runs[0]) == strip(runs[1])
