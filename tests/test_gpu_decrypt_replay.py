"""GPU: the host mirror's batched decrypt (alchemy_amd/host/symmshe_gen.hpp: decryptBatch over alch_ct_decrypt_lift, then divG /
twace / l on the plaintext rings) inside the HomomRLWR replay: with --device-decrypt the closing check of
examples/homomrlwr_replay.cpp prints the same PASS line and the same error-rate statistics as the per-ciphertext host decrypt on
the same seed -- the two runs compute the same maxima, only the place differs.

The flag and the entry point behind it do not exist before library version 1.8: on the parent commit the replay takes
"--device-decrypt" for a batch size of 0 and the comparison below fails."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replay") / "homomrlwr_replay")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "examples", "homomrlwr_replay.cpp"),
                    "-L" + os.path.join(ROOT, "alchemy_amd", "lib"), "-lalchemy_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "alchemy_amd", "lib")], check=True)
    return exe


def test_device_decrypt_prints_pass_and_the_same_statistics(replay_exe):
    runs = []
    for extra in ([], ["--device-decrypt"]):
        out = subprocess.run([replay_exe, "5", "--seed", "77", "--quiet-stages"] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.strip().endswith("PASS"), out.stdout
        runs.append(out.stdout)
    pick = lambda text, pat: re.findall(pat, text, flags=re.M)
    for pat in (r"^STATS .*$", r"^decrypted results equal to the plaintext results: .*$"):
        host, dev = pick(runs[0], pat), pick(runs[1], pat)
        assert len(host) == 1 and host == dev, (host, dev)
    assert "decrypted results equal to the plaintext results: 5 of 5" in runs[1]
    assert re.search(r"^STATS batch 5 .* equal 5 ", runs[1], flags=re.M)
