"""GPU: the host mirror's hint generation on resident buffers (alchemy_amd/host/symmshe_gen.hpp: ksHintDevice, ksQuadCircHintDevice,
tunnelHintDevice over alch_buf_gauss_dec, l / crt and alch_ct_ks_hint) inside the HomomRLWR replay: with --device-hints the five
tunnel hints and the four quadratic hints of examples/homomrlwr_replay.cpp are made on the device from the genSK keys, and the
unchanged evaluation and closing check -- every result decrypted and compared with the plaintext computation -- still end in PASS.

The flag does not exist on the parent commit: there the replay takes "--device-hints" for a batch size of 0 and the run fails."""
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


def test_device_hints_end_in_pass(replay_exe):
    out = subprocess.run([replay_exe, "5", "--seed", "77", "--quiet-stages", "--device-hints"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("PASS"), out.stdout
    assert "decrypted results equal to the plaintext results: 5 of 5" in out.stdout
    assert re.search(r"^STATS batch 5 .* equal 5 ", out.stdout, flags=re.M)
