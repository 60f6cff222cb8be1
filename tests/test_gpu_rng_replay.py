"""GPU: the HomomRLWR replay of the host mirror with every device sampler under a key -- examples/homomrlwr_replay.cpp with
--device-encrypt --device-hints --rng-key: the ring cache sets the key on every ring (alch_ring_set_rng_key), the keys' hints and the
encrypted secret come from ChaCha20 keystreams, and the unchanged evaluation and closing check still end in PASS.

The flag does not exist on the parent commit: there the replay takes "--rng-key" for a batch size of 0 and the run fails."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KEY_HEX = "".join(f"{(17 * i + 3) & 255:02x}" for i in range(32))


@pytest.fixture(scope="module")
def replay_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replay") / "homomrlwr_replay")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "examples", "homomrlwr_replay.cpp"),
                    "-L" + os.path.join(ROOT, "alchemy_amd", "lib"), "-lalchemy_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "alchemy_amd", "lib")], check=True)
    return exe


def test_keyed_device_samplers_end_in_pass(replay_exe):
    out = subprocess.run([replay_exe, "5", "--seed", "77", "--quiet-stages", "--device-encrypt", "--device-hints", "--rng-key", KEY_HEX],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rng: ChaCha20 keystreams" in out.stdout
    assert out.stdout.strip().endswith("PASS"), out.stdout
    assert "decrypted results equal to the plaintext results: 5 of 5" in out.stdout
    assert re.search(r"^STATS batch 5 .* equal 5 ", out.stdout, flags=re.M)


def test_a_malformed_key_is_refused(replay_exe):
    out = subprocess.run([replay_exe, "5", "--rng-key", "abc"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "64 hex digits" in out.stderr
