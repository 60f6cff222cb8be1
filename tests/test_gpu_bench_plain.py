"""GPU: bench.py's plain run (no --full) times the headline only, and --dump-outputs writes what its last timed step computed:
a seeded sample of the result ciphertexts, equal word for word to what the C oracle computes from the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CFG3_QS, ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("batch_checksum", "out_checksum", "full_mul", "pow_basis_in_out", "general_index", "homomrlwr", "tunnel_hs", "config2",
             "moduli_below_2_30", "n16_six_limbs", "result_gather", "cpu_baseline")


def test_plain_run_dumps_the_last_step(tmp_path, oracle_lib):
    B, steps = 64, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(B),
           "--dump-outputs", str(tmp_path / "dump")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "ctxt-mul+relinearize/sec at n=2^15, 4 RNS limbs" and d["unit"] == "ctxt-mul+relin/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u32" and d["steps"] == steps
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - B * steps / (d["ms_per_step"] * steps * 1e-3)) < 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d], "a plain run measures the headline only"

    got = np.load(tmp_path / "dump" / "ct_mul_relin_out.npy")
    idx = np.load(tmp_path / "dump" / "ct_mul_relin_out_index.npy")
    assert got.dtype == np.float64 and idx.dtype == np.float64
    assert got.shape == (16, 2, 1 << 15, 4) and got.nbytes + idx.nbytes <= 64 << 20
    assert len(set(idx.tolist())) == 16 and 0 <= idx.min() and idx.max() < B

    # the oracle's own result for each sampled ciphertext, from bench.py's seeded inputs
    o = oracle_lib.Ring(1 << 15, CFG3_QS)
    hint = [o.fill_uniform(0xA1C4E5, i) for i in range(2 * len(CFG3_QS))]
    for k, ct in enumerate(int(x) for x in idx):
        w0, w1 = o.ct_mul_relin(hint, o.fill_uniform(2026, 2 * ct), o.fill_uniform(2026, 2 * ct + 1),
                                o.fill_uniform(900_000_007, 2 * ct), o.fill_uniform(900_000_007, 2 * ct + 1))
        assert np.array_equal(got[k, 0], w0) and np.array_equal(got[k, 1], w1), ct
