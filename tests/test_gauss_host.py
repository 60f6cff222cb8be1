"""CPU: the sampler code the device kernels share with the host (alchemy_amd/csrc/gauss_sampler.hpp, through the host mirror
gaussDecCounter of alchemy_amd/host/cycgen.hpp) in a stand-alone program (tests/sanitize/gauss_harness.cpp) built with
AddressSanitizer and UndefinedBehaviorSanitizer: the scalar deviate at crafted words on both sides of table boundaries
(w0 = 2 T[t] + {-1, 0, 1, 2}, t in {0, 1, 290, 580, 581}; w0 = 0 and 2^64 - 1) and whole elements for m in {16, 21, 45, 91}, without a
coset and with p in {2, 32, 7}, every printed value equal to the Python model's (tests/gauss_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import gauss_model as GM
from conftest import ROOT

ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gauss") / "gauss_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "gauss_harness.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    got = out.stdout.strip().splitlines()
    assert got[-1] == "OK"
    return got[:-1]


def test_scalar_deviate_at_the_table_boundaries(lines):
    T = GM.table()
    rows = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("D ")]
    want_w0 = [(2 * T[t] + d) % (1 << 64) for t in (0, 1, 290, 580, 581) for d in (-1, 0, 1, 2)] + [0, (1 << 64) - 1]
    assert [r[0] for r in rows] == want_w0
    w0 = np.array([r[0] for r in rows], dtype=np.uint64)
    w1 = np.array([r[1] for r in rows], dtype=np.uint64)
    assert [r[2] for r in rows] == GM.deviate(w0, w1).tolist()
    # the boundaries themselves, spelled out: u = T[t] - 1 counts t entries, u = T[t] counts t + 1; the sign is bit 0
    k = lambda r: (r[2] - (r[1] >> 32) + (1 << 31)) >> 32
    for i, t in enumerate((0, 1, 290)):
        assert [k(r) for r in rows[4 * i:4 * i + 4]] == [-t, t + 1, -(t + 1), t + 1], t
    assert T[575] < T[576] == T[580] == T[581] - 1                      # the table's tail is flat: T[576 .. 580] = 2^63 - 2
    assert [k(r) for r in rows[12:16]] == [-576, 581, -581, 582]
    assert [k(r) for r in rows[16:20]] == [-581, 582, -582, 0]          # 2 T[581] + 2 wraps to 0
    assert k(rows[20]) == 0 and k(rows[21]) == -582
    assert all(abs(r[2]) < 1 << 42 for r in rows)


def test_host_mirror_elements_equal_the_model(lines):
    rows = [l for l in lines if l.startswith("E ")]
    assert len(rows) == 4 * 4 * 2
    seen = set()
    for l in rows:
        head, coset, z = [part.split() for part in l[2:].split("|")]
        m, svar_bits, seed, elem, p = [int(v) for v in head]
        svar = float(np.array([svar_bits], dtype=np.uint64).view(np.float64)[0])
        n = GM.totient(m)
        cs = np.array([int(v) for v in coset], dtype=np.int64).reshape(1, n) if p else None
        want = GM.gauss_dec(m, svar, seed, elem, 1, p if p else None, cs)[0].tolist()
        assert [int(v) for v in z] == want, (m, p, elem)
        if p:
            assert all((a - b) % p == 0 for a, b in zip(want, cs[0].tolist()))
        assert max(abs(v) for v in want) > 0
        seen.add((m, p))
    assert seen == {(m, p) for m in (16, 21, 45, 91) for p in (0, 2, 32, 7)}
