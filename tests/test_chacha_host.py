"""CPU: the keyed-stream code the device kernels share with the host (alchemy_amd/csrc/chacha_stream.hpp, and through the host mirror
gaussDecCounter of alchemy_amd/host/cycgen.hpp with a key) in a stand-alone program (tests/sanitize/chacha_harness.cpp) built with
AddressSanitizer and UndefinedBehaviorSanitizer: the known-answer blocks, the 128-bit reduction against Python integers (the program
checks it against unsigned __int128 itself) at the moduli of the issue, and whole keyed Gaussian elements for m in {16, 9, 21}, every
printed value equal to the Python model's (tests/chacha_model.py)."""
import os
import subprocess

import numpy as np
import pytest

import chacha_model as CM
import gauss_model as GM
from conftest import ROOT

ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
KEY_E = bytes((200 - 5 * i) & 255 for i in range(32))
RFC = ("e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
       "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split()


def is_prime(n: int) -> bool:
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:                                   # deterministic below 3.3 * 10^24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def primes_below(bound: int, count: int):
    out, q = [], bound - 1
    while len(out) < count:
        if is_prime(q):
            out.append(q)
        q -= 1
    return out


def first_prime_above(bound: int) -> int:
    q = bound + 1
    while not is_prime(q):
        q += 1
    return q


MODULI = primes_below(1 << 31, 2) + primes_below(1 << 62, 2) + [first_prime_above(1 << 31), 65537, 12289]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chacha") / "chacha_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "chacha_harness.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe] + [str(q) for q in MODULI], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    got = out.stdout.strip().splitlines()
    assert got[-1] == "OK"
    return got[:-1]


def test_moduli_are_the_ones_asked_for():
    assert MODULI[0] == (1 << 31) - 1 and MODULI[0] > MODULI[1] > (1 << 30)
    assert (1 << 62) > MODULI[2] > MODULI[3] > (1 << 61)
    assert MODULI[4] == (1 << 31) + 11 and all(is_prime(q) for q in MODULI)


def test_known_answer_blocks(lines):
    v = {l.split()[1]: l.split()[2:] for l in lines if l.startswith("V ")}
    assert v["rfc8439"] == RFC
    as_bytes = lambda ws: b"".join(int(w, 16).to_bytes(4, "little") for w in ws).hex()
    assert as_bytes(v["zero0"][:4]) == "76b8e0ada0f13d90405d6ae55386bd28"
    assert as_bytes(v["zero1"][:2]) == "9f07e7be5551387a"


def test_pairs_through_the_addressing(lines):
    rows = [[int(t) for t in l.split()[1:]] for l in lines if l.startswith("P ")]
    assert [r[1] for r in rows] == [3, 4, 5, 6, 7, 8, (1 << 58) - 1]
    assert rows[1][2:] == [0x15593BD1E4E7F110, 0xC47120A31FDD0F50]
    for d, x, a, b in rows:
        nonce = 0x4A000000 if d == 9 else 77
        A, B = CM.pairs(bytes(range(32)), nonce, d, [x])
        assert (a, b) == (int(A[0]), int(B[0])), (d, x)


def test_reduction_of_128_bits(lines):
    rows = [l.split()[1:] for l in lines if l.startswith("R ")]
    assert len(rows) == len(MODULI) * (9 + 24)
    assert [int(r[0]) for r in rows[::33]] == MODULI
    m64 = (1 << 64) - 1
    for i, q in enumerate(MODULI):
        assert [(int(r[1]), int(r[2])) for r in rows[33 * i:33 * i + 9]] == [(a, b) for a in (0, 1, m64) for b in (0, 1, m64)]
    for q, a, b, r64, r32 in rows:
        want = ((int(b) << 64) | int(a)) % int(q)
        assert int(r64) == want, (q, a, b)
        assert (r32 == "-") == (int(q) >= 1 << 31)
        if r32 != "-":
            assert int(r32) == want, (q, a, b)


def test_keyed_host_mirror_elements_equal_the_model(lines):
    rows = [l for l in lines if l.startswith("E ")]
    assert len(rows) == 3 * 3 * 2
    seen = set()
    for l in rows:
        head, coset, z = [part.split() for part in l[2:].split("|")]
        m, svar_bits, seed, elem, p = [int(v) for v in head]
        svar = float(np.array([svar_bits], dtype=np.uint64).view(np.float64)[0])
        n = GM.totient(m)
        cs = np.array([int(v) for v in coset], dtype=np.int64).reshape(1, n) if p else None
        want = CM.gauss_dec(KEY_E, m, svar, seed, elem, 1, p if p else None, cs)[0].tolist()
        assert [int(v) for v in z] == want, (m, p, elem)
        assert want != GM.gauss_dec(m, svar, seed, elem, 1, p if p else None, cs)[0].tolist()       # and not the unkeyed stream
        if p:
            assert all((a - b) % p == 0 for a, b in zip(want, cs[0].tolist()))
        seen.add((m, p, elem == 3))
    assert seen == {(m, p, s) for m in (16, 9, 21) for p in (0, 2, 7) for s in (True, False)}
