"""Randomised parity of the encrypt path against the Python model (tests/gauss_model.py): per trial a random index, limb count, moduli
class (31-bit / mixed small and large / just below 2^62), coset modulus (or none), batch, offsets, elem0 and a random cut of the batch
into chunks -- alch_buf_gauss_dec word for word, then alch_ct_encrypt of the same error terms against Python integers.
The log goes to profiles/fuzz_parity_encrypt.log.
Run on the GPU machine:  python tests/sweeps/fuzz_parity_encrypt.py [--trials N] [--seed S]"""
import argparse
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import alchemy_amd as A  # noqa: E402
import gauss_model as GM  # noqa: E402
from alchemy_amd import encrypt as E  # noqa: E402
from helpers import draw_resident_edge_ring, primes_1_mod, primes_below  # noqa: E402

INDICES = [4, 8, 16, 32, 64, 256, 3, 7, 9, 13, 21, 27, 45, 60, 63, 91, 169, 420, 1365, 4095, 2912]
P_SET = [None, 2, 3, 7, 8, 32, 1 << 20, (1 << 31) - 1]


def moduli(rnd, m, L):
    kind = rnd.choice(["w32", "mixed", "w62"])
    if kind == "w32":
        return kind, primes_1_mod(m, L, 1 << rnd.choice([12, 20, 29]))
    if kind == "w62":
        return kind, primes_below(m, L, 1 << 62)
    return kind, (primes_1_mod(m, max(1, L - 1), 1 << 10) + primes_below(m, 1, 1 << rnd.choice([40, 62])))[:L] if L > 1 else primes_1_mod(m, 1, 1 << 40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=200)
    ap.add_argument("--seed", type=int, default=2026)
    a = ap.parse_args()
    rnd = random.Random(a.seed)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    bad = 0
    with open(os.path.join(ROOT, "profiles", "fuzz_parity_encrypt.log"), "w") as log:
        for trial in range(a.trials):
            m, L, p = rnd.choice(INDICES), rnd.randint(1, 4), rnd.choice(P_SET)
            kind, qs = draw_resident_edge_ring(rnd, m) if rnd.random() < 0.25 else moduli(rnd, m, L)      # one trial in four: the edge rings
            L = len(qs)
            count, first = rnd.randint(1, 9), rnd.randint(0, 3)
            seed, elem0 = rnd.getrandbits(64), rnd.choice([0, rnd.getrandbits(20), (1 << 64) - rnd.randint(1, 5)])
            svar = rnd.choice([3.0, 5.0, 50.0]) / math.sqrt(GM.totient(m)) * (float(p) ** 2 if p else 1.0)
            ring = A.Ring(m, qs)
            dst = ring.alloc(first + count)
            cb = cw = None
            if p:
                zp = A.Ring(m, [p], nocrt=True)
                cb = zp.alloc(first + count)
                cb.fill_uniform(rnd.getrandbits(32))
                cw = cb.download()[first:, :, 0]
            cut = rnd.randint(0, count)
            for lo, hi in ((0, cut), (cut, count)):
                E.gauss_dec(dst, svar, seed, first + lo, hi - lo, cb, first + lo, elem0 + lo)
            z = GM.gauss_dec(m, svar, seed, elem0, count, p, cw)
            ok = np.array_equal(dst.download()[first:], GM.words(z, qs))
            # the RLWE pass on these error terms (taken as CRT-basis words) against Python integers
            sk, out = ring.alloc(1), ring.alloc(2 * count)
            sk.fill_uniform(rnd.getrandbits(32))
            useed, ct0 = rnd.getrandbits(64), rnd.getrandbits(16)
            E.ct_encrypt(out, count, dst, sk, useed, err_first=first, ct0=ct0)
            got, e, s = out.download(), dst.download()[first:], sk.download()[0]
            n = ring.n
            for b in range(count):
                for j, q in enumerate(qs):
                    pos = (((2 * (ct0 + b) + 1) * L + j) * n + np.arange(n, dtype=np.uint64).astype(object)) + useed
                    c1 = [E.splitmix64(int(v) & ((1 << 64) - 1)) % q for v in pos]
                    c0 = [(int(ev) - u * int(sv)) % q for ev, u, sv in zip(e[b, :, j], c1, s[:, j])]
                    ok = ok and got[2 * b + 1, :, j].tolist() == c1 and got[2 * b, :, j].tolist() == c0
            bad += not ok
            line = f"trial {trial}: m={m} L={L} {kind} p={p} count={count} first={first} cut={cut} elem0={elem0} -> {'ok' if ok else 'MISMATCH'}"
            print(line, file=log, flush=True)
            if not ok:
                print(line, flush=True)
            del dst, cb, sk, out
        print(f"{a.trials} trials, {bad} mismatches", file=log)
    print(f"{a.trials} trials, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
