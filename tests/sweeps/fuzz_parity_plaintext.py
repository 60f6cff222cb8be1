"""Sweep (not part of the suite; needs the GPU): random indices, plaintext moduli, lifting rings, batches and scratch sizes for
alch_pt_mul / alch_pt_eval_lin / alch_pt_rescale against the by-definition model.

    python tests/sweeps/fuzz_parity_plaintext.py [--rounds N] [--seed S]

Prints one line per round and exits non-zero at the first mismatch."""
import argparse
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import alchemy_amd as A                      # noqa: E402
from helpers import primes_1_mod, threshold_moduli   # noqa: E402
from oracle import model_gen as G            # noqa: E402

INDICES = [4, 8, 9, 12, 15, 16, 20, 21, 28, 32, 36, 45, 63, 64, 91, 128, 448]
MODULI = [2, 4, 7, 8, 9, 32, 100]


def lift_ring(m, rng):
    kind = rng.choice(["two31", "one60", "three29", "edges", "edges"])   # edges: the ends of k_pt_mac's group-size classes
    qs = {"two31": lambda: primes_1_mod(m, 2, 1 << 30), "one60": lambda: primes_1_mod(m, 1, 1 << 59),
          "three29": lambda: primes_1_mod(m, 3, 1 << 28), "edges": lambda: threshold_moduli(rng, m, 2)}[kind]()
    r = A.Ring(m, qs)
    r.set_option("scratch_mib", rng.choice([1, 2, 4096]))
    return r, kind


def up(ring, elems):
    return ring.upload(np.asarray(elems, dtype=np.int64).reshape(len(elems), ring.n, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    rng = random.Random(args.seed)
    for rnd in range(args.rounds):
        m, p, batch = rng.choice(INDICES), rng.choice(MODULI), rng.choice([1, 2, 5, 17])
        idx = G.Index(m)
        lift, kind = lift_ring(m, rng)
        r = A.Ring(m, [p], nocrt=True)
        a = [[rng.randrange(p) for _ in range(idx.n)] for _ in range(batch)]
        b = [[rng.randrange(p) for _ in range(idx.n)] for _ in range(batch)]
        out = r.alloc(batch)
        A.pt_mul(lift, out, up(r, a), up(r, b), batch)
        ok = out.download()[:, :, 0].tolist() == [G.ring_mul_def(x, y, idx, p) for x, y in zip(a, b)]
        # a hop from a random index to this one
        rr = rng.choice(INDICES)
        e = math.gcd(rr, m)
        E, R = G.Index(e), G.Index(rr)
        ys = [[rng.randrange(p) for _ in range(idx.n)] for _ in range(R.n // E.n)]
        xs = [[rng.randrange(p) for _ in range(R.n)] for _ in range(batch)]
        f = A.pt_linear(lift, up(r, ys), rr)
        dst = r.alloc(batch)
        A.pt_eval_lin(f, up(A.Ring(rr, [p], nocrt=True), xs), dst, batch)
        ok_lin = dst.download()[:, :, 0].tolist() == [G.eval_lin_dec(ys, G.linv_def(x, R, p), E, R, idx, p) for x in xs]
        # rescale by a random divisor
        divs = [d for d in range(2, p + 1) if p % d == 0 and p // d >= 2]
        ok_rs = True
        if divs:
            d = rng.choice(divs)
            half = A.Ring(m, [p // d], nocrt=True).alloc(batch)
            even = A.pt_rescale(up(r, a), half, batch)
            ok_rs = half.download()[:, :, 0].tolist() == [[v // d for v in x] for x in a] and even == all(v % d == 0 for x in a for v in x)
        print(f"round {rnd}: m={m} p={p} batch={batch} lift={kind} hop {rr}->{m}: mul {ok} evalLin {ok_lin} rescale {ok_rs}", flush=True)
        if not (ok and ok_lin and ok_rs):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
