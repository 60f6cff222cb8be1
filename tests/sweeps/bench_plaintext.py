"""Sweep (not part of the suite; needs the GPU): throughput of alch_pt_mul on H5 and of alch_pt_eval_lin on each hop H_k -> H_(k+1) of
the reference's ring round (examples/Common.hs:38-54,78-95) at its plaintext modulus 2^5, on one resident batch.

    python tests/sweeps/bench_plaintext.py [--batch 8192] [--blocks 5] [--reps 10] [--out profiles/plaintext.jsonl]

Each figure is the median over `blocks` blocks of `reps` calls, timed with HIP events on the lifting ring's stream after a warm-up
block; operands are uniform residues (throughput does not depend on the values).  Writes one JSON line per measurement."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import alchemy_amd as A                      # noqa: E402

H = [128, 448, 2912, 3640, 5460, 4095]       # H0 .. H5 (examples/homomrlwr_replay.cpp)
P = 32
LIFT = [1556755201, 1567238401]              # the two word-size primes PtOps lifts to (the last two HomomRLWR moduli)


def timed(ring, fn, reps, blocks):
    fn(); ring.sync()
    out = []
    for _ in range(blocks):
        ring.timer_start()
        for _ in range(reps):
            fn()
        out.append(ring.timer_stop() / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--indices", type=int, nargs="*", default=H, help="the chain of plaintext indices (default H0 .. H5)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plaintext.jsonl"))
    args = ap.parse_args()
    hs = args.indices
    B, lines = args.batch, []
    rng = np.random.default_rng(1)

    def rand(ring, count):
        b = ring.alloc(count); b.fill_uniform(int(rng.integers(1, 1 << 30))); return b

    m5 = hs[-1]
    r5, lift5 = A.Ring(m5, [P], nocrt=True), A.Ring(m5, LIFT)
    a, b, o = rand(r5, B), rand(r5, B), r5.alloc(B)
    ms = timed(lift5, lambda: A.pt_mul(lift5, o, a, b, B), args.reps, args.blocks)
    lines.append({"op": "pt_mul", "m": m5, "n": r5.n, "batch": B, "ms": ms, "per_s": B / ms * 1e3})
    for k in range(len(hs) - 1):
        r, s = hs[k], hs[k + 1]
        rr, rs, lift = A.Ring(r, [P], nocrt=True), A.Ring(s, [P], nocrt=True), A.Ring(s, LIFT)
        d_rel = rr.n // A.Ring(math.gcd(r, s), [P], nocrt=True).n
        f = A.pt_linear(lift, rand(rs, d_rel), r)
        x, y = rand(rr, B), rs.alloc(B)
        ms = timed(lift, lambda: A.pt_eval_lin(f, x, y, B), args.reps, args.blocks)
        lines.append({"op": "pt_eval_lin", "hop": k + 1, "r": r, "s": s, "d_rel": d_rel, "batch": B, "ms": ms, "per_s": B / ms * 1e3})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for ln in lines:
            print(json.dumps(ln)); fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
