#!/usr/bin/env python3
"""Rates of encrypt_batch with and without a ring key, at the two shapes of section 17's table: n = 2^15 with the
four config-3 moduli (plaintext index 128) and H5' = F20475 (phi 8640) with four HomomRLWR moduli (plaintext index 4095); p = 32.

The rule of DESIGN section 11: same box, same day, alternating runs -- every round visits the unkeyed and the keyed arm once, in ONE
process, `--rounds` rounds; the figure of an arm is the median over the rounds with the spread (max - min) / median next to it.  Beside
encrypt_batch the two sampler calls inside it are timed alone (alch_buf_gauss_dec with a coset, alch_ct_encrypt), which shows where the
difference between the arms comes from; no kernel trace is taken.  Nothing is asserted.

The unkeyed arm against another commit (the parent): `--arms unkeyed --tree DIR` imports `alchemy_amd` from a built checkout of that
commit; run it alternately with `--arms unkeyed` on this tree, several processes each.  `--compare A.log B.log` then prints each arm's
median over its processes, its spread, the relative difference and the bar of twice the larger spread.

    python tools/rng_rates.py [--batch 8192] [--rounds 5] [--arms unkeyed,keyed] [--tree DIR]
    python tools/rng_rates.py --compare this_tree.log other_build.log"""
import argparse
import json
import math
import os
import statistics
import sys

RLWR = [1543651201, 689270401, 718099201, 720720001, 1556755201, 1567238401]
CFG3 = [2147352577, 2146959361, 2146041857, 2145976321]
KEY = bytes(range(32))
SHAPES = (("n=2^15 L=4", 128, 1 << 16, CFG3), ("H5' phi=8640 L=4", 4095, 20475, list(reversed(RLWR[:4]))))


def compare(path_a, path_b):
    def arm(path):
        runs = {}
        for line in open(path):
            if line.startswith('{"shape"'):
                row = json.loads(line)
                runs.setdefault(row["shape"], []).append(row["unkeyed"]["encrypt_batch"]["ciphertexts_per_s"])
        return runs
    a, b = arm(path_a), arm(path_b)
    for name in a:
        ma, mb = statistics.median(a[name]), statistics.median(b[name])
        sa, sb = (max(a[name]) - min(a[name])) / ma, (max(b[name]) - min(b[name])) / mb
        print(json.dumps({"shape": name, "a": {"median": round(ma, 1), "spread": round(sa, 4), "runs": len(a[name])},
                          "b": {"median": round(mb, 1), "spread": round(sb, 4), "runs": len(b[name])},
                          "a_over_b_minus_1": round(ma / mb - 1, 4), "bar": round(2 * max(sa, sb), 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("A_LOG", "B_LOG"))
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default="unkeyed,keyed")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    arms = a.arms.split(",")
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch  # noqa: F401  (before the HIP library: one HIP runtime per process)
    import alchemy_amd as A
    from alchemy_amd import encrypt as E

    p, B = 32, a.batch
    for name, m_pt, m, qs in SHAPES:
        ring, zp_small, zp_big = A.Ring(m, qs), A.Ring(m_pt, [p], nocrt=True), A.Ring(m, [p], nocrt=True)
        zp_small.share_stream(ring)
        zp_big.share_stream(ring)
        svar = 5.0 / math.sqrt(ring.n)
        pt = zp_small.alloc(B)
        pt.fill_uniform(3)
        sk = E.gen_sk(ring, svar, 1)
        coset, err, out = zp_big.alloc(B), ring.alloc(B), ring.alloc(2 * B)
        coset.fill_uniform(4)
        err.fill_uniform(5)

        def timed(fn):
            ring.timer_start()
            fn()
            return ring.timer_stop()

        calls = {
            "encrypt_batch": lambda s: E.encrypt_batch(ring, sk, pt, zp_small, zp_big, svar, s),
            "gauss_dec": lambda s: E.gauss_dec(out, svar * p * p, s, 0, B, coset),
            "ct_encrypt": lambda s: E.ct_encrypt(out, B, err, sk, s),
        }
        ms = {arm: {c: [] for c in calls} for arm in arms}
        for rnd in range(-1, a.rounds):                                   # round -1 warms scratch and pools up, for both arms
            for arm in arms:
                if arm == "keyed":
                    ring.set_rng_key(KEY)
                for c, fn in calls.items():
                    t = timed(lambda: fn(100 + rnd))
                    if rnd >= 0:
                        ms[arm][c].append(t)
                if arm == "keyed":
                    ring.set_rng_key(None)
        row = {"shape": name, "batch": B, "word_bytes": ring.word_bytes, "rounds": a.rounds}
        for arm in arms:
            row[arm] = {}
            for c in calls:
                med = statistics.median(ms[arm][c])
                row[arm][c] = {"ms": round(med, 3), "ciphertexts_per_s": round(B / med * 1e3, 1),
                               "spread": round((max(ms[arm][c]) - min(ms[arm][c])) / med, 4)}
        if "keyed" in arms and "unkeyed" in arms:
            row["keyed_over_unkeyed_time"] = {c: round(row["keyed"][c]["ms"] / row["unkeyed"][c]["ms"], 3) for c in calls}
        print(json.dumps(row), flush=True)
        del pt, sk, coset, err, out


if __name__ == "__main__":
    main()
