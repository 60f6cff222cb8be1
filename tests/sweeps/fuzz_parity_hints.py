"""Randomised parity of the hint pass against Python integers: per trial a random index, limb count, moduli class (31-bit / mixed
small and large / just below 2^62), gadget, n_v, offsets of every buffer, ct0 (small, or within a few entries of 2^64) and a random
cut of the entries into two parts -- alch_ct_ks_hint in one call and alch_ct_ks_hint_part in two, both word for word.
The log goes to profiles/fuzz_parity_hints.log.
Run on the GPU machine:  python tests/sweeps/fuzz_parity_hints.py [--trials N] [--seed S]"""
import argparse
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
from alchemy_amd import capi  # noqa: E402
from alchemy_amd import hints as H  # noqa: E402
from helpers import draw_resident_edge_ring, primes_1_mod, primes_below  # noqa: E402

INDICES = [4, 8, 16, 32, 64, 256, 3, 7, 9, 13, 21, 27, 45, 60, 63, 91, 169, 420]
M64 = (1 << 64) - 1


def moduli(rnd, m, L):
    kind = rnd.choice(["w32", "mixed", "w62"])
    if kind == "w32":
        return kind, primes_1_mod(m, L, 1 << rnd.choice([12, 20, 29]))
    if kind == "w62":
        return kind, primes_below(m, L, 1 << 62)
    return kind, (primes_1_mod(m, max(1, L - 1), 1 << 10) + primes_below(m, 1, 1 << rnd.choice([40, 62])))[:L] if L > 1 else primes_1_mod(m, 1, 1 << 40)


def uniform_words(seed, pair, qs, n):
    """(n, L) Python integers: the odd element of pair `pair` under alch_buf_fill_uniform's rule."""
    L = len(qs)
    cols = []
    for j, q in enumerate(qs):
        pos = (seed + ((2 * pair + 1) * L + j) * n) & M64
        with np.errstate(over="ignore"):
            w = GM.splitmix64(np.uint64(pos) + np.arange(n, dtype=np.uint64))
        cols.append(np.array([int(x) % q for x in w], dtype=object))
    return np.stack(cols, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=120)
    ap.add_argument("--seed", type=int, default=2026)
    a = ap.parse_args()
    rnd = random.Random(a.seed)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    bad = 0
    with open(os.path.join(ROOT, "profiles", "fuzz_parity_hints.log"), "w") as log:
        for trial in range(a.trials):
            m, L = rnd.choice(INDICES), rnd.randint(1, 4)
            kind, qs = draw_resident_edge_ring(rnd, m) if rnd.random() < 0.25 else moduli(rnd, m, L)      # one trial in four: the edge rings
            L = len(qs)
            gadget = rnd.choice([capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2])
            ring = A.Ring(m, qs)
            n, D = ring.n, ring.gadget_digits(gadget)
            ent = [(i, d) for i, q in enumerate(qs) for d in range((q - 1).bit_length() if gadget else 1)]
            assert len(ent) == D
            n_v = rnd.randint(1, 3)
            total = n_v * D
            out_first, v_first, err_first, sk_index = (rnd.randint(0, 3) for _ in range(4))
            seed = rnd.getrandbits(64)
            ct0 = rnd.choice([0, rnd.getrandbits(20), (1 << 64) - rnd.randint(1, total)])
            cut = rnd.randint(0, total)
            one, two = ring.alloc(out_first + 2 * total), ring.alloc(out_first + 2 * total)
            v, err, sk = ring.alloc(v_first + n_v), ring.alloc(err_first + total), ring.alloc(sk_index + 1)
            for b in (one, two, v, err, sk):
                b.fill_uniform(rnd.getrandbits(32))
            keep = one.download(0, out_first) if out_first else None
            H.ct_ks_hint(one, gadget, n_v, v, err, sk, seed, out_first=out_first, v_first=v_first, err_first=err_first, sk_index=sk_index, ct0=ct0)
            for lo, hi in ((0, cut), (cut, total)):
                H.ct_ks_hint_part(two, gadget, lo, hi - lo, v, err, sk, seed, out_first=out_first + 2 * lo, v_first=v_first,
                                  err_first=err_first + lo, sk_index=sk_index, ct0=ct0 + lo)
            got = one.download()
            ok = np.array_equal(two.download()[out_first:], got[out_first:])
            if out_first:
                ok = ok and np.array_equal(got[:out_first], keep)
            vv, ee, ss = v.download()[v_first:].astype(object), err.download()[err_first:].astype(object), sk.download()[sk_index].astype(object)
            q = np.array(qs, dtype=object)
            for e in range(total):
                i, t = divmod(e, D)
                u = uniform_words(seed, (ct0 + e) & M64, qs, n)
                g = np.zeros(L, dtype=object)
                g[ent[t][0]] = 1 << ent[t][1]
                b = (ee[e] - u * ss + g * vv[i]) % q
                ok = ok and np.array_equal(got[out_first + 2 * e + 1].astype(object), u) and np.array_equal(got[out_first + 2 * e].astype(object), b)
            bad += not ok
            line = (f"trial {trial}: m={m} L={L} {kind} gadget={gadget} D={D} n_v={n_v} offsets={out_first},{v_first},{err_first},{sk_index} "
                    f"ct0={ct0} cut={cut} -> {'ok' if ok else 'MISMATCH'}")
            print(line, file=log, flush=True)
            if not ok:
                print(line, flush=True)
            del one, two, v, err, sk
        print(f"{a.trials} trials, {bad} mismatches", file=log)
    print(f"{a.trials} trials, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
