#!/usr/bin/env python3
"""Weighted sums of hoisted rotations on resident batches, measured (include/alchemy_hip.h, "Weighted sums of hoisted rotations";
DESIGN section 24).  The method is tools/bench_hoisted.py's.

HIP-event time on the ring's stream (Ring.timer_start / timer_stop), per figure a warm-up block and then the median of 5 blocks of
back-to-back calls (block length calibrated to about 0.1 s), min and max alongside; ONE PROCESS PER CASE.  64 resident ciphertexts on
four 31-bit limbs: n = 2^15 (radix-16 engine) and H5' = 20475 (general engine, phi = 8640).
  cases   {TrivGad, BaseBGad 2} x (R in {2, 8, 32} with n_out = 1; R = 8 with n_out in {ROWS, 8})
  arms    alch_ct_automorph_lincomb; the composition of existing calls on the same build -- alch_ct_automorph_hoisted without the sum
          flag, n_out R alch_buf_mul_public and n_out (R - 1) alch_buf_add -- the comparator, code the entry point does not touch
  bar     a gain (or a loss) is claimed only where the median ratio differs from 1 by more than twice the larger relative [min, max]
          spread of the two arms' blocks (DESIGN section 11's bar); otherwise the line says "within the spread"
  --ab composition   instead: the comparator alone at R = 8, n_out = 1, `--label NAME`
  --ab hoisted       instead: eight back-to-back alch_ct_automorph_hoisted calls (R = 8, per-rotation form)
          run either alternately with ALCH_LIB_PATH naming the parent commit's library to see that existing paths did not move; they
          touch no new symbol.
Lines are appended to profiles/slot_linear.jsonl (`--fresh` truncates it first)."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_hoisted import GADGETS, QS_2P, RINGS, fig, measure, primes_1_mod, spread, units  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "slot_linear.jsonl")


def kernel_rows():
    src = open(os.path.join(ROOT, "alchemy_amd", "csrc", "kernel_lincomb.hpp")).read()
    return int(re.search(r"constexpr int LINCOMB_ROWS = (\d+);", src).group(1))


def verdict(comparator, arm):
    ratio, bar = comparator[0] / arm[0], 2 * max(spread(comparator), spread(arm))
    word = "gain" if ratio - 1 > bar else "loss: call the composition there" if 1 - ratio > bar else "within the spread"
    return {"comparator_over_arm": round(ratio, 4), "bar": round(bar, 4), "verdict": word}


def one_case(a):
    import torch  # noqa: F401  (one HIP runtime per process: before the library)
    import alchemy_amd as A
    from alchemy_amd import capi
    m = RINGS[a.ring]
    qs = QS_2P if m == 1 << 16 else primes_1_mod(m, 4, 1 << 31)
    gadget, B, R, G = GADGETS[a.gadget], a.batch, a.units, a.rows
    ring = A.Ring(m, qs)
    D = ring.gadget_digits(gadget)
    js = units(m, R)
    cts = ring.alloc(2 * B)
    cts.fill_uniform(3)
    base = {"build": a.label, "library": os.path.relpath(capi.lib_path(), ROOT), "ring": a.ring, "index": m, "n": ring.n, "limbs": ring.L,
            "word_bytes": ring.word_bytes, "ciphertexts": B, "gadget": a.gadget, "digits": D, "units": R, "n_out": G}
    ks = ring.alloc(2 * D * R)
    ks.fill_uniform(2)
    aset = A.AutomorphSet(ring, js, ks, gadget)
    rot = ring.alloc(2 * B * R)
    if a.ab == "hoisted":
        t = measure(ring, lambda: [A.ct_automorph_hoisted(aset, cts, B, out=rot) for _ in range(8)])
        return {**base, "what": "(ab) eight back-to-back alch_ct_automorph_hoisted calls alone", "hoisted_x8": fig(t)}
    wts = ring.alloc(G * R)
    wts.fill_uniform(4)
    tmp, out = ring.alloc(2 * B), ring.alloc(2 * B * G)

    def composition():
        A.ct_automorph_hoisted(aset, cts, B, out=rot)
        for g in range(G):
            row = out.view(2 * B * g, 2 * B)
            for r in range(R):
                dst = row if r == 0 else tmp
                dst.mul_public(rot.view(2 * B * r, 2 * B), wts, g * R + r, 2 * B)
                if r:
                    row.add(row, tmp, 2 * B)

    if a.ab == "composition":
        tc = measure(ring, composition)
        return {**base, "what": "(ab) the composition of existing calls alone", "composition": fig(tc)}
    tl = measure(ring, lambda: A.ct_automorph_lincomb(aset, wts, cts, B, n_out=G, out=out))
    tc = measure(ring, composition)
    return {**base, "what": "alch_ct_automorph_lincomb vs hoisted + n_out R mul_public + n_out (R - 1) add", "lincomb": fig(tl),
            "composition": fig(tc), "lincomb_vs_composition": verdict(tc, tl)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--label", default="this build")
    ap.add_argument("--fresh", action="store_true")
    ap.add_argument("--ab", choices=["composition", "hoisted"])
    ap.add_argument("--ring", choices=sorted(RINGS))
    ap.add_argument("--gadget", choices=sorted(GADGETS))
    ap.add_argument("--units", type=int)
    ap.add_argument("--rows", type=int, default=1)
    a = ap.parse_args()
    if a.ring and a.gadget and a.units:                               # a child: one case, one line on stdout
        print(json.dumps(one_case(a)), flush=True)
        return
    rows = kernel_rows()
    shapes = [(8, 1)] if a.ab else [(2, 1), (8, 1), (32, 1), (8, rows), (8, 8)]
    gadgets = ["TrivGad"] if a.ab else list(GADGETS)                  # --ab: one line per engine
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w" if a.fresh else "a") as out:
        for ring in RINGS:
            for gadget in gadgets:
                for n_units, n_out in shapes:
                    cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--label", a.label, "--ring", ring,
                           "--gadget", gadget, "--units", str(n_units), "--rows", str(n_out)] + (["--ab", a.ab] if a.ab else [])
                    child = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                    if child.returncode != 0:
                        sys.stderr.write(child.stdout[-2000:] + child.stderr[-2000:])
                        raise SystemExit(f"case {ring} / {gadget} / {n_units} units / {n_out} rows ended with status {child.returncode}")
                    line = child.stdout.strip().split("\n")[-1]
                    json.loads(line)
                    print(line, flush=True)
                    print(line, file=out, flush=True)


if __name__ == "__main__":
    main()
