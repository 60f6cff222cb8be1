#!/usr/bin/env python3
"""Galois automorphisms on resident batches, measured (include/alchemy_hip.h, "Galois automorphisms").

One process, HIP-event time on the ring's stream (Ring.timer_start / timer_stop), per figure a warm-up block and then the median of
5 blocks of back-to-back calls (block length calibrated to about 0.1 s), min and max alongside.  Two rings of four 31-bit limbs with
64 resident ciphertexts (128 ring elements): n = 2^15 (radix-16 engine, closed-form gather) and H5' = 20475 (general engine, table).
  (a) alch_buf_automorph of the 128 elements against alch_buf_copy (a device-to-device copy) of the same bytes
  (b) alch_ct_automorph against the ring-to-itself identity tunnel alone -- the key switch it contains -- TrivGad and BaseBGad 2
  (c) alch_ct_automorph against the two-call composition alch_buf_automorph + alch_ct_tunnel
  (d) `--tunnel-only --label NAME` measures just the identity tunnel of (b): run it once more with ALCH_LIB_PATH naming another build
      of the library (the parent commit's) to see that the existing path did not move.  It touches no new symbol.
Lines are appended to profiles/automorph.jsonl (`--fresh` truncates it first)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import alchemy_amd as A  # noqa: E402
from alchemy_amd import capi  # noqa: E402

QS_2P = [2147352577, 2146959361, 2146041857, 2145976321]            # the four largest primes below 2^31 that are 1 mod 2^16
BLOCKS = 5


def primes_1_mod(m, count, hi):
    """The `count` largest primes below hi that are 1 mod m (trial division: 31-bit candidates)."""
    out, q = [], ((hi - 2) // m) * m + 1
    while len(out) < count:
        if q % 2 and all(q % d for d in range(3, int(q ** 0.5) + 1, 2)):
            out.append(q)
        q -= m
    return out


def measure(ring, fn):
    """(median, min, max) milliseconds per call of fn."""
    fn()
    ring.sync()
    ring.timer_start()
    for _ in range(3):
        fn()
    per = max(ring.timer_stop() / 3, 1e-3)
    reps = int(max(3, min(2000, 100.0 / per)))
    for _ in range(reps):                                            # the warm-up block
        fn()
    ring.sync()
    ms = []
    for _ in range(BLOCKS):
        ring.timer_start()
        for _ in range(reps):
            fn()
        ms.append(ring.timer_stop() / reps)
    return statistics.median(ms), min(ms), max(ms), reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tunnel-only", action="store_true")
    ap.add_argument("--label", default="this build")
    ap.add_argument("--fresh", action="store_true")
    a = ap.parse_args()
    B = a.batch
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "automorph.jsonl")
    out = open(path, "w" if a.fresh else "a")

    def emit(rec):
        rec = {"build": a.label, "library": os.path.relpath(capi.lib_path(), ROOT), **rec}
        line = json.dumps(rec)
        print(line, flush=True)
        print(line, file=out, flush=True)

    def fig(t):
        return {"ms": round(t[0], 5), "ms_min_max": [round(t[1], 5), round(t[2], 5)], "calls_per_block": t[3], "blocks": BLOCKS}

    for name, m, qs, j in (("n = 2^15", 1 << 16, QS_2P, 5), ("H5' = 20475", 20475, primes_1_mod(20475, 4, 1 << 31), 2)):
        ring = A.Ring(m, qs)
        elem_bytes = ring.n * ring.L * ring.word_bytes
        cts, perm, res = ring.alloc(2 * B), ring.alloc(2 * B), ring.alloc(2 * B)
        cts.fill_uniform(3)
        base = {"ring": name, "index": m, "n": ring.n, "limbs": ring.L, "word_bytes": ring.word_bytes, "ciphertexts": B}
        if not a.tunnel_only:
            moved = 2 * 2 * B * elem_bytes                            # read once, written once
            ta = measure(ring, lambda: A.buf_automorph(perm, cts, j))
            tc = measure(ring, lambda: perm.copy_from(cts, 2 * B))
            ts = measure(ring, lambda: perm.scale(cts, 2 * B, [1] * ring.L))   # context: an element-wise kernel of the same launch form, no gather
            emit({**base, "what": "(a) alch_buf_automorph vs device-to-device copy (context: alch_buf_scale, same bytes)", "j": j,
                  "bytes_read_plus_written": moved,
                  "automorph": {**fig(ta), "GB_per_s": round(moved / ta[0] / 1e6, 1)}, "copy": {**fig(tc), "GB_per_s": round(moved / tc[0] / 1e6, 1)},
                  "scale": {**fig(ts), "GB_per_s": round(moved / ts[0] / 1e6, 1)},
                  "automorph_over_copy": round(ta[0] / tc[0], 3), "automorph_over_scale": round(ta[0] / ts[0], 3)})
        lin = ring.upload(np.ones((1, ring.n, ring.L), dtype=np.int64))
        for gname, gadget in (("TrivGad", capi.ALCH_GAD_TRIV), ("BaseBGad 2", capi.ALCH_GAD_BASE2)):
            D = ring.gadget_digits(gadget)
            ks = ring.alloc(2 * D)
            ks.fill_uniform(2)
            tun = A.Tunnel(ring, ring, lin, ks, gadget=gadget)
            tt = measure(ring, lambda: tun.apply(cts, res, B))
            rec = {**base, "gadget": gname, "digits": D, "identity_tunnel": fig(tt)}
            if a.tunnel_only:
                emit({**rec, "what": "(d) ring-to-itself identity tunnel alone"})
            else:
                auto = A.Automorph(ring, j, ks, gadget)
                tk = measure(ring, lambda: A.ct_automorph(auto, cts, B, out=res))

                def two_calls():
                    A.buf_automorph(perm, cts, j)
                    tun.apply(perm, res, B)

                t2 = measure(ring, two_calls)
                emit({**rec, "what": "(b), (c) alch_ct_automorph vs the key switch it contains and vs the two-call composition", "j": j,
                      "ct_automorph": fig(tk), "two_calls": fig(t2), "ct_automorph_over_identity_tunnel": round(tk[0] / tt[0], 4),
                      "ct_automorph_over_two_calls": round(tk[0] / t2[0], 4)})
                auto.free()
            tun.free()
            del ks
        del cts, perm, res, lin
        ring.close()
    out.close()


if __name__ == "__main__":
    main()
