"""Cost of SymmSHE (+) on resident batches with unaligned operands: HIP-event time of alch_ct_add against the same sum composed from
the entry points that existed before it, and against a device-to-device copy of the bytes the sum must move.
  (i)   aligned linear + linear                                     alch_ct_add, one launch (4 elements read, 2 written per ciphertext)
  (ii)  quadratic (k = 1, scalar) + linear (k = 0, scalar)          alch_ct_add, one launch (5 read, 3 written)
  (ii)  composed: alch_buf_scale, alch_buf_scale, alch_buf_mulg (CRT), alch_buf_add on the shared components, alch_buf_copy of c2 --
        five launches.  The composed form gets the layout that suits it: its quadratic operand is stored planar ([B] pairs (c0, c1),
        then [B] c2), so every step is ONE call over contiguous elements; on the interleaved layout of alch_ct_mul it would need a
        gather per ciphertext.  It moves 22 elements per ciphertext against 8.
  copy  alch_buf_copy of 4 (3) elements per ciphertext: the 8 (6) element moves of (ii) ((i)) as a plain copy
Shapes: n = 2^15 with 4 limbs, and H5' = F20475 (phi 8640) with 4 limbs.  Each figure is the median of 5 blocks of --reps calls after
a warm-up block.  One JSON line per shape, printed and appended to --out (default profiles/ct_add.jsonl).
Run on the GPU box:  python tests/sweeps/bench_ct_add.py [--batch N] [--reps R] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import numpy as np  # noqa: E402
import alchemy_amd as A  # noqa: E402
from alchemy_amd.capi import ALCH_BASIS_CRT  # noqa: E402
from alchemy_amd.ctadd import ct_add_raw  # noqa: E402

RLWR = [1543651201, 689270401, 718099201, 720720001, 1556755201, 1567238401]
CFG3 = [2147352577, 2146959361, 2146041857, 2145976321]                    # config 3: 31-bit primes = 1 mod 2^16


def timed(ring, fn, reps, blocks=5):
    for _ in range(reps):                                                    # warm-up block
        fn()
    out = []
    for _ in range(blocks):
        ring.timer_start()
        for _ in range(reps):
            fn()
        out.append(ring.timer_stop() / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ct_add.jsonl"))
    a = ap.parse_args()
    B = a.batch
    for name, m, qs in (("n = 2^15, 4 limbs", 1 << 16, CFG3), ("H5' (phi 8640), 4 limbs", 20475, list(reversed(RLWR[:4])))):
        ring = A.Ring(m, qs)
        s_a, s_b = [q // 3 for q in qs], [q // 5 for q in qs]
        lin_a, lin_b, quad = ring.alloc(2 * B), ring.alloc(2 * B), ring.alloc(3 * B)
        lin_a.fill_uniform(1)
        lin_b.fill_uniform(2)
        quad.fill_uniform(3)
        planar = ring.alloc(3 * B)                                           # the same quadratic ciphertexts, pairs first, then the c2
        for ct in range(B):
            planar.copy_from(quad, 2, dst_first=2 * ct, src_first=3 * ct)
            planar.copy_from(quad, 1, dst_first=2 * B + ct, src_first=3 * ct + 2)
        out1, out2 = ring.alloc(2 * B), ring.alloc(3 * B)
        t_a, t_b, out_c = ring.alloc(3 * B), ring.alloc(2 * B), ring.alloc(3 * B)
        src, dst = ring.alloc(4 * B), ring.alloc(4 * B)
        src.fill_uniform(4)

        def aligned():
            ct_add_raw(out1, B, lin_a, 1, None, 0, lin_b, 1, None, 0)

        def fused():
            ct_add_raw(out2, B, quad, 2, s_a, 0, lin_b, 1, s_b, 1)

        def composed():
            t_a.scale(planar, 3 * B, s_a)
            t_b.scale(lin_b, 2 * B, s_b)
            t_b.mulg(ALCH_BASIS_CRT, 0, 2 * B)
            out_c.add(t_a, t_b, 2 * B)
            out_c.copy_from(t_a, B, dst_first=2 * B, src_first=2 * B)

        t_i = timed(ring, aligned, a.reps)
        t_f, t_c = timed(ring, fused, a.reps), timed(ring, composed, a.reps)
        same = True
        for ct in (0, B // 2, B - 1):
            f = out2.download(3 * ct, 3)
            same = same and np.array_equal(f[:2], out_c.download(2 * ct, 2)) and np.array_equal(f[2:], out_c.download(2 * B + ct, 1))
        t_cp4 = timed(ring, lambda: dst.copy_from(src, 4 * B), a.reps)
        t_cp3 = timed(ring, lambda: dst.copy_from(src, 3 * B), a.reps)
        eb = ring.n * ring.L * ring.word_bytes
        line = json.dumps({"shape": name, "batch": B, "word_bytes": ring.word_bytes, "same_words": bool(same),
                           "aligned_lin_lin_ms": round(t_i, 3), "aligned_GBps": round(6 * B * eb / (t_i * 1e-3) / 1e9, 1),
                           "copy_6_moves_ms": round(t_cp3, 3), "aligned_over_copy": round(t_i / t_cp3, 2),
                           "quad_plus_lin_fused_ms": round(t_f, 3), "fused_GBps": round(8 * B * eb / (t_f * 1e-3) / 1e9, 1),
                           "quad_plus_lin_composed_ms": round(t_c, 3), "composed_over_fused": round(t_c / t_f, 2),
                           "copy_8_moves_ms": round(t_cp4, 3), "fused_over_copy": round(t_f / t_cp4, 2)})
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del lin_a, lin_b, quad, planar, out1, out2, t_a, t_b, out_c, src, dst


if __name__ == "__main__":
    main()
