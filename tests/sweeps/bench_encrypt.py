"""Time of SymmSHE encrypt on a resident plaintext batch (alchemy_amd.encrypt_batch: embed, lInv, alch_buf_gauss_dec, l, crt,
alch_ct_encrypt) next to the per-ciphertext host path it replaces and to a device-to-device copy of the bytes it writes.
Rings: n = 2^15 with the four config-3 moduli (plaintext index 128), and H5' = F20475 (phi 8640) with four HomomRLWR moduli
(plaintext index H5 = 4095); p = 32; 8192 plaintexts (--batch).  All rings of a shape share one stream, so the HIP-event time of the
ciphertext ring covers the whole sequence, allocations of the intermediates included.
The yardstick is the host path of the binding on the same machine, per ciphertext: a numpy Gaussian with the same correlation, `l` over
the integers and `crt` through the host-buffer Tensor calls, c1 and c0 on the host, one upload -- timed on --host-cts ciphertexts.
One JSON line per ring; no figure is asserted anywhere.
Run on the GPU machine:  python tests/sweeps/bench_encrypt.py [--batch N] [--reps R] [--host-cts K]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import alchemy_amd as A  # noqa: E402
import gauss_model as GM  # noqa: E402
from alchemy_amd import encrypt as E  # noqa: E402

RLWR = [1543651201, 689270401, 718099201, 720720001, 1556755201, 1567238401]
CFG3 = [2147352577, 2146959361, 2146041857, 2145976321]


def host_encrypt_one(ring, zint, zp_small, zp_big, sk_host_crt, pt, p, svar, rng, out, b):
    """One ciphertext the way the per-ciphertext host path makes it (host-buffer Tensor calls, one upload of two elements)."""
    m, n = ring.m, ring.n
    coset = zp_big.linv(zp_small.embed_pow(zp_big, pt))[:, 0]
    _, _, axes = GM.plan(m, svar * p * p)
    rad = 1
    for q, _ in GM.factor(m):
        rad *= q
    x = rng.normal(0.0, math.sqrt(svar * p * p * (m // rad) / (2.0 * math.pi)), size=(1, n))
    for q, mp, stride, Lc in axes:
        h = q - 1
        X = x.reshape(1, n // (h * mp * stride), h, mp * stride)
        x = np.einsum("ik,abkc->abic", np.array(Lc), X).reshape(1, n)
    c = np.where(coset > (p - 1) // 2, coset - p, coset)
    z = c + p * np.rint((x[0] - c) / p).astype(np.int64)
    e_pow = zint.l(z.reshape(n, 1))[:, 0] if zint is not None else z       # l is the identity on a two-power index
    e = ring.crt(np.stack([np.mod(e_pow, q) for q in ring.qs], axis=1))
    c1 = np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in ring.qs], axis=1)
    c0 = ring.sub(e, ring.mul(c1, sk_host_crt))
    out.upload(np.stack([c0, c1]), 2 * b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cts", type=int, default=4)
    a = ap.parse_args()
    p = 32
    for name, m_pt, m, qs in (("n = 2^15, 4 limbs", 128, 1 << 16, CFG3), ("H5' (phi 8640), 4 limbs", 4095, 20475, list(reversed(RLWR[:4])))):
        ring, zp_small, zp_big = A.Ring(m, qs), A.Ring(m_pt, [p], nocrt=True), A.Ring(m, [p], nocrt=True)
        zp_small.share_stream(ring)
        zp_big.share_stream(ring)
        B, svar = a.batch, 5.0 / math.sqrt(ring.n)
        pt = zp_small.alloc(B)
        pt.fill_uniform(3)
        sk = E.gen_sk(ring, svar, 1)
        out = {"ring": name, "batch": B, "word_bytes": ring.word_bytes, "output_bytes": 2 * B * ring.L * ring.n * ring.word_bytes}
        cts = E.encrypt_batch(ring, sk, pt, zp_small, zp_big, svar, 7)                  # warm-up: scratch, pools
        best = 1e30
        for rep in range(a.reps):
            del cts
            ring.timer_start()
            cts = E.encrypt_batch(ring, sk, pt, zp_small, zp_big, svar, 8 + rep)
            best = min(best, ring.timer_stop())
        out["encrypt_batch"] = {"ms": round(best, 3), "ciphertexts_per_s": round(B / best * 1e3, 1)}
        other = ring.alloc(2 * B)
        other.copy_from(cts, 2 * B)
        best = 1e30
        for _ in range(a.reps):
            ring.timer_start()
            other.copy_from(cts, 2 * B)
            best = min(best, ring.timer_stop())
        out["d2d_copy_of_the_output"] = {"ms": round(best, 3)}
        zint, rng = (A.Ring(m, [0], nocrt=True) if m & (m - 1) else None), np.random.default_rng(5)
        skh = sk.download()[0]
        pth = pt.download(0, a.host_cts)
        host_out = ring.alloc(2 * a.host_cts)
        host_encrypt_one(ring, zint, zp_small, zp_big, skh, pth[0], p, svar, rng, host_out, 0)   # warm-up
        t0 = time.perf_counter()
        for b in range(a.host_cts):
            host_encrypt_one(ring, zint, zp_small, zp_big, skh, pth[b], p, svar, rng, host_out, b)
        ring.sync()
        out["per_ciphertext_host_path_ciphertexts_per_s"] = round(a.host_cts / (time.perf_counter() - t0), 1)
        print(json.dumps(out), flush=True)
        del cts, other, pt, sk, host_out


if __name__ == "__main__":
    main()
