"""Time of hint generation on resident buffers (alchemy_amd/hints.py over alch_buf_gauss_dec, l / crt and alch_ct_ks_hint).
  * ks_quad_circ_hint at n = 2^15 with the four config-3 moduli, TrivGad and BaseBGad 2;
  * the five tunnel_hints of the HomomRLWR hops H_k' -> H_k+1' at the limb counts PT2CT gives them (TrivGad; the linear functions are
    seeded words: the time does not depend on their values);
  * the element-wise pass alch_ct_ks_hint alone on the BaseBGad 2 hint of 8 values at n = 2^15 (992 entries), as bytes read and
    written per second, next to a device-to-device copy of its output on the same footing (bytes read plus bytes written).
Every figure is the minimum HIP-event time of --reps calls after one warm-up call; the rings of a shape share one stream, so the event
pair covers the whole sequence.  One JSON line per figure, appended by the caller to profiles/bench_hints.jsonl; nothing is asserted.
Run on the GPU machine:  python tests/sweeps/bench_hints.py [--reps R]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: F401,E402  (one HIP runtime per process: before the library)
import alchemy_amd as A  # noqa: E402
from alchemy_amd import capi, ringround  # noqa: E402
from alchemy_amd import encrypt as E  # noqa: E402
from alchemy_amd import hints as H  # noqa: E402

CFG3 = [2147352577, 2146959361, 2146041857, 2145976321]
GADGETS = (("TrivGad", capi.ALCH_GAD_TRIV), ("BaseBGad 2", capi.ALCH_GAD_BASE2))


def best_ms(ring, reps, call):
    call()                                                                   # warm-up: scratch, pools, tables
    best = 1e30
    for _ in range(reps):
        ring.timer_start()
        keep = call()
        best = min(best, ring.timer_stop())
        del keep
    return round(best, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    m = 1 << 16
    ring = A.Ring(m, CFG3)
    svar = 5.0 / math.sqrt(ring.n)
    sk = E.gen_sk(ring, svar, 1)
    for name, gadget in GADGETS:
        ms = best_ms(ring, a.reps, lambda: H.ks_quad_circ_hint(ring, gadget, sk, svar, 7))
        print(json.dumps({"what": "ks_quad_circ_hint", "ring": "n = 2^15, 4 limbs", "gadget": name, "entries": ring.gadget_digits(gadget),
                          "ms": ms}), flush=True)
    # the pass alone
    gadget, n_v = capi.ALCH_GAD_BASE2, 8
    total = n_v * ring.gadget_digits(gadget)
    v, err, out, other = ring.alloc(n_v), ring.alloc(total), ring.alloc(2 * total), ring.alloc(2 * total)
    v.fill_uniform(2)
    err.fill_uniform(3)
    elem = ring.n * ring.L * ring.word_bytes
    ms = best_ms(ring, a.reps, lambda: H.ct_ks_hint(out, gadget, n_v, v, err, sk, 11))
    moved = 3 * total * elem                                                 # err read, (b, a) written; v and the key stay in cache
    ms_copy = best_ms(ring, a.reps, lambda: other.copy_from(out, 2 * total))
    print(json.dumps({"what": "alch_ct_ks_hint", "ring": "n = 2^15, 4 limbs", "gadget": "BaseBGad 2", "entries": total, "ms": ms,
                      "bytes_read_and_written": moved, "GB_per_s": round(moved / ms / 1e6, 1),
                      "d2d_copy_of_the_output": {"ms": ms_copy, "bytes_read_and_written": 4 * total * elem,
                                                 "GB_per_s": round(4 * total * elem / ms_copy / 1e6, 1)}}), flush=True)
    del v, err, out, other
    # the five hops of HomomRLWR
    p, tuns = 0, []
    for _ in range(4):
        _, _, _, p = capi.select_limbs(ringround.QS, p, capi.ALCH_OP_MUL)
    for _ in range(5):
        lin_, lh, lout, p = capi.select_limbs(ringround.QS, p, capi.ALCH_OP_TUNNEL)
        tuns.append(lh)
    tuns.reverse()
    all_ms = 0.0
    for k in range(5):
        qs = ringround.moduli(tuns[k])
        rr, rs = A.Ring(ringround.HP[k], qs), A.Ring(ringround.HP[k + 1], qs)
        rr.share_stream(rs)
        _, d_rel = A.Tunnel.info(rr, rs)
        lin = rs.alloc(d_rel)
        lin.fill_uniform(100 + k)
        sk_in = E.gen_sk(rr, 5.0 / math.sqrt(rr.n), 20 + k)
        sk_out = E.gen_sk(rs, 5.0 / math.sqrt(rs.n), 21 + k)
        svar_s = 5.0 / math.sqrt(rs.n)
        ms = best_ms(rs, a.reps, lambda: H.tunnel_hint(rr, rs, capi.ALCH_GAD_TRIV, lin, sk_out, sk_in, svar_s, 30 + k))
        all_ms += ms
        print(json.dumps({"what": "tunnel_hint", "hop": f"H{k}' -> H{k + 1}'", "indices": [ringround.HP[k], ringround.HP[k + 1]],
                          "limbs": tuns[k], "d_rel": d_rel, "gadget": "TrivGad", "ms": ms}), flush=True)
    print(json.dumps({"what": "tunnel_hint, five hops", "ms": round(all_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
