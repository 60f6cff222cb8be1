#!/usr/bin/env python3
"""BASELINE config 5 at the reference's real parameters: the ring tunnels of examples/Tunnel.hs -- BaseBGad 2 hints (:24), its five
~30-bit moduli (:34-39), the hops of examples/Common.hs:78-95 over H0' .. H5' -- as `modSwitch . tunnel hint . modSwitch` (PT2CT.hs:224-229)
on a batch of ciphertexts resident in HBM
(`bench_tunnel.py twopower ...`: tunnels between two-power rings instead, see twopower_mode).  Limb counts from alch_select_limbs with the BaseBGad rule (KSPNoise (BaseBGad 2) = p + KSAccumPNoise,
PT2CT.hs:140), resolved backwards from the output pNoise 0 for the five-hop chain.  Synthetic residues and hints.  One JSON line per hop."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import alchemy_amd as A
from alchemy_amd import capi


def twopower_mode(argv):
    """`bench_tunnel.py twopower [batch] [rp:sp ...]`: tunnels between TWO-POWER rings (alchemy_amd/tunnelhops_pow2.py), six limbs on the
    hint's ring, 32-bit moduli of examples/Tunnel.hs's size, BaseBGad 2 and TrivGad; default hops 2^16 -> 2^17 and 2^17 -> 2^16.  Per hop:
    warm-up, then the median of 5 blocks of back-to-back runs between HIP events; algorithmic bytes = one linear ciphertext in, one out,
    8-byte words; fraction_of_8TBps = those bytes per second over the 8 TB/s of HBM.  Last line: the same build's composed key switch
    (alch_ct_mul_relin, TrivGad) on the largest target ring, as context."""
    import statistics
    from alchemy_amd.tunnelhops_pow2 import TwoPowerHop, tunnel_sized_moduli
    nums = [a for a in argv if a.isdigit()]
    B = int(nums[0]) if nums else 64
    pairs = [tuple(int(x) for x in a.split(":")) for a in argv if ":" in a] or [(1 << 16, 1 << 17), (1 << 17, 1 << 16)]
    L, blocks = 6, 5
    for rp, sp in pairs:
        for gname, gadget in (("BaseBGad 2", capi.ALCH_GAD_BASE2), ("TrivGad", capi.ALCH_GAD_TRIV)):
            hop = TwoPowerHop(rp, sp, B, l_hint=L, gadget=gadget)
            hop.measure(1)                                                   # warm-up: scratch allocation, code objects
            reps = max(1, min(20, 2048 // B))
            rates = [hop.measure(reps)[0] for _ in range(blocks)]
            rate = statistics.median(rates)
            nbytes = hop.algorithmic_bytes()
            print(json.dumps({"hop": f"2^{rp.bit_length() - 1} -> 2^{sp.bit_length() - 1}", "indices": [rp, sp], "limbs_in_hint_out": [hop.lin, hop.lh, hop.lout],
                              "d_rel": hop.d_rel, "gadget": gname, "digits_per_coefficient": hop.D, "batch": B, "runs_per_block": reps, "blocks": blocks,
                              "tunnels_per_s": rate, "tunnels_per_s_min_max": [min(rates), max(rates)], "algorithmic_bytes_per_tunnel": nbytes,
                              "fraction_of_8TBps": rate * nbytes / 8e12}), flush=True)
            del hop
    m = max(sp for _, sp in pairs)
    ring = A.Ring(m, tunnel_sized_moduli(L))
    hint_src, a, b, out = ring.alloc(2 * L), ring.alloc(2 * B), ring.alloc(2 * B), ring.alloc(2 * B)
    hint_src.fill_uniform(2); a.fill_uniform(3); b.fill_uniform(4)
    hint = ring.hint_from_buf(hint_src)
    ring.ct_mul_relin(hint, a, b, out, B); ring.sync()
    rates = []
    for _ in range(blocks):
        ring.timer_start()
        for _ in range(4):
            ring.ct_mul_relin(hint, a, b, out, B)
        rates.append(4 * B / (ring.timer_stop() * 1e-3))
    print(json.dumps({"context": "composed key switch on the target ring (alch_ct_mul_relin, TrivGad)", "index": m, "limbs": L, "batch": B,
                      "ops_per_s": statistics.median(rates), "ops_per_s_min_max": [min(rates), max(rates)]}), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "twopower":
    twopower_mode(sys.argv[2:])
    sys.exit(0)

QS = [537264001, 539884801, 555609601, 560851201, 566092801]          # examples/Tunnel.hs:34-39, Zqs order
HP = [11648, 29120, 43680, 54600, 27300, 20475]
B = int(sys.argv[1]) if len(sys.argv) > 1 and "=" not in sys.argv[1] else 2048
OPTS = [(a.split("=")[0], int(a.split("=")[1])) for a in sys.argv[1:] if "=" in a]        # launch options, e.g. tunnel_mac=0

_rings = {}
def ring(m, L):
    if (m, L) not in _rings:
        _rings[(m, L)] = A.Ring(m, list(reversed(QS[:L])))
        for k_, v_ in OPTS:
            _rings[(m, L)].set_option(k_, v_)
    return _rings[(m, L)]

p, tuns = 0, []
for _ in range(5):
    lin, lh, lout, p = capi.select_limbs(QS, p, capi.ALCH_OP_TUNNEL, capi.ALCH_GAD_BASE2)
    tuns.append((lin, lh, lout))
tuns.reverse()
for k, (lin, lh, lout) in enumerate(tuns):
    rin, rr, rs, ro = ring(HP[k], lin), ring(HP[k], lh), ring(HP[k + 1], lh), ring(HP[k + 1], lout)
    _, d_rel = A.Tunnel.info(rr, rs)
    D = rs.gadget_digits(capi.ALCH_GAD_BASE2)
    lin_buf, ks = rs.alloc(d_rel), rs.alloc(2 * d_rel * D)
    lin_buf.fill_uniform(1); ks.fill_uniform(2)
    tun = A.Tunnel(rr, rs, lin_buf, ks, gadget=capi.ALCH_GAD_BASE2)
    x, up, mid, out = rin.alloc(2 * B), rr.alloc(2 * B), rs.alloc(2 * B), ro.alloc(2 * B)
    x.fill_uniform(3)

    def hop():
        src = x
        if lh != lin:                        # BaseBGad hints can sit on FEWER limbs than the input: modSwitch goes either way
            capi.ct_mod_switch(x, up, B); src = up
        tun.apply(src, mid, B)
        if lout != lh:
            capi.ct_mod_switch(mid, out, B)

    hop(); rs.sync()
    rs.timer_start(); hop(); ms = rs.timer_stop()
    print(json.dumps({"hop": f"H{k}' -> H{k+1}'", "indices": [HP[k], HP[k + 1]], "limbs_in_hint_out": [lin, lh, lout], "d_rel": d_rel,
                      "gadget": "BaseBGad 2", "digits_per_coefficient": D, "digit_transforms_per_ciphertext": d_rel * D * lh,
                      "batch": B, "tunnels_per_s": B / (ms * 1e-3)}), flush=True)
    del tun, x, up, mid, out, lin_buf, ks
