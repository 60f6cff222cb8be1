"""Shared helpers for the test-suite: layout conversions between the fixtures (limb-major lists), the C
oracle / C ABI host layout (numpy int64, shape (n, L), Lol's tuple-interleaved order) and SHA-256 digests."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def to_aos(elem):
    """limb-major [L][n] python ints -> (n, L) int64 (host layout)."""
    return np.ascontiguousarray(np.array(elem, dtype=np.int64).T)


def from_aos(arr):
    return np.asarray(arr).T.tolist()


def digest_limb_major(*aos_arrays):
    h = hashlib.sha256()
    for a in aos_arrays:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.int64).T).tobytes())
    return h.hexdigest()


def hint_to_crt_aos(ring_oracle, hint_pow):
    """fixture hint [[h0_i, h1_i]] (Pow basis, limb-major) -> list of 2*D CRT-basis (n, L) arrays in the
    order the C ABI wants: h0_0, h1_0, h0_1, h1_1, ..."""
    out = []
    for h0, h1 in hint_pow:
        out.append(ring_oracle.crt(to_aos(h0)))
        out.append(ring_oracle.crt(to_aos(h1)))
    return out


def oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, hint_crt, a0, a1, b0, b1, s_pre=None, pow_out=False, gadget="triv"):
    """PT2CT's whole mul_ (PT2CT.hs:172-177) composed from the C restatement's primitives:
    modSwitch (keySwitchQuadCirc hint (modSwitch (a * b))) with operands on the last l_in limbs of qs_h, the hint on
    all of qs_h and the result on the last l_out limbs.  Operands / hint / result in the CRT basis ((n, L) int64),
    result in the Pow basis with pow_out.  Pinned to the exact model by tests/golden/full_mul_small.json."""
    L = len(qs_h)
    dup = L - l_in
    o_in, o_h = oracle_lib.Ring(n, qs_h[dup:]), oracle_lib.Ring(n, qs_h)
    s = list(s_pre) if s_pre is not None else [1] * l_in
    # (*) and the encoding scalars
    c = [o_in.mul(a0, b0), o_in.add(o_in.mul(a0, b1), o_in.mul(a1, b0)), o_in.mul(a1, b1)]
    c = [o_in.scale(x, s) for x in c]
    # modSwitch up: Rescale b -> (a, b):  x -> (0, q_a x)
    mult = 1
    for q in qs_h[:dup]:
        mult *= q
    up = []
    for x in c:
        scaled = o_in.scale(x, [mult % q for q in qs_h[dup:]])
        up.append(np.ascontiguousarray(np.concatenate([np.zeros((n, dup), dtype=np.int64), scaled], axis=1)))
    # keySwitchQuadCirc: [c0, c1] + sum_i crt(reduce d_i) * hint_i
    digs = o_h.decompose_triv(o_h.crtinv(up[2])) if gadget == "triv" else o_h.decompose_base2(o_h.crtinv(up[2]))
    assert 2 * len(digs) == len(hint_crt)
    ks = [up[0], up[1]]
    for i, d in enumerate(digs):
        dc = o_h.crt(d)
        ks[0] = o_h.add(ks[0], o_h.mul(dc, hint_crt[2 * i]))
        ks[1] = o_h.add(ks[1], o_h.mul(dc, hint_crt[2 * i + 1]))
    # modSwitch down: Rescale (a, b) -> b in the Pow basis, outermost limb first
    out = []
    for x in ks:
        cur = o_h.crtinv(x)
        for k in range(L, l_out, -1):
            cur = oracle_lib.Ring(n, qs_h[L - k:]).rescale_drop0(cur)
        out.append(cur if pow_out else oracle_lib.Ring(n, qs_h[L - l_out:]).crt(cur))
    return out[0], out[1]


def oracle_full_mul_base2_down(oracle_lib, n, qs_in, l_h, l_out, hint_crt, a0, a1, b0, b1, s_pre=None, pow_out=False, m=None):
    """PT2CT's whole mul_ with a BaseBGad 2 hint on FEWER limbs than the operands (PT2CT.hs:140,164), from the C restatement's
    primitives: (*) on the operands' ring qs_in (mulG on a general index m), modSwitch DOWN of the quadratic ciphertext to the last l_h
    limbs (rescaleDec on c0, rescalePow on c1 and c2), BaseBGad 2 decomposition of c2, hint products, modSwitch down to l_out limbs."""
    L = len(qs_in)
    ring = (lambda qs: oracle_lib.GenRing(m, qs)) if m else (lambda qs: oracle_lib.Ring(n, qs))
    o_in, o_h, o_out = ring(qs_in), ring(qs_in[L - l_h:]), ring(qs_in[L - l_out:])
    s = list(s_pre) if s_pre is not None else [1] * L
    c = [o_in.mul(a0, b0), o_in.add(o_in.mul(a0, b1), o_in.mul(a1, b0)), o_in.mul(a1, b1)]
    c = [o_in.scale(o_in.mulg_crt(x) if m else x, s) for x in c]

    def down(x_pow, l_from, l_to, dec):
        cur = ring(qs_in[L - l_from:]).linv(x_pow) if dec else x_pow
        for k in range(l_from, l_to, -1):
            cur = ring(qs_in[L - k:]).rescale_drop0(cur)
        return ring(qs_in[L - l_to:]).l(cur) if dec else cur

    dec0 = bool(m)                                   # two-power index: the decoding basis is the powerful basis
    low = [down(o_in.crtinv(x), L, l_h, dec0 and comp == 0) for comp, x in enumerate(c)]
    digs = decompose_base2(low[2], qs_in[L - l_h:]) if m else o_h.decompose_base2(low[2])
    assert 2 * len(digs) == len(hint_crt)
    ks = [o_h.crt(low[0]), o_h.crt(low[1])]
    for i, d in enumerate(digs):
        dc = o_h.crt(d)
        ks[0] = o_h.add(ks[0], o_h.mul(dc, hint_crt[2 * i]))
        ks[1] = o_h.add(ks[1], o_h.mul(dc, hint_crt[2 * i + 1]))
    out = []
    for comp, x in enumerate(ks):
        cur = down(o_h.crtinv(x), l_h, l_out, dec0 and comp == 0)
        out.append(cur if pow_out else o_out.crt(cur))
    return out[0], out[1]


def oracle_mul_relin_base2(oracle_lib, n, qs, hint_crt, a0, a1, b0, b1, s_pre=None, pow_out=False):
    """keySwitchQuadCirc hint (a * b) with a BaseBGad 2 hint, composed from the C restatement's primitives
    (CRT-basis operands and hint).  Pinned to the exact model by tests/golden/mul_relin_base2_small.json."""
    o = oracle_lib.Ring(n, qs)
    s = list(s_pre) if s_pre is not None else [1] * len(qs)
    c0 = o.scale(o.mul(a0, b0), s)
    c1 = o.scale(o.add(o.mul(a0, b1), o.mul(a1, b0)), s)
    c2 = o.scale(o.mul(a1, b1), s)
    digs = o.decompose_base2(o.crtinv(c2))
    assert 2 * len(digs) == len(hint_crt)
    for i, d in enumerate(digs):
        dc = o.crt(d)
        c0 = o.add(c0, o.mul(dc, hint_crt[2 * i]))
        c1 = o.add(c1, o.mul(dc, hint_crt[2 * i + 1]))
    return (o.crtinv(c0), o.crtinv(c1)) if pow_out else (c0, c1)


def primes_1_mod(m, count, lo=0):
    """The first `count` primes q > lo with q = 1 (mod m)."""
    from oracle.model import is_prime
    out, q = [], (lo // m) * m + 1
    while len(out) < count:
        if q > max(lo, 2) and is_prime(q):
            out.append(q)
        q += m
    return out


def primes_below(m, count, hi):
    """The `count` largest primes q < hi with q = 1 (mod m), largest first: the mirror of primes_1_mod."""
    from oracle.model import is_prime
    out, q = [], ((hi - 2) // m) * m + 1
    while len(out) < count:
        assert q > 2, "fewer than `count` such primes"
        if is_prime(q):
            out.append(q)
        q -= m
    return out


def worst_residues(q):
    """0, 1, -2, -1 and the two residues next to q / 2: where a missing or doubled conditional subtraction shows."""
    return [0, 1, q - 2, q - 1, (q - 1) // 2, (q + 1) // 2]


def centred_extremes(q):
    """Centred: 0, 1, -1, the largest positive value, the most negative one, the second largest."""
    return [0, 1, q - 1, (q - 1) // 2, (q + 1) // 2, (q - 3) // 2]


def extreme_words(rng, count, n, qs, extremes=worst_residues):
    """(count, n, L) int64: per word one of the six residues extremes(q) (3 in 4) or a uniform one (1 in 4).  Every value is a
    residue below q, so int64 holds it for any q < 2^63; nothing is added or multiplied in int64."""
    limbs = []
    for q in qs:
        ext = np.array(extremes(q), dtype=np.int64)
        assert ext.shape == (6,) and int(ext.min()) >= 0 and int(ext.max()) < q
        pick = rng.integers(0, 8, size=(count, n))
        fill = rng.integers(0, q, size=(count, n), dtype=np.int64)
        limbs.append(np.where(pick < 6, ext[np.minimum(pick, 5)], fill))
    return np.ascontiguousarray(np.stack(limbs, axis=2))


def centred_extreme_words(rng, count, n, qs):
    """extreme_words on the ends of the centred range (the digits of a TrivGad decomposition)."""
    return extreme_words(rng, count, n, qs, extremes=centred_extremes)


def carve(ring, host, *spans):
    """(parent, [views]): one device buffer holding `host` ((count, n, L) int64) and one alch_buf_view of it per span (first, count)
    -- the operands of one overlap case (tests/test_gpu_overlap_contract.py): adjacent, coinciding or shifted ranges of one parent."""
    parent = ring.upload(host)
    return parent, [parent.view(first, count) for first, count in spans]


def assert_parent_unchanged(parent, host, written=()):
    """Every element of `parent` outside the `written` spans (first, count) still holds the uploaded words; returns the download."""
    got = parent.download()
    keep = np.ones(len(host), dtype=bool)
    for first, count in written:
        keep[first:first + count] = False
    assert got.shape == np.asarray(host).shape
    assert np.array_equal(got[keep], np.asarray(host)[keep]), "words outside the written range changed"
    return got


class Gapped:
    """Operand and result placement of one sweep case (tests/sweeps/fuzz_parity.py, fuzz_parity_gen.py): with `on`, every operand and
    the result are views in the interior of parents of their own, `margin` uniform elements before and `margin` + `tail` behind
    (tail: what a kernel's rounded-up last tile could reach), and check() asserts every word outside the result range as uploaded
    (tests/test_gpu_footprint.py's rule); without, plain buffers, as the sweeps always had."""

    def __init__(self, on, nprng, margin=3, tail=16):
        self.on, self.nprng, self.margin, self.tail, self.parents = on, nprng, margin, tail, []

    def _fill(self, ring, count):
        return np.ascontiguousarray(np.stack([self.nprng.integers(0, q, size=(count, ring.n), dtype=np.int64) for q in ring.qs], axis=2))

    def _place(self, ring, host, count, written):
        before, behind = self._fill(ring, self.margin), self._fill(ring, self.margin + self.tail)
        whole = np.concatenate([before, host if host is not None else self._fill(ring, count), behind])
        parent = ring.upload(whole)
        self.parents.append((parent, whole, [(self.margin, count)] if written else []))
        return parent.view(self.margin, count)

    def operand(self, ring, host):
        return self._place(ring, np.asarray(host), len(host), False) if self.on else ring.upload(host)

    def result(self, ring, count):
        return self._place(ring, None, count, True) if self.on else ring.alloc(count)

    def check(self):
        for parent, whole, written in self.parents:
            assert_parent_unchanged(parent, whole, written)


def assert_reduced(got, qs):
    """Every stored word of a (..., L) result lies in [0, q_j)."""
    got = np.asarray(got)
    assert got.shape[-1] == len(qs)
    assert int(got.min()) >= 0, "a stored word is negative as int64 (at or above 2^63)"
    for j, q in enumerate(qs):
        assert int(got[..., j].max()) < q, f"limb {j}: a stored word is not below its modulus"


def oracle_full_mul_general(oracle_lib, m, qs_h, l_in, l_out, hint_crt, a0, a1, b0, b1, s_pre=None, pow_out=False):
    """PT2CT's whole mul_ on a GENERAL cyclotomic index, composed from the general C restatement's primitives:
    (*) with mulG on every product coefficient (Eval.hs:65-67), modSwitch up, keySwitchQuadCirc (Eval.hs:133),
    modSwitch down with rescaleDec on c0 and rescalePow on c1 (Eval.hs:130).  Same layout rules as oracle_full_mul."""
    L = len(qs_h)
    dup = L - l_in
    o_in, o_h = oracle_lib.GenRing(m, qs_h[dup:]), oracle_lib.GenRing(m, qs_h)
    n = o_h.n
    s = list(s_pre) if s_pre is not None else [1] * l_in
    c = [o_in.mul(a0, b0), o_in.add(o_in.mul(a0, b1), o_in.mul(a1, b0)), o_in.mul(a1, b1)]
    c = [o_in.scale(o_in.mulg_crt(x), s) for x in c]
    mult = 1
    for q in qs_h[:dup]:
        mult *= q
    up = []
    for x in c:
        scaled = o_in.scale(x, [mult % q for q in qs_h[dup:]])
        up.append(np.ascontiguousarray(np.concatenate([np.zeros((n, dup), dtype=np.int64), scaled], axis=1)))
    digs = o_h.decompose_triv(o_h.crtinv(up[2]))
    ks = [up[0], up[1]]
    for i, d in enumerate(digs):
        dc = o_h.crt(d)
        ks[0] = o_h.add(ks[0], o_h.mul(dc, hint_crt[2 * i]))
        ks[1] = o_h.add(ks[1], o_h.mul(dc, hint_crt[2 * i + 1]))
    out = []
    for comp, x in enumerate(ks):
        cur = o_h.crtinv(x)
        if comp == 0:
            cur = o_h.linv(cur)                                   # c0: rescaleDec
        for k in range(L, l_out, -1):
            cur = oracle_lib.GenRing(m, qs_h[L - k:]).rescale_drop0(cur)
        o_out = oracle_lib.GenRing(m, qs_h[L - l_out:])
        if comp == 0:
            cur = o_out.l(cur)
        out.append(cur if pow_out else o_out.crt(cur))
    return out[0], out[1]


def decompose_base2(elem, qs):
    """BaseBGad 2 decompose + reduce of one Pow-basis element ((n, L) residues), index-agnostic: per limb i the centred lift is
    split into ceil(log2 q_i) balanced binary digits (remainder 1 taken as -1, the top digit absorbs the rest), limb 0's digits
    first; every digit is returned reduced into all limbs.  Checked against the C restatement (cref.Ring.decompose_base2) in
    tests/test_oracle_general.py."""
    out = []
    qv = np.array(qs, dtype=np.int64)
    for i, q in enumerate(qs):
        v = elem[:, i].astype(np.int64)
        v = np.where(v > (q - 1) // 2, v - q, v)
        kd = (q - 1).bit_length()
        for t in range(kd):
            if t + 1 < kd:
                d = -(v & 1)
                v = (v - d) // 2
            else:
                d = v
            out.append(np.ascontiguousarray(np.mod(d[:, None], qv[None, :])))
    return out


def oracle_tunnel(oracle_lib, r_p, s_p, qs, lin_crt, ks_crt, c0, c1, s_pre=None, pow_out=False, gadget="triv"):
    """SymmSHE.tunnel (Eval.hs:134) on one linear ciphertext (k = 0), composed from the general C restatement's primitives and
    the model's index maps -- following the definition literally: full lInv on R', Tensor `coeffs`, l on every E'-coefficient,
    embedPow into S', crt, times f'(d_i); for c1: `coeffs` on the Pow basis, embedPow, gadget decompose (TrivGad or BaseBGad 2,
    D digits), crt, hint products.
    c0, c1: CRT basis over R' ((n_r, L)); lin_crt: d_rel CRT elements of S'; ks_crt: [(i * D + t) * 2 + {0: b, 1: a}]."""
    import math
    from oracle import model_gen as G
    e_p = math.gcd(r_p, s_p)
    ie, ir, isx = G.Index(e_p), G.Index(r_p), G.Index(s_p)
    Or, Os, Oe = oracle_lib.GenRing(r_p, qs), oracle_lib.GenRing(s_p, qs), oracle_lib.GenRing(e_p, qs)
    L = len(qs)
    s = list(s_pre) if s_pre is not None else [1] * L
    c0p, c1p = Or.scale(Or.crtinv(c0), s), Or.scale(Or.crtinv(c1), s)
    c0d = Or.linv(c0p)
    rows, emb = np.array(G.coeffs_indices(ie, ir)), np.array(G.embed_indices(ie, isx))
    acc0, acc1 = np.zeros((isx.n, L), dtype=np.int64), np.zeros((isx.n, L), dtype=np.int64)
    for i, row in enumerate(rows):
        x = np.zeros((isx.n, L), dtype=np.int64)
        x[emb] = Oe.l(np.ascontiguousarray(c0d[row]))
        acc0 = Os.add(acc0, Os.mul(Os.crt(x), lin_crt[i]))
        x1 = np.zeros((isx.n, L), dtype=np.int64)
        x1[emb] = c1p[row]
        digs = Os.decompose_triv(x1) if gadget == "triv" else decompose_base2(x1, qs)
        for t, d in enumerate(digs):
            dc = Os.crt(d)
            acc0 = Os.add(acc0, Os.mul(dc, ks_crt[(i * len(digs) + t) * 2]))
            acc1 = Os.add(acc1, Os.mul(dc, ks_crt[(i * len(digs) + t) * 2 + 1]))
    return (Os.crtinv(acc0), Os.crtinv(acc1)) if pow_out else (acc0, acc1)


# ---- 32-bit words: the moduli at which a lazy 64-bit sum changes its group size ------------------------------------------------------
DENSE_LEVEL2_BELOW = 715827882                  # 2^32 / 6: below it six products stay under q 2^32 (dense_row level 2)
DENSE_LEVEL1_BELOW = 1753413056                 # 2^32 / sqrt(6): below it six products stay under 2^64 (level 1)


def lazy_group(q):
    """Products per 64-bit group of the 32-bit inner-product kernels (k_tunnel_mac_e, k_tun2_mac, k_pt_mac), from the documented
    bound alone: the largest K <= 8 with (K + 2) q < 2^32, and 0 (one product at a time) where not even two fit."""
    k = min(8, ((1 << 32) - 1) // q - 2)
    assert k < 2 or (k + 2) * q < (1 << 32) and (k == 8 or (k + 3) * q >= (1 << 32))
    return k if k >= 2 else 0


def group_class_primes(m, kmax):
    """(top, bottom): the largest and the smallest prime q = 1 (mod m) with (2^32 - 1) // q == kmax.  The top of a class has the
    least headroom under (K + 2) q < 2^32; the bottom is the first modulus that gets one product more."""
    top = primes_below(m, 1, ((1 << 32) - 1) // kmax + 1)[0]
    bottom = primes_1_mod(m, 1, ((1 << 32) - 1) // (kmax + 1))[0]
    assert ((1 << 32) - 1) // top == kmax == ((1 << 32) - 1) // bottom, (m, kmax, top, bottom)
    return top, bottom


def level_edge_primes(m):
    """Primes q = 1 (mod m) next to the constants that choose the variant of dense_row (general-index CRT_p / DFT_p passes):
    'below2' / 'above2': the two largest below 2^32 / 6 (largest first) and the two smallest at or above it; 'below1' / 'above1':
    the same at 2^32 / sqrt(6); 'top': the two largest below 2^31."""
    return {"below2": primes_below(m, 2, DENSE_LEVEL2_BELOW), "above2": primes_1_mod(m, 2, DENSE_LEVEL2_BELOW - 1),
            "below1": primes_below(m, 2, DENSE_LEVEL1_BELOW), "above1": primes_1_mod(m, 2, DENSE_LEVEL1_BELOW - 1),
            "top": primes_below(m, 2, 1 << 31)}


def dense_level(qs):
    """The dense_row variant a 32-bit general-index ring with these moduli runs: the least level over its limbs."""
    return min(2 if q < DENSE_LEVEL2_BELOW else 1 if q < DENSE_LEVEL1_BELOW else 0 for q in qs)


def threshold_moduli(rng, m, count):
    """`count` distinct primes = 1 (mod m) below 2^31 from both ends of every group-size class and from the level edges: the modulus
    draw of the sweeps (rng: random.Random)."""
    pool = {q for kmax in range(2, 12) for q in group_class_primes(m, kmax)} | {q for v in level_edge_primes(m).values() for q in v}
    return rng.sample(sorted(q for q in pool if q < (1 << 31)), count)


def word32_edge_rings(m):
    """Two-limb rings of primes = 1 (mod m) at the dispatch boundaries of the 4-byte two-power kernels: the first primes above 2^30
    (the smallest ring that is not q30), one limb on each side of 2^30, and for the largest prime below 2^31 and below 2^30 the
    partner just above and just at or below (qmax - 1) / 2 (balanced / not).  The rings of tests/test_gpu_word32_edges.py for
    m = 2^16; the modulus class the sweeps draw from."""
    top30, above30 = primes_below(m, 1, 1 << 30)[0], primes_1_mod(m, 2, 1 << 30)
    out = {"above30": above30, "straddle30": [top30, above30[0]]}
    for bits, qmax in ((31, primes_below(m, 1, 1 << 31)[0]), (30, top30)):
        half = (qmax - 1) // 2
        out[f"edge_bal{bits}"] = [qmax, primes_1_mod(m, 1, half)[0]]
        out[f"edge_unbal{bits}"] = [qmax, primes_below(m, 1, half + 1)[0]]
    return out


def resident_edge_rings(m):
    """The nine rings of tests/test_gpu_resident_edges.py for primes = 1 (mod m): the two largest primes below 2^31 and below 2^62, the
    first two above 2^31 (the smallest that take 8-byte words), the largest 31-bit / 62-bit prime next to a 17-bit one and a 21-bit /
    32-bit one, and for either top prime the partner just above and just below (qmax - 1) / 2 (balanced / not; the 62-bit pair by the
    rule of tests/test_gpu_word64_edges.py).  The modulus class the resident-batch sweeps draw from."""
    e32 = word32_edge_rings(m)
    top31, top62, low64 = primes_below(m, 2, 1 << 31), primes_below(m, 2, 1 << 62), primes_1_mod(m, 2, 1 << 31)
    q17, half = primes_1_mod(m, 1, 1 << 16)[0], (top62[0] - 1) // 2
    return {"TOP31": top31, "MIX31": [top31[0], q17, primes_1_mod(m, 1, 1 << 20)[0]],
            "EDGE_BAL31": e32["edge_bal31"], "EDGE_UNBAL31": e32["edge_unbal31"],
            "LOW64": low64, "TOP62": top62, "MIX64": [top62[0], q17, low64[0]],
            "EDGE_BAL62": [top62[0], primes_1_mod(m, 1, half)[0]], "EDGE_UNBAL62": [top62[0], primes_below(m, 1, half)[0]]}


RESIDENT_WORD_BYTES = {"TOP31": 4, "MIX31": 4, "EDGE_BAL31": 4, "EDGE_UNBAL31": 4, "LOW64": 8, "TOP62": 8, "MIX64": 8, "EDGE_BAL62": 8,
                       "EDGE_UNBAL62": 8}


def draw_resident_edge_ring(rnd, m):
    """("edge:NAME", moduli): one of resident_edge_rings(m) at random -- the draw of the ext, encrypt and hint sweeps (rnd: random.Random)."""
    name = rnd.choice(sorted(RESIDENT_WORD_BYTES))
    return "edge:" + name, resident_edge_rings(m)[name]


def check_resident_edge_rings(rings):
    """What the cases of tests/test_gpu_resident_edges.py need of resident_edge_rings(m), on the moduli alone: the word size every ring
    must get, (qmax - 1) / 2 < qmin exactly on the BAL rings, q_i < 2 q_j for all i, j (LiftPar::bal) on exactly the same, the TOP primes
    within 2^22 of their power of two, the small limbs of 17, 21 and 32 bits."""
    assert set(rings) == set(RESIDENT_WORD_BYTES)
    for name, qs in rings.items():
        assert len(set(qs)) == len(qs) and (8 if max(qs) >= (1 << 31) else 4) == RESIDENT_WORD_BYTES[name], name
        assert max(qs) < ((1 << 31) if RESIDENT_WORD_BYTES[name] == 4 else (1 << 62)), name
        balanced = (max(qs) - 1) // 2 < min(qs)
        assert balanced == (not name.startswith(("EDGE_UNBAL", "MIX"))), name
        assert all(2 * a > b for a in qs for b in qs) == balanced, name
    assert all((1 << 31) - (1 << 22) < q < (1 << 31) for q in rings["TOP31"])
    assert all((1 << 62) - (1 << 22) < q < (1 << 62) for q in rings["TOP62"])
    assert all((1 << 31) < q < (1 << 31) + (1 << 22) for q in rings["LOW64"])
    assert [(q - 1).bit_length() for q in rings["MIX31"]] == [31, 17, 21] and [(q - 1).bit_length() for q in rings["MIX64"]] == [62, 17, 32]
    for bits in (31, 62):
        bal, unbal = rings[f"EDGE_BAL{bits}"], rings[f"EDGE_UNBAL{bits}"]
        top = rings[f"TOP{bits}"][0]
        assert bal[0] == unbal[0] == top and unbal[1] <= (top - 1) // 2 < bal[1] and bal[1] - unbal[1] < 1 << (22 if bits == 31 else 32)


def tunnel_worst_operands(oracle_lib, rp, sp, qs, batch, plus, check_digits):
    """The worst case of a tunnel's hint inner product on 32-bit words, as operands(rng, d_rel, D, n_r, n_s) -> (lin, ks, cts) (D: digits
    per E'-coefficient; the kernel sums d_rel D products per slot).  lin, c0 and the odd ciphertexts: extreme words.  Hint rows:
    extreme words in the upper half of the slots, q-1 in the lower half.  c1 of the even ciphertexts: crt of the element whose every
    E'-coefficient is the constant -1 (+1 with plus: s_pre = -1 turns it round) -- the Pow-basis word at position rows[i][0] of
    every row of coeffs_indices, zero elsewhere.  Every TrivGad digit of it is then the constant -1, whose CRT image is q-1 in every
    slot: with the lower half of the hint the kernel sums D products (q-1)^2.  check_digits: assert exactly that with the oracle,
    following oracle_tunnel's own steps."""
    import math
    from oracle import model_gen as G
    e_p = math.gcd(rp, sp)
    ie, ir, isx = G.Index(e_p), G.Index(rp), G.Index(sp)
    rows, emb = np.array(G.coeffs_indices(ie, ir)), np.array(G.embed_indices(ie, isx))
    L = len(qs)
    qv = np.array(qs, dtype=np.int64)

    def make(rng, d_rel, D, n_r, n_s):
        assert (n_r, n_s) == (ir.n, isx.n) and rows.shape == (d_rel, ie.n)
        Or, Os = oracle_lib.GenRing(rp, qs), oracle_lib.GenRing(sp, qs)
        lin, ks = extreme_words(rng, d_rel, n_s, qs), extreme_words(rng, 2 * d_rel * D, n_s, qs)
        ks[:, :n_s // 2, :] = qv - 1
        cts = extreme_words(rng, 2 * batch, n_r, qs)
        x = np.zeros((n_r, L), dtype=np.int64)
        x[rows[:, 0], :] = 1 if plus else qv - 1
        worst = Or.crt(x)
        for ct in range(0, batch, 2):
            cts[2 * ct + 1] = worst
        if check_digits:
            assert D == L                                         # TrivGad: one digit per limb and E'-coefficient
            c1p = Or.scale(Or.crtinv(worst), [q - 1 for q in qs] if plus else [1] * L)
            for row in rows:
                x1 = np.zeros((n_s, L), dtype=np.int64)
                x1[emb] = c1p[row]
                digs = Os.decompose_triv(x1)
                assert len(digs) == L
                for d in digs:
                    assert np.array_equal(Os.crt(d), np.broadcast_to(qv - 1, (n_s, L))), "a digit's CRT image is not q-1 everywhere"
        return lin, ks, cts

    return make
