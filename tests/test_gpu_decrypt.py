"""GPU: decrypt and error rates on device-resident ciphertext batches -- alch_ct_error_term, alch_buf_lift and alch_ct_decrypt_lift
through the ctypes binding (alchemy_amd/decrypt.py), kernels k_ct_eval_sk and k_lift (alchemy_amd/csrc/kernel_lift.hpp).

Every comparison is exact: lifts against Python integers, c(s) against the C restatement's composition (crt-basis Horner, crtInv,
lInv), the semantic cases against the model (oracle/model_gen.py: g_decrypt, lift_dec).  The one float comparison, error_rates,
allows relative 1e-12: one double rounding of an exactly computed fraction.

Before library version 1.8 the binding has none of the three symbols and the package no `decrypt` module, so this module does not
import on the parent commit and every test in it fails there."""
import random

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from alchemy_amd import decrypt as D
from helpers import assert_reduced, extreme_words, primes_1_mod, primes_below, to_aos, word32_edge_rings
from test_gpu_word64_edges import EDGE_BAL, EDGE_UNBAL

pytestmark = pytest.mark.gpu

P_SET = [2, 8, 7, 1 << 30]
P_MAX = (1 << 31) - 1                            # the largest destination modulus alch_buf_lift accepts; run by the 62- and 31-bit rows


def to_digits(x, qs):
    out = []
    for q in qs:
        out.append(x % q)
        x //= q
    return out


def prod(qs):
    Q = 1
    for q in qs:
        Q *= q
    return Q


def centred(x, Q):
    x %= Q
    return x - Q if x > (Q - 1) // 2 else x


def residues(ints, qs):
    """(count, n) integers (numpy int64 for the bulk, `special` overrides as Python integers) -> (count, n, L) int64 residues."""
    return np.stack([np.mod(ints, q) for q in qs], axis=2).astype(np.int64)


class Crafted:
    """`count` Dec-basis elements over moduli qs: small random coefficients, the six special values 0, 1, -1, (Q-1)/2, -(Q-1)/2 and
    Q-1 in every element, the +(Q-1)/2 placed at index 0, n-1 or n-3 (a lane of the last wave) in turn."""

    def __init__(self, n, qs, count, seed):
        rng = np.random.default_rng(seed)
        self.n, self.qs, self.count, self.Q = n, qs, count, prod(qs)
        Q = self.Q
        self.small = rng.integers(-1000, 1001, size=(count, n), dtype=np.int64)
        self.special = []                                              # per element: {index: integer}
        for e in range(count):
            top = [0, n - 1, n - 3][e % 3]
            free = [k for k in range(n) if k != top]
            rnd = random.Random(seed * 1000 + e)
            rnd.shuffle(free)
            vals = [0, 1, -1, (Q + 1) // 2, Q - 1]                     # (Q+1)/2 = -(Q-1)/2, Q-1 = -1 (mod Q)
            sp = {top: (Q - 1) // 2}
            for k, v in zip(free, vals):
                sp[k] = v
            self.special.append(sp)
        self.res = residues(self.small, qs)
        for e, sp in enumerate(self.special):
            for k, v in sp.items():
                self.res[e, k, :] = [v % q for q in qs]

    def lifted(self, e):
        x = [int(v) for v in self.small[e]]
        for k, v in self.special[e].items():
            x[k] = centred(v, self.Q)
        return x


def lift_ring_cases():
    cases = []
    for m in (32, 21, 420, 1 << 13):
        for L in (1, 2, 5, 8):
            cases.append((m, L, 30, True))
    for L in (1, 3):
        cases.append((1 << 12, L, 59, True))
    cases.append((256, 2, 30, True))            # n = 128: the largest ring on the wave-per-element path
    cases.append((512, 2, 30, True))            # n = 256: the smallest on the workgroup-per-element path
    cases.append((32, 4, 30, False))            # moduli of very different sizes: digits enter a limb through a full product
    cases.append((1 << 12, 3, 59, False))
    for m, L in ((1 << 12, 3), (32, 4)):        # moduli just below 2^62, the top of the accepted range: k_lift<u64> with bal 1 and 0
        cases.append((m, L, 62, True))
        cases.append((m, L, 62, False))
    cases.append((64, 2, 62, "edge_bal"))       # either side of the boundary q_i < 2 q_j that sets LiftPar::bal
    cases.append((64, 2, 62, "edge_unbal"))
    cases.append((32, 4, 31, True))             # the largest primes below 2^31: k_lift<u32> at the top of its range, bal 1 and 0
    cases.append((32, 4, 31, False))
    cases.append((420, 2, 31, True))
    cases.append((512, 2, 31, True))
    cases.append((64, 2, 31, "edge_bal31"))     # the same boundary on 4-byte words
    cases.append((64, 2, 31, "edge_unbal31"))
    cases.append((64, 2, 32, "low64"))          # the first primes above 2^31: the smallest ring that runs k_lift<u64>
    return cases


def moduli(m, L, bits, balanced):
    """bits < 62: the first primes above 2^(bits-1); bits = 62: the last ones BELOW 2^62 (nothing at or above it is accepted); bits =
    31: the last ones below 2^31 (the top of the 4-byte words).  Tags: the rings either side of q_i < 2 q_j on 8-byte words (edge_bal,
    edge_unbal) and on 4-byte words (edge_bal31, edge_unbal31: helpers.word32_edge_rings), and the first two primes above 2^31 (low64)."""
    if balanced in ("edge_bal", "edge_unbal"):
        qs = EDGE_BAL if balanced == "edge_bal" else EDGE_UNBAL
        assert all(2 * a > b for a in qs for b in qs) == (balanced == "edge_bal")
        return qs
    if balanced in ("edge_bal31", "edge_unbal31"):
        qs = word32_edge_rings(m)[balanced]
        assert len(qs) == L and max(qs) < (1 << 31) and all(2 * a > b for a in qs for b in qs) == (balanced == "edge_bal31")
        return qs
    if balanced == "low64":
        qs = primes_1_mod(m, L, 1 << 31)
        assert bits == 32 and all((1 << 31) < q < (1 << 31) + (1 << 22) for q in qs)
        return qs
    big = ((lambda count: primes_below(m, count, 1 << bits)) if bits in (31, 62)
           else (lambda count: primes_1_mod(m, count, 1 << (bits - 1))))
    if balanced:
        return big(L)
    lo = primes_1_mod(m, L - 1, 0)                                     # the smallest primes that are 1 mod m
    return [lo[0], big(1)[0]] + lo[1:]


@pytest.mark.parametrize("m,L,bits,balanced", lift_ring_cases())
def test_lift_crafted(m, L, bits, balanced):
    """alch_buf_lift alone on crafted Dec-basis elements: residues l * (x mod p) mod p for p in {2, 8, 7, 2^30}, l in {1, p-1}, and
    the digit vectors of max |x|, for count in {1, 3, 65} at element offsets first = 1 / dst_first = 2; the destination's other
    elements keep what fill_uniform wrote; once more through views."""
    qs = moduli(m, L, bits, balanced)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == (4 if bits <= 31 else 8)
    n, total = ring.n, 65
    cr = Crafted(n, qs, total, seed=m * 10 + L)
    lifted = [cr.lifted(e) for e in range(total)]
    src = ring.alloc(total + 2)
    src.fill_uniform(5)
    src.upload(cr.res, first=1)
    want_digits = [to_digits(max(abs(v) for v in x), qs) for x in lifted]
    assert all(d == to_digits((cr.Q - 1) // 2, qs) for d in want_digits)
    lifted_np = np.array(lifted, dtype=object)
    for p in P_SET + ([P_MAX] if bits in (31, 62) else []):
        zp = A.Ring(m, [p], nocrt=True)
        dst = zp.alloc(total + 3)
        for l in (1, p - 1):
            want = np.array((lifted_np * l) % p, dtype=np.int64)
            for count in (1, 3, 65):
                dst.fill_uniform(1000 + p % 97 + count)
                before = dst.download()
                digits = D.lift(src, dst, l=l, want_max=True, first=1, count=count, dst_first=2)
                got = dst.download()
                assert_reduced(got[2:2 + count], [p])
                assert np.array_equal(got[2:2 + count, :, 0], want[:count]), (m, L, p, l, count)
                assert np.array_equal(got[:2], before[:2]) and np.array_equal(got[2 + count:], before[2 + count:]), (m, L, p, l, count)
                assert digits == want_digits[:count], (m, L, p, l, count)
        # views: element 4 of the source into element 1 of the destination
        dst.fill_uniform(3)
        before = dst.download()
        digits = D.lift(src.view(5, 1), dst.view(1, 1), l=1, want_max=True)
        got = dst.download()
        assert np.array_equal(got[1, :, 0], np.array(lifted_np[4] % p, dtype=np.int64)) and digits == [want_digits[4]]
        assert np.array_equal(got[:1], before[:1]) and np.array_equal(got[2:], before[2:])
        # residues alone, digits alone
        assert D.lift(src, dst, l=1, first=1, count=3) is None
        assert np.array_equal(dst.download(0, 3)[:, :, 0], np.array(lifted_np[:3] % p, dtype=np.int64))
        del dst
    assert D.lift(src, None, want_max=True, first=1, count=3) == want_digits[:3]
    assert np.array_equal(src.download(1, total), cr.res)                 # source untouched


@pytest.mark.parametrize("m,L,bits,balanced", [(32, 3, 30, True), (420, 2, 30, True), (1 << 13, 3, 30, True), (1 << 13, 8, 30, True),
                                               (1 << 12, 3, 59, True), (32, 4, 30, False), (512, 2, 30, True),
                                               (1 << 12, 3, 62, True), (32, 4, 62, False), (64, 2, 62, "edge_bal"), (64, 2, 62, "edge_unbal"),
                                               (64, 2, 31, "edge_bal31"), (64, 2, 31, "edge_unbal31"), (64, 2, 32, "low64")])
def test_lift_maximum_position_and_sign(m, L, bits, balanced):
    """The lexicographic maximum of |x|: small random elements with ONE planted magnitude M = Q // 3 + 5 at index 0, at n - 1, at
    n - 3 (a lane of the last wave), as -M, as +M and -M together, as +M against -(M + 1) (the negative wins by one: complement and
    carry), and an element whose largest magnitude is -(q_0 q_1 ...) exactly (a carry through every low digit)."""
    qs = moduli(m, L, bits, balanced)
    ring = A.Ring(m, qs)
    n, Q = ring.n, prod(qs)
    M = Q // 3 + 5 if Q > 1000 else (Q - 1) // 2
    carry = -(Q // qs[-1]) if L > 1 else -1                           # digits (0, .., 0, 1): q_0 .. q_{L-2}
    plant = [{0: M}, {n - 1: M}, {n - 3: M}, {n - 3: -M}, {1: M, n - 2: -M}, {2: M, n - 1: -(M + 1)}, {n // 2: carry}, {}]
    rng = np.random.default_rng(m + L)
    small = rng.integers(-1, 2, size=(len(plant), n), dtype=np.int64)
    res = residues(small, qs)
    want = []
    for e, sp in enumerate(plant):
        x = [int(v) for v in small[e]]
        for k, v in sp.items():
            x[k] = v
            res[e, k, :] = [v % q for q in qs]
        want.append(to_digits(max(abs(v) for v in x), qs))
    src = ring.upload(res)
    assert D.lift(src, None, want_max=True) == want


# ---- c(s) ------------------------------------------------------------------------------------------------------------------------
def rand_elems(rng, count, n, qs):
    return np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(count)])


def oracle_ring(oracle_lib, m, qs):
    if m >= 32 and m & (m - 1) == 0:
        return oracle_lib.Ring(m // 2, qs), False
    return oracle_lib.GenRing(m, qs), True


def oracle_error_term(O, general, comps, sk, s_pre):
    """c(s) on the decoding basis from CRT-basis components: Horner in s, toLSD's scalar, crtInv, lInv."""
    acc = comps[-1]
    for c in reversed(comps[:-1]):
        acc = O.add(O.mul(acc, sk), c)
    if s_pre is not None:
        acc = O.scale(acc, s_pre)
    acc = O.crtinv(np.ascontiguousarray(acc))
    return O.linv(acc) if general else acc


ERROR_TERM_RINGS = [(32, 2, 30, 3), (64, 3, 30, 3), (45, 3, 30, 3), (420, 2, 30, 3), (11648, 5, 30, 2), (1 << 12, 2, 60, 3), (1 << 17, 2, 30, 2),
                    (1 << 12, 2, 62, 3), (420, 2, 62, 3),               # 62: just below 2^62, on extreme words
                    (1 << 12, 2, 31, 3), (420, 2, 31, 3)]               # 31: just below 2^31 (k_ct_eval_sk<u32>), on extreme words


@pytest.mark.parametrize("m,L,bits,batch", ERROR_TERM_RINGS)
def test_error_term_matches_the_oracle(oracle_lib, m, L, bits, batch):
    """alch_ct_error_term on random ciphertext words (parity does not need them valid): degree 1 and 2, with and without s_pre, CRT
    input and ALCH_POW_IN, written at an element offset of the output; equal to lInv(crtInv(Horner)) limb by limb; input untouched.
    The 62-bit and the 31-bit rows draw key, ciphertexts and scalar from the extreme residues (helpers.extreme_words, s_pre = -1)."""
    qs = moduli(m, L, bits, True)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == (4 if bits <= 31 else 8)
    O, general = oracle_ring(oracle_lib, m, qs)
    rng = np.random.default_rng(m + L)
    words = extreme_words if bits in (31, 62) else rand_elems
    sk = words(rng, 2, ring.n, qs)
    gsk = ring.upload(sk)
    for degree in (1, 2):
        per = degree + 1
        cts = words(rng, per * batch, ring.n, qs)
        for with_s_pre in (False, True):
            s_pre = [int(rng.integers(1, q)) for q in qs] if with_s_pre else None
            if with_s_pre and bits in (31, 62):
                s_pre = [q - 1 for q in qs]
            want = [oracle_error_term(O, general, [cts[per * b + c] for c in range(per)], sk[1], s_pre) for b in range(batch)]
            for flags in (0, capi.ALCH_POW_IN):
                src = np.stack([O.crtinv(np.ascontiguousarray(c)) for c in cts]) if flags else cts
                gin = ring.upload(src)
                out = ring.alloc(batch + 2)
                out.fill_uniform(77)
                before = out.download()
                D.error_term(gin, batch, gsk, degree=degree, s_pre=s_pre, flags=flags, out=out, out_first=1, sk_index=1)
                got = out.download()
                assert_reduced(got, qs)
                for b in range(batch):
                    assert np.array_equal(got[1 + b], want[b]), (m, L, degree, with_s_pre, flags, b)
                assert np.array_equal(got[0], before[0]) and np.array_equal(got[-1], before[-1])
                assert np.array_equal(gin.download(), src)
                del out, gin


@pytest.mark.parametrize("m,bits,split", [(1 << 12, 30, False), (1 << 16, 60, True), (1 << 17, 30, True)])
def test_pow_in_staging_on_resident_and_split_rings(oracle_lib, m, bits, split):
    """ALCH_POW_IN through do_decrypt's staging, the CRT copy of one chunk's input in the ring's scratch: transformed out of place,
    straight from the caller's ciphertexts, where a limb-polynomial fits one LDS-resident transform; copied and transformed in place
    on the split rings -- the smallest of them, n = 2^15 on 8-byte words and n = 2^16 on 4-byte words.  One limb, batch 2, degree 1:
    alch_ct_error_term (c(s) into the caller's buffer) and alch_ct_decrypt_lift (c(s) in the scratch, next to the staged input)
    against the C restatement and Python integers; the input is left as uploaded."""
    qs = moduli(m, 1, bits, True)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == (4 if bits <= 31 else 8)
    assert (ring.n.bit_length() - 1 > (15 if ring.word_bytes == 4 else 14)) == split        # split_ring
    O, general = oracle_ring(oracle_lib, m, qs)
    batch, q = 2, qs[0]
    rng = np.random.default_rng(m + bits)
    sk, cts = rand_elems(rng, 1, ring.n, qs), rand_elems(rng, 2 * batch, ring.n, qs)
    want = [oracle_error_term(O, general, [cts[2 * b], cts[2 * b + 1]], sk[0], None) for b in range(batch)]
    src = np.stack([O.crtinv(np.ascontiguousarray(c)) for c in cts])
    gin, gsk, out = ring.upload(src), ring.upload(sk), ring.alloc(batch)
    D.error_term(gin, batch, gsk, degree=1, flags=capi.ALCH_POW_IN, out=out)
    got = out.download()
    for b in range(batch):
        assert np.array_equal(got[b], want[b]), (m, b)
    p = primes_1_mod(m, 1, 1 << 24)[0]                  # a ring of its own for the lift: no nocrt ring exists at n = 2^16
    zp = A.Ring(m, [p])
    dst = zp.alloc(batch)
    digits = D.decrypt_lift(gin, batch, gsk, dst=dst, l=1, want_max=True, flags=capi.ALCH_POW_IN)
    low = dst.download()
    for b in range(batch):
        lifted = [centred(int(v), q) for v in want[b][:, 0]]
        assert low[b, :, 0].tolist() == [v % p for v in lifted], (m, b)
        assert digits[b] == to_digits(max(abs(v) for v in lifted), qs), (m, b)
    assert np.array_equal(gin.download(), src)


def decrypt_lift_case(oracle_lib, m, L, bits, balanced, word_bytes):
    qs = moduli(m, L, bits, balanced)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == word_bytes
    O, general = oracle_ring(oracle_lib, m, qs)
    n, batch, Q = ring.n, 3, prod(qs)
    rng = np.random.default_rng(62 + m + L)
    sk, cts = extreme_words(rng, 1, n, qs), extreme_words(rng, 2 * batch, n, qs)
    s_pre = [q - 1 for q in qs]
    coef = [Q // q * pow(Q // q, -1, q) for q in qs]
    lifted = []
    for b in range(batch):
        et = oracle_error_term(O, general, [cts[2 * b], cts[2 * b + 1]], sk[0], s_pre)
        lifted.append([centred(sum(int(r) * c for r, c in zip(row, coef)), Q) for row in et])
    gin, gsk = ring.upload(cts), ring.upload(sk)
    for p in (P_MAX, 8):
        zp = A.Ring(m, [p], nocrt=True)
        dst = zp.alloc(batch)
        digits = D.decrypt_lift(gin, batch, gsk, s_pre=s_pre, dst=dst, l=p - 1, want_max=True)
        got = dst.download()
        assert_reduced(got, [p])
        for b in range(batch):
            assert got[b, :, 0].tolist() == [v * (p - 1) % p for v in lifted[b]], (p, b)
            assert digits[b] == to_digits(max(abs(v) for v in lifted[b]), qs), (p, b)
        del dst
    assert np.array_equal(gin.download(), cts)


@pytest.mark.parametrize("m,L,balanced", [(1 << 12, 3, True), (32, 4, False), (64, 2, "edge_bal"), (64, 2, "edge_unbal")])
def test_decrypt_lift_moduli_below_2_62(oracle_lib, m, L, balanced):
    """alch_ct_decrypt_lift (k_ct_eval_sk<u64>, then k_lift<u64> with bal 1 and 0) on extreme words, s_pre = -1, at the top of the
    accepted modulus range: residues modulo 2^31 - 1 (the largest destination modulus) and modulo 8 and the digit vectors of max |x|
    against the oracle's c(s) lifted in Python integers."""
    decrypt_lift_case(oracle_lib, m, L, 62, balanced, 8)


@pytest.mark.parametrize("m,L,balanced", [(1 << 12, 3, True), (32, 4, False), (64, 2, "edge_bal31"), (64, 2, "edge_unbal31")])
def test_decrypt_lift_moduli_below_2_31(oracle_lib, m, L, balanced):
    """The 4-byte twin: k_ct_eval_sk<u32>, then k_lift<u32> with bal 1 and 0, on the largest primes below 2^31 and on the two rings
    either side of q_i < 2 q_j."""
    decrypt_lift_case(oracle_lib, m, L, 31, balanced, 4)


# ---- semantic cases ----------------------------------------------------------------------------------------------------------------
def model_cases(m, mp, p, seed):
    """Valid model instances over three limbs: a fresh encryption, one product (degree 2, k = 1), and the product after
    keySwitchQuadCirc and modSwitch down (linear, MSD, two limbs)."""
    from oracle import model_gen as G
    rng = random.Random(seed)
    small, big = G.Index(m), G.Index(mp)
    qs = primes_1_mod(mp, 4, 1 << 29)
    sk = G.g_gen_sk(big, rng)
    pa = [rng.randrange(p) for _ in range(small.n)]
    pb = [rng.randrange(p) for _ in range(small.n)]
    ca, cb = G.g_encrypt(sk, pa, small, big, p, qs[1:], rng), G.g_encrypt(sk, pb, small, big, p, qs[1:], rng)
    prod_ct = G.g_ct_mul(ca, cb)
    hint = G.g_ks_hint(sk, big, qs, rng)
    switched = G.g_mod_switch_down(G.g_key_switch(hint, G.g_mod_switch_up(prod_ct, qs[:1])), 1)
    assert len(switched.qs) == 3 and len(switched.c) == 2
    return G, sk, [("fresh", ca), ("product", prod_ct), ("switched", switched)]


@pytest.mark.parametrize("m,mp,p", [(16, 64, 8), (9, 45, 4), (9, 45, 7)])
def test_decrypt_and_error_rates_of_model_ciphertexts(m, mp, p):
    """decrypt_batch equals the model's g_decrypt coefficient for coefficient; the digit vectors of alch_ct_decrypt_lift equal
    max |lift_dec(c(s))| exactly and error_rates equals it over Q to one double rounding -- for a fresh encryption, a product
    (degree 2, k = 1) and the product after key switch and modSwitch, on a two-power and on a composite index, three limbs,
    CRT-basis input and ALCH_POW_IN."""
    G, sk, cases = model_cases(m, mp, p, seed=m * 100 + mp + p)
    zp_big, zp_small = A.Ring(mp, [p], nocrt=True), A.Ring(m, [p], nocrt=True)
    for name, ct in cases:
        lsd = G.g_to_lsd(ct)
        qs, Q = ct.qs, prod(ct.qs)
        ring = A.Ring(mp, qs)
        s_pre = None if ct.enc == G.LSD else [p % q for q in qs]
        degree = len(ct.c) - 1
        batch = 3                                                        # the ciphertext three times over, in a larger buffer
        host = np.stack([to_aos(c) for c in ct.c] * batch)
        gsk = ring.upload(np.stack([to_aos([[v % q for v in sk] for q in qs])]))
        gsk.crt()
        # the model's view: c(s) of the LSD form, lifted on the decoding basis
        acc = [[0] * ct.big.n for _ in qs]
        for comp in reversed(lsd.c):
            acc = [[(u + v) % q for u, v in zip(G.ring_mul_def(al, sk, ct.big, q), cl)] for al, cl, q in zip(acc, comp, qs)]
        worst = max(abs(v) for v in G.lift_dec(acc, ct.big, qs))
        want_pt = G.g_decrypt(sk, ct)
        for flags in (capi.ALCH_POW_IN, 0):
            gin = ring.upload(host)
            if not flags:
                gin.crt()
            pt = D.decrypt_batch(gin, batch, gsk, zp_big, zp_small, lsd.k, lsd.l, degree=degree, s_pre=s_pre, flags=flags)
            got = pt.download(0, batch)
            for b in range(batch):
                assert got[b, :, 0].tolist() == want_pt, (name, flags, b)
            digits = D.decrypt_lift(gin, batch, gsk, degree=degree, s_pre=s_pre, want_max=True, flags=flags)
            assert digits == [to_digits(worst, qs)] * batch, (name, flags)
            assert [D.digits_to_int(d, qs) for d in digits] == [worst] * batch
            rates = D.error_rates(gin, batch, gsk, degree=degree, s_pre=s_pre, flags=flags)
            assert all(abs(r - worst / Q) <= 1e-12 * (worst / Q) for r in rates), (name, flags, rates, worst / Q)
            # the two-step form gives the same: error_term, then lift
            et = D.error_term(gin, batch, gsk, degree=degree, s_pre=s_pre, flags=flags)
            assert D.lift(et, None, want_max=True, count=batch) == digits
            del pt, et, gin


def test_decrypt_batch_reports_a_failed_divg():
    """g does not divide modulo p when p shares a factor with the odd radical: the library's ALCH_NOT_DIVISIBLE status is raised."""
    mp, p = 45, 3
    qs = primes_1_mod(mp, 2, 1 << 29)
    ring, zp = A.Ring(mp, qs), A.Ring(mp, [p], nocrt=True)
    cts, sk = ring.alloc(2), ring.alloc(1)
    cts.fill_uniform(1)
    sk.fill_uniform(2)
    with pytest.raises(A.AlchemyError) as ei:
        D.decrypt_batch(cts, 1, sk, zp, zp, 1, 1)
    assert ei.value.code == capi.ALCH_NOT_DIVISIBLE


# ---- edges -----------------------------------------------------------------------------------------------------------------------
def test_edges_and_statuses():
    lib = capi.load_library()
    assert lib.alch_version() == (1 << 16) | 8
    qs = primes_1_mod(64, 2, 1 << 29)
    ring, other, r32 = A.Ring(64, qs), A.Ring(64, qs[:1]), A.Ring(32, primes_1_mod(32, 2, 1 << 29))
    zp, zp32, zint = A.Ring(64, [8], nocrt=True), A.Ring(32, [8], nocrt=True), A.Ring(64, [0], nocrt=True)
    zp2 = A.Ring(64, [8, 7], nocrt=True)
    cts, sk, out = ring.alloc(6), ring.alloc(1), ring.alloc(3)
    for b in (cts, sk, out):
        b.fill_uniform(9)
    dst, dst32, dint, dst2 = zp.alloc(3), zp32.alloc(3), zint.alloc(3), zp2.alloc(3)
    dst.fill_uniform(4)
    before_out, before_dst = out.download(), dst.download()

    def status(fn, *args):
        rc = fn(*args)
        return rc, lib.alch_last_error().decode()

    et, lf, dl = lib.alch_ct_error_term, lib.alch_buf_lift, lib.alch_ct_decrypt_lift
    # batch 0 / count 0: success, nothing written
    assert et(cts._h, 0, 1, sk._h, 0, None, out._h, 0, 0) == 0
    assert lf(out._h, 0, 0, dst._h, 0, 1, None) == 0
    assert dl(cts._h, 0, 1, sk._h, 0, None, dst._h, 0, 1, None, 0) == 0
    # both outputs null: success, nothing done
    assert lf(out._h, 0, 3, None, 0, 1, None) == 0
    assert dl(cts._h, 3, 1, sk._h, 0, None, None, 0, 1, None, 0) == 0
    assert np.array_equal(out.download(), before_out) and np.array_equal(dst.download(), before_dst)
    bad = [
        (et, (cts._h, 2, 3, sk._h, 0, None, out._h, 0, 0)),                      # degree 3
        (et, (cts._h, 2, 0, sk._h, 0, None, out._h, 0, 0)),                      # degree 0
        (et, (cts._h, 4, 1, sk._h, 0, None, out._h, 0, 0)),                      # 8 elements wanted of 6
        (et, (cts._h, 2, 1, sk._h, 1, None, out._h, 0, 0)),                      # key index
        (et, (cts._h, 2, 1, sk._h, 0, None, out._h, 2, 0)),                      # output range
        (et, (cts._h, 2, 1, sk._h, 0, None, other.alloc(3)._h, 0, 0)),           # output on another ring
        (et, (cts._h, 2, 1, r32.alloc(1)._h, 0, None, out._h, 0, 0)),            # key on another ring
        (et, (cts._h, 2, 1, sk._h, 0, None, out._h, 0, 2)),                      # ALCH_POW_OUT is not a flag of this call
        (et, (cts._h, 2, 1, sk._h, 0, None, cts._h, 0, 0)),                      # output over the input
        (lf, (out._h, 2, 2, dst._h, 0, 1, None)),                                # source range
        (lf, (out._h, 0, 3, dst._h, 1, 1, None)),                                # destination range
        (lf, (out._h, 0, 3, dst32._h, 0, 1, None)),                              # destination index
        (lf, (out._h, 0, 3, dst2._h, 0, 1, None)),                               # two destination moduli
        (dl, (cts._h, 2, 3, sk._h, 0, None, dst._h, 0, 1, None, 0)),
        (dl, (cts._h, 2, 1, sk._h, 0, None, dst32._h, 0, 1, None, 0)),
        (dl, (cts._h, 3, 1, sk._h, 0, None, dst._h, 1, 1, None, 0)),
    ]
    for fn, args in bad:
        rc, msg = status(fn, *args)
        assert rc == capi.ALCH_E_INVALID and msg, (fn.__name__, args, rc, msg)
    for fn, args in [(lf, (out._h, 0, 3, dint._h, 0, 1, None)), (dl, (cts._h, 3, 1, sk._h, 0, None, dint._h, 0, 1, None, 0))]:
        rc, msg = status(fn, *args)
        assert rc == capi.ALCH_E_UNSUPPORTED and msg, (fn.__name__, rc, msg)
    # a ring without CRT basis cannot hold ciphertexts
    rc, msg = status(et, dst._h, 1, 1, dst._h, 0, None, dst._h, 2, 0)
    assert rc == capi.ALCH_E_NO_CRT and msg
    assert np.array_equal(out.download(), before_out) and np.array_equal(dst.download(), before_dst)
