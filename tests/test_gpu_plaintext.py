"""GPU: the plaintext-side operations of E on resident batches of rings without a CRT basis (alch_pt_mul, alch_pt_linear_create /
alch_pt_eval_lin, alch_pt_rescale, alch_buf_add_bcast), bit for bit against the by-definition model (oracle/model_gen.py:
ring_mul_def, eval_lin_dec, l_def / linv_def, crt_set_dec_def), which takes any modulus.

None of the entry points exists before the feature: every test here fails on the parent commit for want of the symbols."""
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi, plaintext
from helpers import group_class_primes, lazy_group, primes_1_mod, primes_below
from oracle import model_gen as G

pytestmark = pytest.mark.gpu


def lift_ring(m, kind):
    """two31: two 31-bit primes (32-bit words; k_pt_mac one product at a time); one60: one prime just above 2^59 (64-bit words);
    three29: three primes in (2^29, 2^30) -- lazy groups of K = floor((2^32 - 1) / q) - 2 = 5 products; two20: two primes just above
    2^20 -- K = 8, the cap; class3 .. class11: the two largest primes with floor((2^32 - 1) / q) = 3 .. 11, the top of each class of
    group sizes (K = 0, 2, 3, 4, 5, 6, 7, 8, 8: the least headroom under (K + 2) q < 2^32)."""
    if kind == "two31":
        qs = primes_1_mod(m, 2, 1 << 30)
        assert all((1 << 30) < q < (1 << 31) for q in qs)
    elif kind == "one60":
        qs = primes_1_mod(m, 1, 1 << 59)
        assert qs[0] < (1 << 60)
    elif kind == "three29":
        qs = primes_1_mod(m, 3, 1 << 29)
        assert all(0xFFFFFFFF // q - 2 == 5 for q in qs)
    elif kind.startswith("class"):
        kmax = int(kind[5:])
        qs = primes_below(m, 2, 0xFFFFFFFF // kmax + 1)
        assert 3 <= kmax <= 11 and qs[0] == group_class_primes(m, kmax)[0]
        assert all(0xFFFFFFFF // q == kmax and lazy_group(q) == (min(kmax - 2, 8) if kmax >= 4 else 0) for q in qs)
    else:
        qs = primes_1_mod(m, 2, 1 << 20)
        assert all(q < (1 << 21) and 0xFFFFFFFF // q - 2 > 8 for q in qs)
    return A.Ring(m, qs)


def zp(m, p):
    return A.Ring(m, [p], nocrt=True)


def up(ring, elems):
    return ring.upload(np.asarray(elems, dtype=np.int64).reshape(len(elems), ring.n, 1))


def down(buf, count=None):
    return buf.download(0, count)[:, :, 0].tolist()


# (m, p, batch, lifting ring): radix-16 engine (32, 128), Arithmetic.hs's F4 / Zq 7, the general engine (28, 45, 91), m = 448
MUL_CASES = [(32, 2, 37, "two31"), (32, 32, 3, "one60"), (128, 4, 3, "two31"), (128, 32, 1, "one60"),
             (4, 7, 37, "two31"), (4, 7, 3, "one60"),
             (28, 32, 3, "two31"), (28, 2, 1, "one60"), (45, 7, 3, "two31"), (45, 4, 37, "one60"),
             (91, 4, 1, "two31"), (91, 32, 3, "one60"),
             (448, 32, 3, "two31"), (448, 2, 1, "two31"), (448, 32, 1, "one60"), (448, 7, 3, "one60")]


@pytest.mark.parametrize("m,p,batch,kind", MUL_CASES)
def test_pt_mul_equals_the_ring_product_by_definition(m, p, batch, kind):
    rng = random.Random(m * 1000 + p * 10 + batch)
    idx = G.Index(m)
    worst = [p // 2] * idx.n                                           # centred magnitude p/2 in every coefficient
    a = [worst] + [[rng.randrange(p) for _ in range(idx.n)] for _ in range(batch - 1)]
    b = [worst] + [[rng.randrange(p) for _ in range(idx.n)] for _ in range(batch - 1)]
    if batch > 1:
        a[1] = worst
    want = [G.ring_mul_def(x, y, idx, p) for x, y in zip(a, b)]
    lift, r = lift_ring(m, kind), zp(m, p)
    ga, gb, out = up(r, a), up(r, b), r.alloc(batch)
    A.pt_mul(lift, out, ga, gb, batch)
    assert down(out) == want
    assert down(ga) == a and down(gb) == b                             # inputs untouched
    A.pt_mul(lift, ga, ga, gb, batch)                                  # dst aliasing a
    assert down(ga) == want


# (r, s, p): the reference's first hop at real size (e = 64, d_rel = 2); d_rel > 2; r composite with a prime that e lacks
# (12 -> 20: e = 4, 28 -> 12: e = 4, d_rel = 6); shared odd primes only (45 -> 75: e = 15); e = 1 (9 -> 8: d_rel = 6);
# two-power pairs down and up; 128 -> 8: d_rel = 16, more terms than the largest lazy group of k_pt_mac (the carry between groups runs
# at K = 8 and K = 5; d_rel = 6 carries at K = 5)
LIN_CASES = [(128, 448, 32), (32, 24, 4), (12, 20, 32), (28, 12, 8), (45, 75, 4), (9, 8, 32), (128, 32, 32), (32, 128, 2), (128, 8, 4)]


def crt_set_ys(e, s, prime, e_exp, dim):
    """decToCRT's values (examples/Common.hs:65-75): crtSetDec of the prime-free parts mod the prime, taken to the Pow basis, raised
    to the prime^(e_exp - 1)-th power mod prime^e_exp (Hensel) and embedded into index s; the first dim of them."""
    mo, mbo = e, s
    while mo % prime == 0:
        mo //= prime
    while mbo % prime == 0:
        mbo //= prime
    small, big, pe = G.Index(mo), G.Index(mbo), prime ** e_exp
    out = []
    for c in G.crt_set_dec_def(small, big, prime)[:dim]:
        v = G.l_def(c, big, pe)
        for _ in range(e_exp - 1):
            w = v
            for _ in range(prime - 1):
                v = G.ring_mul_def(v, w, big, pe)
        out.append(G.embed_pow(v, big, G.Index(s)))
    assert len(out) == dim
    return out


@functools.lru_cache(maxsize=None)
def lin_case(r, s, p, batch=3):
    """(ys, inputs, expected outputs) of one pair, computed once for all lifting rings."""
    rng = random.Random(r * 1000 + s)
    e = math.gcd(r, s)
    E, R, S = G.Index(e), G.Index(r), G.Index(s)
    d_rel = R.n // E.n
    if (r, s) == (128, 448):
        ys = crt_set_ys(e, s, 2, 5, d_rel)                             # the reference's own linear function
    else:
        ys = [[rng.randrange(p) for _ in range(S.n)] for _ in range(d_rel)]
    xs = [[p // 2] * R.n] + [[rng.randrange(p) for _ in range(R.n)] for _ in range(batch - 1)]
    want = [G.eval_lin_dec(ys, G.linv_def(x, R, p), E, R, S, p) for x in xs]
    return ys, xs, want


@pytest.mark.parametrize("r,s,p", LIN_CASES)
@pytest.mark.parametrize("kind", ["two31", "one60", "three29", "two20"])
def test_pt_eval_lin_equals_the_model(r, s, p, kind):
    ys, xs, want = lin_case(r, s, p)
    batch = len(xs)
    lift, rr, rs = lift_ring(s, kind), zp(r, p), zp(s, p)
    f = A.pt_linear(lift, up(rs, ys), r)
    src, dst = up(rr, xs), rs.alloc(batch)
    A.pt_eval_lin(f, src, dst, batch)
    assert down(dst) == want
    assert down(src) == xs


@pytest.mark.parametrize("m,p,p2", [(32, 32, 16), (45, 4, 2), (9, 32, 16), (448, 32, 4)])
def test_pt_rescale_divides_and_flags(m, p, p2):
    rng = random.Random(m + p)
    n, d, batch = G.Index(m).n, p // p2, 37
    xs = [[d * rng.randrange(p2) for _ in range(n)] for _ in range(batch)]
    src, dst = up(zp(m, p), xs), zp(m, p2).alloc(batch)
    assert A.pt_rescale(src, dst, batch) is True
    assert down(dst) == [[v // d for v in x] for x in xs]
    xs[batch - 1][n - 1] += 1                                          # one coefficient of the last element is not divisible
    src = up(src.ring, xs)
    assert capi.load_library().alch_pt_rescale(src._h, dst._h, batch) == capi.ALCH_NOT_DIVISIBLE
    assert A.pt_rescale(src, dst, batch) is False
    assert down(dst) == [[v // d for v in x] for x in xs]              # floor quotients
    assert A.pt_rescale(src, dst, batch - 1) is True                   # the flag covers the range only


@pytest.mark.parametrize("m,qs,nocrt", [(45, [32], True), (9, [7], True), (64, [2147352577, 2146959361], False)])
def test_add_bcast_against_numpy(m, qs, nocrt):
    rng = np.random.default_rng(m)
    r = A.Ring(m, qs, nocrt=nocrt)
    batch = 5
    x = np.stack([np.stack([rng.integers(0, q, size=r.n, dtype=np.int64) for q in qs], axis=1) for _ in range(batch)])
    lit = np.stack([np.stack([rng.integers(0, q, size=r.n, dtype=np.int64) for q in qs], axis=1) for _ in range(3)])
    gx, gl, out = r.upload(x), r.upload(lit), r.alloc(batch)
    A.add_bcast(out, gx, gl, 2, batch)
    want = (x + lit[2][None]) % np.asarray(qs, dtype=np.int64)[None, None, :]
    assert np.array_equal(out.download(), want)
    A.add_bcast(gx, gx, gl, 0, batch - 1)                              # in place, part of the buffer
    want0 = x.copy()
    want0[:batch - 1] = (x[:batch - 1] + lit[0][None]) % np.asarray(qs, dtype=np.int64)[None, None, :]
    assert np.array_equal(gx.download(), want0)


def test_scratch_chunking_gives_the_same_words():
    """scratch_mib = 1 at n = 4096 on two limbs: a lifted element is 32 KiB, a product holds two -> 16 elements per chunk, so a
    37-batch walks three chunks; evalLin 2048 -> 4096 (d_rel = 1) holds two as well."""
    m, p, batch = 8192, 32, 37
    rng = np.random.default_rng(7)
    r, lift = zp(m, p), lift_ring(m, "two31")
    a = r.upload(rng.integers(0, p, size=(batch, r.n, 1), dtype=np.int64))
    b = r.upload(rng.integers(0, p, size=(batch, r.n, 1), dtype=np.int64))
    whole, parts = r.alloc(batch), r.alloc(batch)
    A.pt_mul(lift, whole, a, b, batch)
    ys = r.upload(rng.integers(0, p, size=(1, r.n, 1), dtype=np.int64))
    f = A.pt_linear(lift, ys, m // 2)
    half = zp(m // 2, p)
    x = half.upload(rng.integers(0, p, size=(batch, half.n, 1), dtype=np.int64))
    lin_whole, lin_parts = r.alloc(batch), r.alloc(batch)
    A.pt_eval_lin(f, x, lin_whole, batch)
    lift.set_option("scratch_mib", 1)
    assert (1 << 20) // (2 * lift.n * lift.L * lift.word_bytes) * 2 < batch          # at least three chunks
    A.pt_mul(lift, parts, a, b, batch)
    A.pt_eval_lin(f, x, lin_parts, batch)
    assert np.array_equal(parts.download(), whole.download())
    assert np.array_equal(lin_parts.download(), lin_whole.download())
    # and the unchunked words are the ring product: one element against the negacyclic convolution
    a0, b0 = a.download(0, 1)[0, :, 0], b.download(0, 1)[0, :, 0]
    full = np.convolve(a0, b0)
    neg = full[:r.n].copy()
    neg[:r.n - 1] -= full[r.n:]
    assert np.array_equal(whole.download(0, 1)[0, :, 0], neg % p)


def test_statuses():
    lib = capi.load_library()
    m, p = 448, 32
    r, lift = zp(m, p), lift_ring(m, "two31")
    a, b, out = r.alloc(4), r.alloc(4), r.alloc(4)
    a.fill_uniform(1); b.fill_uniform(2)

    def mul(lift_, d, x, y, count, flags=0):
        return lib.alch_pt_mul(lift_._h, d._h, x._h, y._h, count, flags)

    assert mul(lift, out, a, b, 4) == capi.ALCH_OK
    # lifting ring of another index / without CRT
    assert mul(lift_ring(64, "two31"), out, a, b, 4) == capi.ALCH_E_INVALID and b"index" in lib.alch_last_error()
    assert mul(A.Ring(m, [7], nocrt=True), out, a, b, 4) == capi.ALCH_E_NO_CRT
    # dst on a ring with several moduli; buffers of different plaintext rings; unknown flag
    two = A.Ring(m, [32, 7], nocrt=True)
    t = two.alloc(4)
    assert mul(lift, t, t, t, 4) == capi.ALCH_E_INVALID and b"one modulus" in lib.alch_last_error()
    assert mul(lift, out, a, zp(m, 16).alloc(4), 4) == capi.ALCH_E_INVALID
    assert mul(lift, out, a, b, 4, 1) == capi.ALCH_E_INVALID
    # Q too small for the bound: one 13-bit prime at m = 448 (bound = 192 * 2 * 16^2 = 98304 > 4481 / 2)
    small = A.Ring(m, [q for q in primes_1_mod(m, 1, 1 << 12)])
    assert small.qs[0] < (1 << 13) and plaintext.coeff_bound(m, p) == 192 * 2 * 256
    assert mul(small, out, a, b, 4) == capi.ALCH_E_INVALID and b"too small" in lib.alch_last_error()
    ys2 = r.upload(np.ones((2, r.n, 1), dtype=np.int64))
    h = C.c_void_p()
    assert lib.alch_pt_linear_create(small._h, ys2._h, 128, C.byref(h)) == capi.ALCH_E_INVALID and not h.value
    # wrong ys count (d_rel = 2 for 128 -> 448)
    assert lib.alch_pt_linear_create(lift._h, r.alloc(3)._h, 128, C.byref(h)) == capi.ALCH_E_INVALID and b"d_rel" in lib.alch_last_error()
    assert lib.alch_pt_linear_create(lift._h, r.alloc(1)._h, 128, C.byref(h)) == capi.ALCH_E_INVALID
    # wrapped ranges: a count whose byte size wraps size_t
    huge = (1 << 64) - 2
    assert mul(lift, out, a, b, huge) == capi.ALCH_E_INVALID
    assert mul(lift, out, a, b, 5) == capi.ALCH_E_INVALID
    f = A.pt_linear(lift, ys2, 128)
    src = zp(128, p).alloc(4)
    assert lib.alch_pt_eval_lin(f._h, src._h, out._h, huge, 0) == capi.ALCH_E_INVALID
    assert lib.alch_pt_eval_lin(f._h, zp(64, p).alloc(4)._h, out._h, 4, 0) == capi.ALCH_E_INVALID      # source of another index
    assert lib.alch_pt_eval_lin(f._h, src._h, zp(m, 16).alloc(4)._h, 4, 0) == capi.ALCH_E_INVALID        # another modulus
    half = zp(m, 16).alloc(4)
    assert lib.alch_pt_rescale(a._h, half._h, huge) == capi.ALCH_E_INVALID
    assert lib.alch_pt_rescale(a._h, zp(m, 7).alloc(4)._h, 4) == capi.ALCH_E_INVALID                     # 7 does not divide 32
    assert lib.alch_buf_add_bcast(out._h, a._h, b._h, 4, 4) == capi.ALCH_E_INVALID                       # index out of bounds
    assert lib.alch_buf_add_bcast(out._h, a._h, b._h, 0, huge) == capi.ALCH_E_INVALID
    # empty batches: ALCH_OK, nothing written
    out.upload(np.full((4, r.n, 1), 5, dtype=np.int64))
    assert mul(lift, out, a, b, 0) == capi.ALCH_OK
    assert lib.alch_pt_eval_lin(f._h, src._h, out._h, 0, 0) == capi.ALCH_OK
    assert lib.alch_pt_rescale(a._h, half._h, 0) == capi.ALCH_OK
    assert lib.alch_buf_add_bcast(out._h, a._h, b._h, 0, 0) == capi.ALCH_OK
    assert (out.download() == 5).all()
