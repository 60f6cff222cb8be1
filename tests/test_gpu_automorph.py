"""GPU: Galois automorphisms on resident batches (include/alchemy_hip.h, "Galois automorphisms"; kernel_automorph.hpp).

alch_buf_automorph against the permutation restated from the header's slot rule (tests/automorph_model.py) on both engines, both word
sizes and both store forms; its algebra; its footprint, overlap rule and statuses; alch_ct_automorph bit for bit against the
composition it is defined by (alch_buf_automorph, then the ring-to-itself alch_ct_tunnel with lin_crt = crt(1)); the whole flow
gen_sk -> automorph_hint -> encrypt -> ct_automorph -> decrypt against sigma_j of the plaintext in Python integers; one case with the
source produced behind a loaded stream.  Every comparison is exact."""
import math
import os
import random
import re

import numpy as np
import pytest

import alchemy_amd as A
import automorph_model as M
from alchemy_amd import capi
from alchemy_amd import encrypt as E
from conftest import ROOT
from helpers import assert_parent_unchanged, assert_reduced, carve, primes_1_mod, primes_below
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

TRIV, BASE2, POW2_4 = capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2, capi.ALCH_GAD_BASEPOW2(4)
KEY = bytes(range(32))


def moduli(m, kind):
    if kind == "top31":                                          # two 31-bit limbs: 4-byte words
        return primes_below(m, 2, 1 << 31)
    if kind == "top62":                                          # one prime just below 2^62: 8-byte words
        return primes_below(m, 1, 1 << 62)
    if kind == "mix64":                                          # 62 + 17 + 32 bits
        qs = [primes_below(m, 1, 1 << 62)[0], primes_1_mod(m, 1, 1 << 16)[0], primes_1_mod(m, 1, 1 << 31)[0]]
        assert [(q - 1).bit_length() for q in qs] == [62, 17, 32]
        return qs
    if kind == "p29":                                            # three 29-bit limbs: room for a key switch's noise
        return primes_1_mod(m, 3, 1 << 28)
    raise AssertionError(kind)


def uniform(rng, count, n, qs):
    return np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2))


def position_coded(n, qs):
    """word k of limb j is (k + 1 + j) mod q_j: all words of a limb differ (n < q), so no wrong permutation can coincide."""
    assert all(n + len(qs) < q for q in qs)
    return np.ascontiguousarray(np.stack([(np.arange(n, dtype=np.int64) + 1 + j) % q for j, q in enumerate(qs)], axis=1))


def seeded_unit(m, seed):
    rnd = random.Random(seed)
    while True:
        j = rnd.randrange(2, m)
        if math.gcd(j, m) == 1:
            return j


_TABLES = {}


def table(m, j):
    key = (m, j % m)
    if key not in _TABLES:
        _TABLES[key] = np.array(M.table(m, j % m), dtype=np.int64)
    return _TABLES[key]


def apply_model(host, m, j):
    """sigma_j on (count, n, L) CRT-basis words: destination slot k takes source slot table[k], in every limb."""
    return np.ascontiguousarray(np.asarray(host)[:, table(m, j), :])


# ---- 1. the permutation ----------------------------------------------------------------------------------------------------------
TWO_POWER = [(32, "top31"), (32, "top62"), (32, "mix64"), (1 << 12, "top31"), (1 << 12, "top62"), (1 << 12, "mix64"),
             (1 << 16, "top31"), (1 << 16, "top62"),             # n = 2^15: the split size of 8-byte words
             (1 << 17, "top31")]                                 # n = 2^16: the split size of 4-byte words
GENERAL = [(9, "top31"), (9, "top62"), (9, "mix64"),             # n = 6: the one-word form
           (45, "top31"), (45, "top62"), (45, "mix64"),          # n = 24: 16-byte packs
           (21, "top31"), (121, "top31"), (11648, "top31"), (11648, "top62")]


@pytest.mark.parametrize("m,kind", TWO_POWER + GENERAL, ids=lambda v: str(v))
def test_buf_automorph_equals_the_model(m, kind):
    qs = moduli(m, kind)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == (4 if kind == "top31" else 8) and ring.n == M.phi(m)
    pow2 = m >= 32 and m & (m - 1) == 0
    js = [3, 5, m - 1, seeded_unit(m, m)] if pow2 else [j for j in (2, m - 1, seeded_unit(m, m)) if math.gcd(j, m) == 1][:2]
    assert len(js) >= 2
    rng = np.random.default_rng(m)
    host = uniform(rng, 3, ring.n, qs)
    host[1] = position_coded(ring.n, qs)
    src, dst = ring.upload(host), ring.alloc(3)
    for j in js:
        dst.fill_uniform(j)
        A.buf_automorph(dst, src, j)
        got = dst.download()
        assert np.array_equal(got, apply_model(host, m, j)), (m, kind, j)
    assert np.array_equal(src.download(), host)
    # j is reduced mod m
    A.buf_automorph(dst, src, js[0])
    first = dst.download()
    dst.fill_uniform(99)
    _check_raw(ring, dst, 0, src, 0, 3, js[0] + 3 * m, capi.ALCH_OK)
    assert np.array_equal(dst.download(), first)


def _check_raw(ring, dst, df, src, sf, count, j, want):
    lib = capi.load_library()
    rc = lib.alch_buf_automorph(dst._h, df, src._h, sf, count, j)
    assert rc == want, (rc, lib.alch_last_error())
    return lib.alch_last_error().decode()


def grid_cap_lanes():
    """The element-wise grid of the library: ew_grid caps the workgroups, each of 256 lanes."""
    src = open(os.path.join(ROOT, "alchemy_amd", "csrc", "alchemy_hip.hip")).read()
    body = re.search(r"static inline unsigned ew_grid\(size_t items\) \{(.*?)\n\}", src, flags=re.S).group(1)
    cap = re.search(r"if \(g > (\d+)\) g = \1;", body)
    assert cap and "(items + 255) / 256" in body
    return int(cap.group(1)) * 256


def test_buf_automorph_past_the_grid():
    """n = 2^15, one limb: a lane owns four words, 8192 lanes per element; 66 elements are more lanes than the grid holds, with a
    ragged last round, so the grid-stride loop wraps."""
    m, count = 1 << 16, 66
    cap = grid_cap_lanes()
    lanes = count * (m // 2) // 4
    assert cap == 2048 * 256 and cap < lanes < 2 * cap and lanes % cap
    qs = primes_1_mod(m, 1, 1 << 29)
    ring = A.Ring(m, qs)
    host = uniform(np.random.default_rng(66), count, ring.n, qs)
    host[count - 1] = position_coded(ring.n, qs)
    src, dst = ring.upload(host), ring.alloc(count)
    dst.fill_uniform(1)
    A.buf_automorph(dst, src, 5)
    assert np.array_equal(dst.download(), apply_model(host, m, 5))


# ---- 2. algebra --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [45, 1 << 12])
def test_group_law_copy_and_ring_homomorphism(m):
    qs = moduli(m, "top31")
    ring = A.Ring(m, qs)
    rng = np.random.default_rng(7 + m)
    ha, hb = uniform(rng, 2, ring.n, qs), uniform(rng, 2, ring.n, qs)
    a, b = ring.upload(ha), ring.upload(hb)
    t1, t2, t3 = ring.alloc(2), ring.alloc(2), ring.alloc(2)
    j1, j2 = seeded_unit(m, 1), seeded_unit(m, 2)
    A.buf_automorph(t1, a, j2)
    A.buf_automorph(t2, t1, j1)                                  # sigma_j1 (sigma_j2 a)
    A.buf_automorph(t3, a, j1 * j2)
    assert np.array_equal(t2.download(), t3.download())
    A.buf_automorph(t1, a, 1)
    assert np.array_equal(t1.download(), ha)                     # sigma_1 is a copy
    # sigma_j (a . b) = sigma_j a . sigma_j b
    prod = ring.alloc(2)
    prod.mul(a, b, 2)
    A.buf_automorph(t1, prod, j1)
    A.buf_automorph(t2, a, j1)
    A.buf_automorph(t3, b, j1)
    t2.mul(t2, t3, 2)
    assert np.array_equal(t1.download(), t2.download())


@pytest.mark.parametrize("m", [32, 64])
def test_on_the_powerful_basis_it_is_the_substitution(m):
    """crtInv . sigma_j . crt is X -> X^j with X^n = -1, in Python integers."""
    qs = moduli(m, "top31")
    ring = A.Ring(m, qs)
    n = ring.n
    host = uniform(np.random.default_rng(m), 1, n, qs)
    for j in M.units(m):
        buf, out = ring.upload(host), ring.alloc(1)
        buf.crt()
        A.buf_automorph(out, buf, j)
        out.crtinv()
        got = out.download()[0]
        for l, q in enumerate(qs):
            assert got[:, l].tolist() == M.sigma_pow_twopower([int(x) for x in host[0, :, l]], j, q), (m, j, l)


@pytest.mark.parametrize("ms,mb", [(9, 45), (32, 64)])
def test_commutes_with_embed(ms, mb):
    qs = moduli(mb, "top31")
    small, big = A.Ring(ms, qs), A.Ring(mb, qs)
    host = uniform(np.random.default_rng(mb), 2, small.n, qs)
    x = small.upload(host)
    for j in (seeded_unit(mb, 5), mb - 1):
        ex, left = big.alloc(2), big.alloc(2)
        ex.embed_from(x, 2, capi.ALCH_BASIS_CRT)
        A.buf_automorph(left, ex, j)                             # sigma_j (embed x)
        sx, right = small.alloc(2), big.alloc(2)
        A.buf_automorph(sx, x, j % ms)
        right.embed_from(sx, 2, capi.ALCH_BASIS_CRT)             # embed (sigma_(j mod m) x)
        assert np.array_equal(left.download(), right.download()), (ms, mb, j)


# ---- 3. footprint, overlap, statuses -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,kind", [(45, "top31"), (9, "mix64"), (64, "top31"), (64, "top62")], ids=lambda v: str(v))
def test_footprint_and_overlap_rule(m, kind):
    qs = moduli(m, kind)
    ring = A.Ring(m, qs)
    j = seeded_unit(m, 3)
    host = uniform(np.random.default_rng(m), 9, ring.n, qs)
    # disjoint views inside one parent: only the destination range changes
    parent, (src, dst) = carve(ring, host, (1, 2), (5, 3))
    _check_raw(ring, dst, 1, src, 0, 2, j, capi.ALCH_OK)         # writes elements 6, 7 of the parent
    got = assert_parent_unchanged(parent, host, [(6, 2)])
    assert np.array_equal(got[6:8], apply_model(host[1:3], m, j))
    # adjacent views are accepted
    parent, (src, dst) = carve(ring, host, (1, 2), (3, 2))
    _check_raw(ring, dst, 0, src, 0, 2, j, capi.ALCH_OK)
    got = assert_parent_unchanged(parent, host, [(3, 2)])
    assert np.array_equal(got[3:5], apply_model(host[1:3], m, j))
    parent, (src, dst) = carve(ring, host, (3, 2), (1, 2))
    _check_raw(ring, dst, 0, src, 0, 2, j, capi.ALCH_OK)
    got = assert_parent_unchanged(parent, host, [(1, 2)])
    assert np.array_equal(got[1:3], apply_model(host[3:5], m, j))
    # coinciding ranges and ranges that share one element on either side are refused, nothing written
    for s_span, d_span in (((1, 3), (1, 3)), ((1, 3), (3, 3)), ((3, 3), (1, 3))):
        parent, (src, dst) = carve(ring, host, s_span, d_span)
        msg = _check_raw(ring, dst, 0, src, 0, 3, j, capi.ALCH_E_INVALID)
        assert msg.startswith("alch_buf_automorph:"), msg
        assert_parent_unchanged(parent, host)
    # the same through offsets into one handle
    whole = ring.upload(host)
    msg = _check_raw(ring, whole, 2, whole, 1, 2, j, capi.ALCH_E_INVALID)
    assert msg.startswith("alch_buf_automorph:")
    assert np.array_equal(whole.download(), host)


def test_statuses():
    m = 45
    qs = moduli(m, "top31")
    ring, other = A.Ring(m, qs), A.Ring(m, qs[:1])
    zp = A.Ring(m, [8], nocrt=True)
    host = uniform(np.random.default_rng(1), 6, ring.n, qs)
    parent, (src, dst) = carve(ring, host, (1, 2), (3, 2))
    lib = capi.load_library()
    for j in (3, 5, 0, 45, 48):                                                          # non-units, before and after reduction
        assert "unit" in _check_raw(ring, dst, 0, src, 0, 2, j, capi.ALCH_E_INVALID)
    _check_raw(ring, dst, 0, src, 0, 3, 7, capi.ALCH_E_INVALID)                          # one past either view
    _check_raw(ring, dst, 1, src, 0, 2, 7, capi.ALCH_E_INVALID)
    _check_raw(ring, dst, 0, src, 1, 2, 7, capi.ALCH_E_INVALID)
    _check_raw(ring, dst, 0, src, 0, 2 ** 64 - 1, 7, capi.ALCH_E_INVALID)
    ob = other.alloc(2)
    _check_raw(ring, ob, 0, src, 0, 2, 7, capi.ALCH_E_INVALID)                           # different rings
    za, zb = zp.alloc(2), zp.alloc(2)
    _check_raw(zp, za, 0, zb, 0, 2, 7, capi.ALCH_E_NO_CRT)
    assert lib.alch_buf_automorph(None, 0, src._h, 0, 1, 7) == capi.ALCH_E_INVALID
    _check_raw(ring, dst, 0, src, 0, 0, 7, capi.ALCH_OK)                                 # count = 0: nothing queued
    _check_raw(ring, dst, 2, src, 2, 0, 7, capi.ALCH_OK)
    assert_parent_unchanged(parent, host)


# ---- 4. the ciphertext operation against the composition that defines it -----------------------------------------------------------
CT_ROWS = [
    # m', moduli, gadget, s_pre = -1, batch, ring options, keyed
    (64, "p29", TRIV, False, 5, {}, False),
    (64, "p29", BASE2, True, 5, {}, False),
    (64, "p29", POW2_4, False, 5, {}, False),
    (64, "top62", TRIV, True, 5, {}, False),
    (1 << 12, "p29", TRIV, True, 5, {}, False),
    (1 << 12, "p29", POW2_4, False, 5, {}, False),
    (1 << 12, "top31x4", BASE2, False, 37, {"scratch_mib": 1}, False),     # 64 KiB per ciphertext: gather chunks of 16, 16, 5
    (45, "p29", TRIV, False, 5, {}, True),
    (45, "p29", BASE2, True, 5, {}, False),
    (45, "p29", POW2_4, False, 5, {}, False),
    (45, "top62", POW2_4, True, 5, {}, False),
]


@pytest.mark.parametrize("m,kind,gadget,neg,batch,opts,keyed", CT_ROWS, ids=lambda v: str(v))
def test_ct_automorph_equals_gather_then_identity_tunnel(m, kind, gadget, neg, batch, opts, keyed):
    qs = primes_below(m, 4, 1 << 31) if kind == "top31x4" else moduli(m, kind)
    ring = A.Ring(m, qs)
    for name, value in opts.items():
        ring.set_option(name, value)
    if opts:
        assert (1 << 20) // (2 * ring.n * ring.L * ring.word_bytes) == 16 and batch % 16
    if keyed:
        ring.set_rng_key(KEY)
    j = seeded_unit(m, 11 + gadget)
    D = ring.gadget_digits(gadget)
    rng = np.random.default_rng(m + gadget)
    ks_host = uniform(rng, 2 * D, ring.n, qs)
    cts_host = uniform(rng, 2 * batch, ring.n, qs)
    ks, cts = ring.upload(ks_host), ring.upload(cts_host)
    s_pre = [q - 1 for q in qs] if neg else None
    # the composition: alch_buf_automorph on the batch, then the existing tunnel from the ring to itself with lin_crt = crt(1)
    lin = ring.upload(np.ones((1, ring.n, ring.L), dtype=np.int64))
    tun = A.Tunnel(ring, ring, lin, ks, gadget=gadget)
    assert A.Tunnel.info(ring, ring) == (m, 1)
    perm, want = ring.alloc(2 * batch), ring.alloc(2 * batch)
    A.buf_automorph(perm, cts, j)
    tun.apply(perm, want, batch, s_pre=s_pre)
    want_host = want.download()
    assert_reduced(want_host, qs)
    auto = A.Automorph(ring, j, ks, gadget)
    ks.fill_uniform(12345)                                       # the hint was copied at create time
    out = ring.alloc(2 * batch + 1)
    out.fill_uniform(3)
    guard = out.download(2 * batch, 1)
    got = A.ct_automorph(auto, cts, batch, s_pre=s_pre, out=out)
    assert got is out
    assert np.array_equal(out.download(0, 2 * batch), want_host)
    assert np.array_equal(out.download(2 * batch, 1), guard)     # nothing past 2 * batch elements
    assert np.array_equal(cts.download(), cts_host)              # the input is not modified
    # a second call reuses the scratch and the cached table
    out2 = A.ct_automorph(auto, cts, batch, s_pre=s_pre)
    assert np.array_equal(out2.download(0, 2 * batch), want_host)
    lib = capi.load_library()
    for flags in (capi.ALCH_POW_IN, capi.ALCH_POW_OUT, capi.ALCH_POW_IN | capi.ALCH_POW_OUT):
        assert lib.alch_ct_automorph(auto._h, cts._h, out._h, batch, None, flags) == capi.ALCH_E_UNSUPPORTED
    assert lib.alch_ct_automorph(auto._h, cts._h, out._h, batch, None, 4) == capi.ALCH_E_INVALID
    assert lib.alch_ct_automorph(auto._h, cts._h, cts._h, batch, None, 0) == capi.ALCH_E_INVALID          # out must not overlap in
    assert lib.alch_last_error().decode().startswith("alch_ct_automorph:")
    assert lib.alch_ct_automorph(auto._h, cts._h, out._h, batch + 1, None, 0) == capi.ALCH_E_INVALID      # in holds 2 * batch
    assert lib.alch_ct_automorph(auto._h, cts._h, out._h, 0, None, 0) == capi.ALCH_OK
    assert np.array_equal(out.download(0, 2 * batch), want_host)
    auto.free()
    tun.free()


def test_create_statuses():
    m = 45
    qs = moduli(m, "p29")
    ring, other = A.Ring(m, qs), A.Ring(m, qs[:2])
    zp = A.Ring(m, [8], nocrt=True)
    ks, short, ko, kz = ring.alloc(2 * ring.L), ring.alloc(2 * ring.L - 1), other.alloc(4), zp.alloc(2)
    ks.fill_uniform(1)
    lib = capi.load_library()
    import ctypes as C
    h = C.c_void_p()

    def create(r, j, gadget, k):
        return lib.alch_automorph_create(r._h, j, gadget, k._h, C.byref(h))

    assert create(ring, 3, TRIV, ks) == capi.ALCH_E_INVALID and b"unit" in lib.alch_last_error()
    assert create(ring, 7, 99, ks) == capi.ALCH_E_INVALID
    assert create(ring, 7, capi.ALCH_GAD_BASEPOW2(17), ks) == capi.ALCH_E_INVALID
    assert create(ring, 7, TRIV, short) == capi.ALCH_E_INVALID
    assert create(ring, 7, TRIV, ko) == capi.ALCH_E_INVALID
    assert create(zp, 7, TRIV, kz) == capi.ALCH_E_NO_CRT
    assert h.value is None
    assert lib.alch_automorph_free(None) == capi.ALCH_OK
    auto = A.Automorph(ring, 7 + 45, ks)                                                  # j is reduced
    assert auto.j == 7
    oc = other.alloc(4)
    assert lib.alch_ct_automorph(auto._h, oc._h, oc._h, 1, None, 0) == capi.ALCH_E_INVALID   # buffers of another ring
    auto.free()


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp,m,p,j,gadget", [(64, 16, 8, 5, TRIV), (64, 16, 8, 63, POW2_4), (45, 9, 4, 7, BASE2), (45, 9, 4, 44, TRIV)])
def test_encrypt_automorph_decrypt(mp, m, p, j, gadget):
    """gen_sk -> automorph_hint -> encrypt_batch -> ct_automorph -> decrypt_batch = sigma_(j mod m) of the plaintext; then sigma_(1/j)
    brings the original back.  The error rates are printed; the assertion is that every ciphertext decrypts."""
    batch, seed = 4, 7000 + mp + j
    qs = moduli(mp, "p29")
    big, sm = G.Index(mp), G.Index(m)
    svar = 3.0 / np.sqrt(float(big.n))
    ring = A.Ring(mp, qs)
    zp_big = A.Ring(mp, [p], nocrt=True)
    zp_small = A.Ring(m, [p], nocrt=True)
    sk = E.gen_sk(ring, svar, seed)
    jinv = pow(j, -1, mp)
    auto = A.Automorph(ring, j, A.automorph_hint(ring, sk, j, gadget, svar, seed + 1), gadget)
    back_auto = A.Automorph(ring, jinv, A.automorph_hint(ring, sk, jinv, gadget, svar, seed + 2), gadget)
    rnd = random.Random(seed)
    pts = np.array([[[rnd.randrange(p)] for _ in range(sm.n)] for _ in range(batch)], dtype=np.int64)
    cts = E.encrypt_batch(ring, sk, zp_small.upload(pts), zp_small, zp_big, svar, seed + 3)
    meta = A.CtMeta("LSD", 0, 1, p)
    out, meta_out = A.ct_automorph(auto, cts, batch, s_pre=[pow(p, -1, q) for q in qs], meta=meta)   # LSD in: toMSD's scalar
    assert meta_out is meta
    to_lsd = [p % q for q in qs]
    rates = A.error_rates(out, batch, sk, s_pre=to_lsd)
    print(f"m'={mp} j={j} gadget={gadget}: error rates after sigma_j {rates}")
    got = A.decrypt_batch(out, batch, sk, zp_big, zp_small, 0, 1, s_pre=to_lsd).download(0, batch)
    for b in range(batch):
        pt = [int(x) for x in pts[b, :, 0]]
        want = M.sigma_pow(pt, sm, j % m, p)
        if m & (m - 1) == 0:
            assert want == M.sigma_pow_twopower(pt, j % m, p)
        assert got[b, :, 0].tolist() == want, b
    again = A.ct_automorph(back_auto, out, batch)                                        # MSD already: no scalar
    rates = A.error_rates(again, batch, sk, s_pre=to_lsd)
    print(f"m'={mp} j={j} gadget={gadget}: error rates after sigma_j then sigma_(1/j) {rates}")
    got = A.decrypt_batch(again, batch, sk, zp_big, zp_small, 0, 1, s_pre=to_lsd).download(0, batch)
    assert np.array_equal(got, pts)
    auto.free()
    back_auto.free()


# ---- 6. a loaded stream -------------------------------------------------------------------------------------------------------------
def test_source_produced_behind_ballast():
    """RAW and the download right behind the call: the source is copied into place behind ballast on the ring's stream, the gather
    must run after it, and the download right after the call must see the gather's words."""
    from stream_load import Ballast, busy
    m, j, count = 1 << 12, 5, 6
    qs = moduli(m, "top31")
    ring = A.Ring(m, qs)
    host = uniform(np.random.default_rng(12), count, ring.n, qs)
    staged, src, dst = ring.upload(host), ring.alloc(count), ring.alloc(count)
    src.fill_uniform(1)
    dst.fill_uniform(2)
    ring.sync()
    ballast = Ballast(ring)
    ballast.push()
    src.copy_from(staged, count)
    A.buf_automorph(dst, src, j)
    assert busy(ring), "the ballast drained before the call returned: the case proved nothing"
    got = dst.download()
    assert np.array_equal(got, apply_model(host, m, j))
    ring.sync()
    ballast.close()
