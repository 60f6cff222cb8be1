"""GPU: the general-index engine (alchemy_amd/csrc/kernel_gen.hpp, gen_host.hpp) at its STRUCTURAL edges, through the C ABI, bit for
bit against the C restatement (oracle/lol_tensor_gen.c, pinned to the by-definition model at these very indices in
tests/test_oracle_general.py).  The engine picks its code by the shape of the index at least as much as by the modulus; ROWS names
the shapes and, for every index, the property it was chosen for.  tests/test_gen_plan_host.py asserts those properties on the plans
gen_plan really lays out (without a device), so this file stays honest if the planner changes.

  prime 11          CRT_11 alone (one group per pass), CRT_11 innermost / in the middle / outermost, DFT_11 with one, two, three stages
  deep DFT chains   DFT_7 / DFT_13 with two stages, DFT_3 with six, DFT_5 with four
  scalar loaders    phi(m) % 4 != 0 at 4-byte words (m = 3^k, 7^k, 11^k): every kernel moves one word at a time
  pass placement    every prime innermost (stride 1: the 16-byte path for R = 4 and 12, the strided one for R = 2, 6, 10) and outermost;
                    a two-power axis ending in a block of 1, 2 and 3 stages in front of an odd axis
  size selectors    gen_threads 128 <-> 256 <-> 512, the fused <-> composed key switch at phi = 12288, the full 160 KiB of LDS
  refusal           one index past the LDS limit at either word size
  8-byte words      every prime's CRT and DFT pass, the 16-byte path for R = 2, 6, 10, the same size selectors

Moduli: the largest primes = 1 (mod m) below 2^31 (below 2^62 in the 8-byte rows); indices with a factor 7 or 13 also run on the largest
primes below 2^32 / 6, which select the SMALLQ = 2 instantiations of the p = 7 and p = 13 passes.  Operands: per case one uniform
element, one of helpers.extreme_words and the constant q - 1, in turn.  The numbered tests are the battery; a row runs the lines ROWS
gives it."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from helpers import assert_reduced, extreme_words, oracle_full_mul_base2_down, oracle_full_mul_general, primes_below

pytestmark = pytest.mark.gpu

SMALLQ_BELOW = 715827882                    # 2^32 / 6 (helpers.DENSE_LEVEL2_BELOW)
LDS_BYTES = 163840                          # alch_ring_create: phi(m) * word <= 160 KiB

Row = namedtuple("Row", "word lines indices nts fused batch")
ALL6, L14, L12, L124 = (1, 2, 3, 4, 5, 6), (1, 2, 3, 4), (1, 2), (1, 2, 4)


def row(word, lines, indices, nts=(0,), fused=(1,), batch=3):
    return Row(word, lines, indices, nts, fused, batch)


# Property words (checked by tests/test_gen_plan_host.py on gen_plan's output; `word` is the row's word size):
#   crt:P         a GK_SYM_CRT pass with r = P - 1              dft:P:K      exactly K GK_SYM_DFT passes with r = P
#   inner:KIND:R  the stride-1 pass is KIND (crt / dft) with r = R; strided:  it takes the strided path (R % (16 / word) != 0)
#   contig:R      the stride-1 pass has r = R and takes the 16-byte path (R % (16 / word) == 0)
#   outer:P       the first factor is P                         last:P       the last factor is P
#   tail:K        the two-power axis ends in a block of K stages, and an odd axis follows it
#   one_group     every pass has a single group                 groups<128   every pass has fewer groups than the smallest workgroup
#   scalar        phi % (16 / word) != 0: the one-word loaders  vector       phi % (16 / word) == 0
#   nt:N          gen_threads picks N threads by size           fused / composed   phi <= / > GEN_KS_T * GEN_KS_NPT
#   lds_full      phi * word == 160 KiB                         npass:K      K passes
ROWS = {
    # CRT_11 alone, one group per pass; again at every workgroup size
    "crt11_alone": (row(4, ALL6, (11,), nts=(0, 128, 256, 512)),
                    {11: "crt:11 inner:crt:10 strided one_group scalar"}),
    # CRT_11 innermost behind other axes; 11 in the middle and outermost
    "crt11_placed": (row(4, ALL6, (33, 44, 77, 143, 1001, 352)),
                     {33: "crt:11 inner:crt:10 outer:3 groups<128", 44: "crt:11 inner:crt:10 outer:2 groups<128",
                      77: "crt:11 inner:crt:10 outer:7 groups<128", 143: "crt:11 outer:11 contig:12 groups<128",
                      1001: "crt:11 outer:7 last:13", 352: "crt:11 inner:crt:10 outer:2 tail:1"}),
    # DFT_11 with one and two stages
    "dft11": (row(4, ALL6, (121, 1331, 5324)),
              {121: "dft:11:1 inner:dft:11 groups<128 scalar", 1331: "dft:11:2 inner:dft:11 scalar", 5324: "dft:11:2 inner:dft:11 outer:2 vector"}),
    # DFT_7 / DFT_13 with two stages, DFT_3 with at least four, DFT_5 with at least three
    "dft_deep": (row(4, L14, (2197, 3125)), {2197: "dft:13:2 inner:dft:13", 3125: "dft:5:4 inner:dft:5"}),
    # phi % 4 != 0: the one-word loaders of every kernel (121 and 1331 run in the row above; 343 and 2187 are deep DFT chains as well)
    "scalar": (row(4, ALL6, (7, 9, 49, 343, 2187)),
               {7: "scalar crt:7", 9: "scalar dft:3:1", 49: "scalar dft:7:1", 343: "scalar dft:7:2 inner:dft:7", 2187: "scalar dft:3:6 inner:dft:3"}),
    # every prime innermost (stride 1) and every prime outermost
    "placement": (row(4, L12, (12, 20, 28, 156, 260, 364, 572, 52, 39, 65, 91)),
                  {12: "outer:2 inner:crt:2 strided tail:1", 20: "outer:2 contig:4", 28: "outer:2 inner:crt:6 strided",
                   156: "crt:3 contig:12", 260: "crt:5 contig:12", 364: "crt:7 contig:12", 572: "crt:11 contig:12", 52: "outer:2 contig:12",
                   39: "outer:3 contig:12", 65: "outer:5 contig:12", 91: "outer:7 contig:12"}),
    # a two-power axis ending in a block of 1, 2, 3 stages in front of an odd axis (3 * 2^a; a = 2 is 12, in the row above)
    "r2tail": (row(4, L12, (24, 48, 96, 192, 384, 768)),
               {24: "tail:2 inner:crt:2", 48: "tail:3 inner:crt:2", 96: "tail:1 inner:crt:2 npass:3", 192: "tail:2 inner:crt:2 npass:3",
                384: "tail:3 inner:crt:2 npass:3", 768: "tail:1 inner:crt:2 npass:4"}),
    # gen_threads 128 <-> 256 (4-byte words: 18431 bytes)
    "nt128_256": (row(4, L14, (15876, 13824), batch=2), {15876: "nt:128 fused", 13824: "nt:256 fused"}),
    # gen_threads 256 <-> 512 (40960 bytes)
    "nt256_512": (row(4, L14, (42240, 31104), batch=2), {42240: "nt:256 crt:11 fused", 31104: "nt:512 dft:3:4 fused"}),
    # fused <-> composed key switch (phi = 12288): with gen_fused at its default and at 0
    "fused_edge": (row(4, L14, (53760, 21609, 14641), fused=(1, 0), batch=2),
                   {53760: "fused vector nt:512", 21609: "composed vector nt:512 dft:7:3", 14641: "composed scalar nt:512 dft:11:3"}),
    # the LDS limit at 4-byte words
    "lds_limit": (row(4, L14, (102400, 90112, 168960, 59049), batch=2),
                  {102400: "lds_full nt:512 composed", 90112: "lds_full nt:512 composed crt:11", 168960: "lds_full nt:512 composed crt:11",
                   59049: "scalar npass:10 nt:512 composed dft:3:9"}),
    # 8-byte words: every prime's CRT and DFT pass; the 16-byte path for R = 2, 6, 10 (12 and 28 are there for R = 2 and 6)
    "word64": (row(8, L124, (9, 49, 121, 169, 100, 132, 1331, 12, 28)),
               {9: "crt:3 dft:3:1", 49: "crt:7 dft:7:1", 121: "crt:11 dft:11:1", 169: "crt:13 dft:13:1", 100: "crt:5 dft:5:1 outer:2",
                132: "contig:10 crt:3", 1331: "dft:11:2", 12: "contig:2", 28: "contig:6"}),
    # 8-byte words: gen_threads and the LDS limit
    "word64_sizes": (row(8, L124, (3969, 5824, 21120, 12285, 84480), batch=2),
                     {3969: "nt:128", 5824: "nt:256", 21120: "nt:256 contig:10", 12285: "nt:512", 84480: "lds_full nt:512 contig:10"}),
}
# refused above the limit: (index, phi, word size at which phi * word first exceeds 160 KiB)
REFUSED = [(60025, 41160, 4), (26411, 20580, 8)]

Case = namedtuple("Case", "row m tag nt batch word")


def has_7_or_13(m):
    return m % 7 == 0 or m % 13 == 0


def cases(line):
    out = []
    for name, (r, _) in ROWS.items():
        if line not in r.lines:
            continue
        for m in r.indices:
            tags = ("top62",) if r.word == 8 else (("top31", "smallq") if has_7_or_13(m) else ("top31",))
            out += [Case(name, m, tag, nt, r.batch, r.word) for tag in tags for nt in r.nts]
    return out


def case_id(c):
    if not isinstance(c, Case):
        return None                             # the other arguments keep pytest's own ids
    return f"{c.row}-{c.m}-{c.tag}" + (f"-nt{c.nt}" if c.nt else "")


def with_fused(line):
    """(case, gen_fused): both settings where the row asks for them (every row on line 2)."""
    return [(c, f) for c in cases(line) for f in ((1, 0) if line == 2 else ROWS[c.row][0].fused)]


@functools.lru_cache(maxsize=None)
def moduli(m, tag, count):
    """The `count` largest primes = 1 (mod m) of the class, largest first; None where the class holds fewer."""
    hi = {"top31": 1 << 31, "smallq": SMALLQ_BELOW, "top62": 1 << 62}[tag]
    try:
        return tuple(primes_below(m, count, hi))
    except AssertionError:
        return None


def ring_moduli(c, count):
    qs = moduli(c.m, c.tag, count)
    if qs is None:
        pytest.skip(f"fewer than {count} primes = 1 (mod {c.m}) in the class {c.tag}")
    return list(qs)


def open_ring(c, qs, *more):
    """A.Ring of every modulus list given, with the case's gen_nt; the first ring asserts the word size of the row."""
    rings = [A.Ring(c.m, q) for q in (qs,) + more]
    assert rings[0].word_bytes == c.word
    for r in rings:
        r.set_option("gen_nt", c.nt)
    return rings if more else rings[0]


def operands(rng, count, n, qs, shift=0):
    """(count, n, L): element e is uniform, extreme words or the constant q - 1, in turn."""
    qv = np.array(qs, dtype=np.int64)
    x = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.int64) for q in qs], axis=1) for _ in range(count)])
    ext = extreme_words(rng, count, n, qs)
    for e in range(count):
        kind = (e + shift) % 3
        if kind == 1:
            x[e] = ext[e]
        elif kind == 2:
            x[e] = qv - 1
    return x


def fetch(buf, qs):
    got = buf.download()
    assert_reduced(got, qs)
    return got


# ---- 1. transforms and columns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", cases(1), ids=case_id)
def test_1_transforms_and_columns(oracle_lib, c):
    qs = ring_moduli(c, 2)
    g, o = open_ring(c, qs), oracle_lib.GenRing(c.m, qs)
    assert g.n == o.n
    x = operands(np.random.default_rng(c.m), 3, g.n, qs)
    for a in x:                                             # host-buffer Tensor methods, one ring element each
        for name in ("crt", "crtinv", "l", "linv", "mulg_pow", "mulg_dec", "mulg_crt", "divg_crt"):
            got = getattr(g, name)(a)
            assert_reduced(got, qs)
            assert np.array_equal(got, getattr(o, name)(a)), name
        for name in ("divg_pow", "divg_dec"):
            want, got = getattr(o, name)(a), getattr(g, name)(a)
            assert want is not None and got is not None, name          # the radical is a unit mod every q = 1 (mod m)
            assert_reduced(got, qs)
            assert np.array_equal(got, want), name
    # batched device forms, with element ranges
    buf = g.upload(x)
    buf.crt()
    want_crt = np.stack([o.crt(e) for e in x])
    assert np.array_equal(fetch(buf, qs), want_crt)
    buf.mulg(capi.ALCH_BASIS_CRT, 1, 2)
    assert np.array_equal(fetch(buf, qs), np.stack([want_crt[0], o.mulg_crt(want_crt[1]), o.mulg_crt(want_crt[2])]))
    buf.crtinv()
    assert np.array_equal(fetch(buf, qs), np.stack([x[0], o.mulg_pow(x[1]), o.mulg_pow(x[2])]))
    assert buf.divg(capi.ALCH_BASIS_POW, 1, 2)
    assert np.array_equal(fetch(buf, qs), x)
    buf.linv(0, 2)
    assert np.array_equal(fetch(buf, qs), np.stack([o.linv(x[0]), o.linv(x[1]), x[2]]))
    buf.mulg(capi.ALCH_BASIS_DEC, 0, 1)
    assert buf.divg(capi.ALCH_BASIS_DEC, 1, 2)
    buf.l(0, 2)
    assert np.array_equal(fetch(buf, qs), np.stack([o.l(o.mulg_dec(o.linv(x[0]))), o.l(o.divg_dec(o.linv(x[1]))), o.divg_dec(x[2])]))


# ---- 2. keySwitchQuadCirc(hint, a * b), TrivGad ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,fused", with_fused(2), ids=case_id)
def test_2_ct_mul_relin(oracle_lib, c, fused):
    qs, batch = ring_moduli(c, 2), c.batch
    g, o = open_ring(c, qs), oracle_lib.GenRing(c.m, qs)
    g.set_option("gen_fused", fused)
    rng = np.random.default_rng(c.m + 2)
    hint, a, b = operands(rng, 4, g.n, qs), operands(rng, 2 * batch, g.n, qs), operands(rng, 2 * batch, g.n, qs, shift=1)
    s_pre = [int(rng.integers(1, q)) for q in qs]
    gh, gout = g.hint_load(hint), g.alloc(2 * batch)
    g.ct_mul_relin(gh, g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
    got = fetch(gout, qs)
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre)
        assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), ct
    apow, bpow = np.stack([o.crtinv(e) for e in a]), np.stack([o.crtinv(e) for e in b])
    g.ct_mul_relin(gh, g.upload(apow), g.upload(bpow), gout, batch, s_pre=s_pre, flags=capi.ALCH_POW_IN | capi.ALCH_POW_OUT)
    assert np.array_equal(fetch(gout, qs), np.stack([o.crtinv(e) for e in got]))


# ---- 3. PT2CT's whole mul_: 2 -> 3 -> 1 and 2 -> 3 -> 2 limbs ---------------------------------------------------------------------
@pytest.mark.parametrize("l_out", [1, 2])
@pytest.mark.parametrize("c,fused", with_fused(3), ids=case_id)
def test_3_ct_mul_full(oracle_lib, c, fused, l_out):
    qs_h, batch = ring_moduli(c, 3), c.batch
    rh, rin, rout = open_ring(c, qs_h, qs_h[1:], qs_h[3 - l_out:])
    for r in (rh, rin, rout):
        r.set_option("gen_fused", fused)
    rng = np.random.default_rng(c.m + 3)
    hint = operands(rng, 6, rh.n, qs_h)
    a, b = operands(rng, 2 * batch, rh.n, qs_h[1:]), operands(rng, 2 * batch, rh.n, qs_h[1:], shift=1)
    s_pre = [int(rng.integers(1, q)) for q in qs_h[1:]]
    gh, ga, gb, gout = rh.hint_load(hint), rin.upload(a), rin.upload(b), rout.alloc(2 * batch)
    want = {po: [oracle_full_mul_general(oracle_lib, c.m, qs_h, 2, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                         s_pre, po) for ct in range(batch)] for po in (False, True)}
    for lin in (1, 0):                          # the closing modSwitch keeps the surviving limbs in the CRT basis / every limb through Pow, Dec
        rh.set_option("rs_lin", lin)
        for pow_out in (False, True):
            capi.ct_mul_full(gh, ga, gb, gout, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
            got = fetch(gout, qs_h[3 - l_out:])
            for ct in range(batch):
                w0, w1 = want[pow_out][ct]
                assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), (ct, pow_out, lin)


# ---- 4. modSwitch down by one and by two limbs from L = 3, and up again -----------------------------------------------------------
@pytest.mark.parametrize("drop", [1, 2])
@pytest.mark.parametrize("c", cases(4), ids=case_id)
def test_4_ct_mod_switch(oracle_lib, c, drop):
    qs, batch = ring_moduli(c, 3), c.batch
    Rb, Rs = open_ring(c, qs, qs[drop:])
    ob, osm = oracle_lib.GenRing(c.m, qs), oracle_lib.GenRing(c.m, qs[drop:])
    x = operands(np.random.default_rng(c.m + 4), 2 * batch, Rb.n, qs)
    gx, gy = Rb.upload(x), Rs.alloc(2 * batch)
    want = []
    for e in range(2 * batch):                  # rescaleDec on c0, rescalePow on c1, one limb at a time
        cur = ob.crtinv(x[e])
        if e % 2 == 0:
            cur = ob.linv(cur)
        for u in range(drop):
            cur = oracle_lib.GenRing(c.m, qs[u:]).rescale_drop0(cur)
        if e % 2 == 0:
            cur = osm.l(cur)
        want.append(osm.crt(cur))
    for lin in (1, 0):                          # k_gen_rescale_drop + _keep / the limb-at-a-time form
        Rb.set_option("rs_lin", lin)
        capi.ct_mod_switch(gx, gy, batch)
        got = fetch(gy, qs[drop:])
        for e in range(2 * batch):
            assert np.array_equal(got[e], want[e]), (e, lin)
        capi.ct_mod_switch(gx, gy, batch, flags=capi.ALCH_POW_OUT)         # k_gen_rescale_keep_pow
        gotp = fetch(gy, qs[drop:])
        for e in range(2 * batch):
            assert np.array_equal(gotp[e], osm.crtinv(want[e])), (e, lin, "pow")
    assert np.array_equal(gx.download(), x)     # input untouched
    capi.ct_mod_switch(gx, gy, batch)
    gz = Rb.alloc(2 * batch)
    capi.ct_mod_switch(gy, gz, batch)           # and up again: (0, .., 0, q_a x)
    up = fetch(gz, qs)
    mult = 1
    for q in qs[:drop]:
        mult *= q
    for e in range(2 * batch):
        assert not up[e][:, :drop].any()
        assert np.array_equal(up[e][:, drop:], osm.scale(want[e], [mult % q for q in qs[drop:]])), e


# ---- 5. mul_ under a BaseBGad 2 hint on fewer limbs (k_gen_crt_base2_digits) -----------------------------------------------------
@pytest.mark.parametrize("c", cases(5), ids=case_id)
def test_5_ct_mul_full_base2(oracle_lib, c):
    qs_in, batch = ring_moduli(c, 3), 2
    rin, rh, rout = open_ring(c, qs_in, qs_in[1:], qs_in[2:])
    n = rin.n
    D = rh.gadget_digits(capi.ALCH_GAD_BASE2)
    rng = np.random.default_rng(c.m + 5)
    hint = operands(rng, 2 * D, n, qs_in[1:])
    a, b = operands(rng, 2 * batch, n, qs_in), operands(rng, 2 * batch, n, qs_in, shift=1)
    s_pre = [int(rng.integers(1, q)) for q in qs_in]
    gh = rh.hint_load(hint, gadget=capi.ALCH_GAD_BASE2)
    for l_out, ro in ((2, rh), (1, rout)):
        for pow_out in (False, True):
            out = ro.alloc(2 * batch)
            capi.ct_mul_full(gh, rin.upload(a), rin.upload(b), out, batch, s_pre=s_pre, flags=capi.ALCH_POW_OUT if pow_out else 0)
            got = fetch(out, qs_in[3 - l_out:])
            for ct in range(batch):
                w0, w1 = oracle_full_mul_base2_down(oracle_lib, n, qs_in, 2, l_out, list(hint), a[2 * ct], a[2 * ct + 1], b[2 * ct],
                                                    b[2 * ct + 1], s_pre, pow_out=pow_out, m=c.m)
                assert np.array_equal(got[2 * ct], w0) and np.array_equal(got[2 * ct + 1], w1), (l_out, ct, pow_out)


# ---- 6. the integer ring: mulG, divG with its not-divisible answer, l, lInv --------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in cases(6) if c.tag == "top31"], ids=case_id)
def test_6_integer_ring(oracle_lib, c):
    g, o = A.Ring(c.m, [0], nocrt=True), oracle_lib.GenRing(c.m, [0])
    assert g.word_bytes == 8 and g.n == o.n
    g.set_option("gen_nt", c.nt)
    rng = np.random.default_rng(c.m + 6)
    top = (1 << 31) - 1
    ext = np.array([0, 1, -1, top, -top, top - 1], dtype=np.int64)
    zs = [rng.integers(-10**6, 10**6, size=(g.n, 1), dtype=np.int64), ext[rng.integers(0, 6, size=(g.n, 1))],
          np.full((g.n, 1), -1, dtype=np.int64)]
    for z in zs:
        for mul, div in (("mulg_pow", "divg_pow"), ("mulg_dec", "divg_dec")):
            gz = getattr(g, mul)(z)
            assert np.array_equal(gz, getattr(o, mul)(z)), mul
            assert np.array_equal(getattr(g, div)(gz), z), div
            bad = gz.copy()
            bad[g.n // 2, 0] += 1
            assert getattr(o, div)(bad) is None
            assert getattr(g, div)(bad) is None, div          # ALCH_NOT_DIVISIBLE
        assert np.array_equal(g.l(z), o.l(z)) and np.array_equal(g.linv(z), o.linv(z))


# ---- refused above the LDS limit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,phi,word", REFUSED)
def test_an_index_past_the_lds_limit_is_refused(oracle_lib, m, phi, word):
    """alch_ring_create answers ALCH_E_UNSUPPORTED before anything is planned on the device; 26411 is past the limit at 8-byte words only
    and is served at 4-byte words."""
    assert phi * word > LDS_BYTES
    qs = list(moduli(m, "top31" if word == 4 else "top62", 2))
    with pytest.raises(A.AlchemyError) as e:
        A.Ring(m, qs)
    assert e.value.code == capi.ALCH_E_UNSUPPORTED and "160 KiB" in str(e.value)
    if word == 8:
        assert phi * 4 <= LDS_BYTES
        qs = list(moduli(m, "top31", 2))
        g, o = A.Ring(m, qs), oracle_lib.GenRing(m, qs)
        assert g.word_bytes == 4 and g.n == phi == o.n
        x = operands(np.random.default_rng(m), 3, g.n, qs)
        buf = g.upload(x)
        buf.crt()
        assert np.array_equal(fetch(buf, qs), np.stack([o.crt(e) for e in x]))
        buf.crtinv()
        assert np.array_equal(fetch(buf, qs), x)
