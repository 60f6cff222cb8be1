"""GPU: every fused two-power kernel variant on workgroups that walk SEVERAL work items.

In production the key-switch, tensor and rescale kernels run as persistent workgroups: the default ks_grid is 4096 and a
1024-ciphertext chunk at L = 4 has 8192 items, so every workgroup walks at least two.  State crosses the item boundary in
k_ks_accum_half -- the previous item's accumulators (pending, po0 / po1, prot), the previous item's modulus pq under which they are
reduced at the deferred store, `continue` on ct >= nct in the middle of a walk, the deferred flush_stores() -- and the rest of the
suite, whose shapes are small, runs nearly every instantiation with one item per workgroup.  Here a batch of 9 (two groups of eight
ciphertexts, the second holding ONE: seven of every eight of its item slots are skipped) runs under grids far below the item count:
  ks_grid = 8          a walk steps through the halves and limbs of one ciphertext slot: pq changes at every second step
  ks_grid = 5          a walk crosses ciphertext slots and groups and meets skipped items between live ones and at its end
  ks_grid = 5, ks_rev  the same from the chunk's last item to its first
  ks_map = 1           limb-per-XCD numbering (pl = 8 / L, x / L) at L = 1, 2, 8; at L = 3 and 5 the dispatch must ignore the option
  ti_split = 7         k_tensor_intt_split<15, .> on persistent workgroups (and ti_split = 9 L / 3 where 7 workgroups would walk fewer
                       than three items: L = 1 and 2); ti_grid = 3 for k_tensor_intt<11, u32>
  rs_slots = 3         k_rescale_out / k_rescale_out_lin: three workgroups over 18 (batch 9) or 10 (batch 5) items
and k_rescale_keep_half, whose XCD-aware numbering is grp = blockIdx / (8 Lo), item = grp * 8 + (rem & 7), gets three groups of items
(the last holding two) at Lo = 1, 3, 4 and 5.  Ciphertext e and hint element e alternate between uniform words and
helpers.extreme_words; the ciphertexts of a batch are all distinct (asserted), so a misdecoded ciphertext index shows.  Every output
buffer is filled with other words before the call, every output word is compared with the C restatement (pinned to the by-definition
model on exactly these rings and shapes by tests/test_oracle_item_walk_rings.py) and every stored word must lie below its modulus.
Every case asserts what it claims: 4-byte words, (qmax - 1) / 2 < qmin or not, every modulus below 2^30 or not, the dispatch's item
count (restated from run_call, whose text is asserted to still stand) and 3 * grid <= items, so that every workgroup walks at least
three items.

Kernels per row, read off `dispatch` (run_call in kernels_ntt.hpp); LOGN in {11, 15}; the tensor kernel in front is
k_tensor_intt<11, u32> at n = 2^11 and k_tensor_intt_split<15, Q30> at n = 2^15 (Q30 = every modulus below 2^30):
  A. test_ct_mul_relin_item_walks (batch 9, 32 L key-switch items, 9 L tensor items)
       TOP1, TOP2, TOP3, TOP5, TOP8     k_tensor_intt_split<15, false> into k_ks_accum_half<LOGN, true>, L = 1, 2, 3, 5, 8
       B30_3, B30_8                     k_tensor_intt_split<15, true>  into k_ks_accum_half<LOGN, true, 32, false, true>, L = 3, 8
       MIXED3                           k_tensor_intt_split<15, false> into k_ks_accum_half<LOGN, false>
       MIXED30                          k_tensor_intt_split<15, true>  into k_ks_accum_half<LOGN, false>
  B. test_ct_mul_full_item_walks (ks_grid = 5 and rs_slots = 3 against default grids)
       top-4-5-3       k_ks_accum_half<LOGN, true, 32, true> (UP);        k_rescale_out_lin<LOGN, u32, 2, true>
       b30-4-5-3       k_ks_accum_half<LOGN, true, 32, true, true> (UP + Q30); k_rescale_out_lin<LOGN, u32, 2, true>
       mixed-4-5-3     k_ks_accum_half<LOGN, false, 32, true> (UP, unbalanced); k_rescale_out<11, u32>; at n = 2^15
                       k_rescale_drop_half + k_rescale_keep_half, ddn = 2, Lo = 3 (batch 9 and batch 5)
       top-7-8-5       k_ks_accum_half<LOGN, true, 32, true> on the largest hint ring, dup = 1; k_rescale_out<11, u32>; at n = 2^15
                       the half-size pair, ddn = 3, Lo = 5
       top-3-4-1       the same kernels, ddn = 3, Lo = 1
       top-4-5-4-half  n = 2^15 only, option rs_half = 1: the half-size pair where k_rescale_out_lin<15, u32, 1, true> would
                       serve, ddn = 1, Lo = 4
  C. test_ct_mul_relin_n65536_item_groups: k_tensor_crtinv_split + k_ks_accum_split<16, u32, true, true> (split_fused = 2) and
     k_tensor_ew, k_crt_split, k_ks_accum_split<16, u32, true> (split_fused = 1) -- one workgroup per item, numbered
     grp = blockIdx / (16 L): three limbs with a ragged second group of ciphertexts (batch 9), eight limbs (batch 2)."""
import functools
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT
from helpers import assert_reduced, extreme_words, oracle_full_mul, primes_1_mod, primes_below

pytestmark = pytest.mark.gpu

M16 = 1 << 16                                                   # moduli = 1 mod 2^16 serve every n <= 2^15
TOP8 = primes_below(M16, 8, 1 << 31)
B30_8 = primes_below(M16, 8, 1 << 30)
SMALL = primes_1_mod(M16, 2, 0)                                 # 65537 and 786433
MIXED3 = [TOP8[0]] + SMALL                                      # unbalanced
MIXED30 = [B30_8[0]] + SMALL                                    # every modulus below 2^30, and unbalanced
MIXED_FULL = MIXED3 + TOP8[1:3]
TOP17_8 = primes_below(1 << 17, 8, 1 << 31)                     # = 1 mod 2^17: n = 2^16

# name -> (moduli, (qmax - 1) / 2 < qmin, every modulus below 2^30): what ring_create_impl derives and `dispatch` picks by
RELIN_RINGS = {"TOP1": (TOP8[:1], True, False), "TOP2": (TOP8[:2], True, False), "TOP3": (TOP8[:3], True, False),
               "TOP5": (TOP8[:5], True, False), "TOP8": (TOP8, True, False), "B30_3": (B30_8[:3], True, True),
               "B30_8": (B30_8, True, True), "MIXED3": (MIXED3, False, False), "MIXED30": (MIXED30, False, True)}
# id -> (moduli of the hint's ring, L_in, L_out, options of every run, balanced, q30, sizes the row runs at)
FULL_ROWS = {"top-4-5-3": (TOP8[:5], 4, 3, {}, True, False, (11, 15)),
             "b30-4-5-3": (B30_8[:5], 4, 3, {}, True, True, (11, 15)),
             "mixed-4-5-3": (MIXED_FULL, 4, 3, {}, False, False, (11, 15)),
             "top-7-8-5": (TOP8, 7, 5, {}, True, False, (11, 15)),
             "top-3-4-1": (TOP8[:4], 3, 1, {}, True, False, (11, 15)),
             "top-4-5-4-half": (TOP8[:5], 4, 4, {"rs_half": 1}, True, False, (15,))}
SPLIT_RINGS = {"TOP17_3": TOP17_8[:3], "TOP17_8": TOP17_8}

BATCH = 9                                                       # two groups of eight ciphertexts, the second holds one
ORACLE_THREADS = 8                                              # the C restatement keeps no state between calls


def is_balanced(qs):
    """r->balanced of ring_create_impl."""
    return (max(qs) - 1) // 2 < min(qs)


def is_q30(qs):
    """r->q30 of ring_create_impl (4-byte rings)."""
    return max(qs) < (1 << 30)


@functools.lru_cache(maxsize=None)
def dispatch_source():
    csrc = os.path.join(ROOT, "alchemy_amd", "csrc")
    return "".join(open(os.path.join(csrc, f)).read() for f in ("kernels_ntt.hpp", "kernel_ks_half.hpp", "kernel_tensor_split.hpp",
                                                                "kernel_rescale_half.hpp", "kernel_rescale_out.hpp",
                                                                "kernel_crt_split.hpp", "alchemy_hip.hip"))


def source_has(*expressions):
    """The item counts and grids below restate what the dispatch computes; each restated expression must still stand in the sources,
    so that a change of the item numbering fails here and names the rows to resize."""
    for e in expressions:
        assert e in dispatch_source(), e


def ks_items(batch, L):
    """Work items of k_ks_accum_half for one chunk of `batch` ciphertexts: run_call's own formula."""
    source_has("size_t chunk = 1024;",                                           # batch 9 is one chunk
               "const size_t groups = (c.nct + 7) / 8;", "const unsigned nitems = (unsigned)(groups * 16 * (size_t)R.L);",
               "const unsigned persist = c.opts.ks_grid ? c.opts.ks_grid : 4096u;", "const unsigned grid = nitems < persist ? nitems : persist;",
               "for (unsigned item = blockIdx.x; item < nitems; item += gridDim.x) {", "if (ct >= nct) continue;")
    return 16 * L * ((batch + 7) // 8)


def tensor_items(batch, L):
    """Work items of k_tensor_intt_split / k_tensor_intt (ti_split > 1 / ti_grid > 0: that many persistent workgroups)."""
    source_has("const unsigned nitems = (unsigned)(c.nct * (size_t)R.L);",
               "const unsigned grid = split > 1 && (unsigned)split < nitems ? (unsigned)split : nitems;",
               "else if (ti_grid > 0 && (unsigned)ti_grid < nitems) grid = (unsigned)ti_grid;")
    return batch * L


def assert_walks(opts, batch, L, logn):
    """Every grid an option set names is so far below its kernel's item count that each workgroup walks at least three items."""
    if "ks_grid" in opts:
        assert 3 * opts["ks_grid"] <= ks_items(batch, L), opts
    if "ti_split" in opts and opts.get("walk", True):
        assert logn == 15 and 3 * opts["ti_split"] <= tensor_items(batch, L), opts
    if "ti_grid" in opts:
        assert logn != 15 and 3 * opts["ti_grid"] <= tensor_items(batch, L), opts
    if "ks_map" in opts:
        source_has("(c.opts.ks_map && 8 % R.L == 0)")


def alternating_words(rng, groups, per, n, qs):
    """(groups * per, n, L): the `per` elements of group e hold uniform words for even e and helpers.extreme_words for odd e."""
    count = groups * per
    uniform = np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2)
    odd = (np.arange(count) // per) % 2 == 1
    return np.ascontiguousarray(np.where(odd[:, None, None], extreme_words(rng, count, n, qs), uniform))


def assert_distinct(a, b, batch):
    """No two ciphertexts of the batch share an operand pair: a result stored under another ciphertext's index cannot be right."""
    for x in (a, b):
        assert len({hashlib.sha256(np.ascontiguousarray(x[2 * ct:2 * ct + 2])).digest() for ct in range(batch)}) == batch


def per_ciphertext(fn, batch):
    """[fn(ct) for ct in range(batch)] on a few threads (ctypes releases the GIL around the C restatement's calls)."""
    with ThreadPoolExecutor(max_workers=ORACLE_THREADS) as pool:
        return list(pool.map(fn, range(batch)))


def check_pairs(got, want, qs, what):
    assert_reduced(got, qs)
    for ct, (w0, w1) in enumerate(want):
        assert np.array_equal(got[2 * ct], w0), f"c0 mismatch ct {ct} {what}"
        assert np.array_equal(got[2 * ct + 1], w1), f"c1 mismatch ct {ct} {what}"


def _minus_one(qs):
    return [q - 1 for q in qs]


def test_the_moduli_are_where_the_cases_need_them():
    assert TOP8 == [2147352577, 2146959361, 2146041857, 2145976321, 2144796673, 2144468993, 2144010241, 2143092737]
    assert B30_8 == [1073479681, 1072496641, 1071513601, 1070727169, 1069219841, 1068564481, 1068433409, 1068236801]
    assert TOP17_8 == [2147352577, 2146959361, 2146041857, 2144468993, 2142502913, 2135818241, 2135162881, 2135031809]
    assert SMALL == [65537, 786433]
    assert len(set(TOP8 + B30_8 + SMALL)) == 18 and len(set(TOP17_8)) == 8
    assert all((1 << 31) - (1 << 23) < q < (1 << 31) for q in TOP8) and all((1 << 31) - (1 << 25) < q < (1 << 31) for q in TOP17_8)
    assert all((1 << 30) - (1 << 24) < q < (1 << 30) for q in B30_8)
    assert all(q % M16 == 1 for q in TOP8 + B30_8 + SMALL) and all(q % (1 << 17) == 1 for q in TOP17_8)
    for name, (qs, bal, q30) in RELIN_RINGS.items():
        assert (is_balanced(qs), is_q30(qs)) == (bal, q30), name
    assert sorted(len(qs) for qs, _, _ in RELIN_RINGS.values()) == [1, 2, 3, 3, 3, 3, 5, 8, 8]
    for name, (qs_h, l_in, l_out, _, bal, q30, _) in FULL_ROWS.items():
        assert (is_balanced(qs_h), is_q30(qs_h)) == (bal, q30) and l_in < len(qs_h) and 1 <= len(qs_h) - l_out <= 3, name
    for qs in SPLIT_RINGS.values():
        assert is_balanced(qs) and not is_q30(qs)


# ---- A. keySwitchQuadCirc hint (a * b) ------------------------------------------------------------------------------------------------
def relin_option_sets(logn, L, batch):
    """(options, s_pre = -1 as well): the control first.  `walk: False` marks ti_split = 7 where its seven workgroups walk fewer than
    three items (9 L < 21: L = 1 and 2); the set behind it then has the largest grid that does walk three."""
    sets = [({}, False), ({"ks_grid": 8}, False), ({"ks_grid": 5}, True), ({"ks_grid": 5, "ks_rev": 1}, False), ({"ks_map": 1}, False)]
    if logn == 15:
        items = tensor_items(batch, L)
        sets.append(({"ti_split": 7, "walk": 3 * 7 <= items}, False))
        if 3 * 7 > items:
            sets.append(({"ti_split": items // 3}, False))
    else:
        sets.append(({"ti_grid": 3}, False))
    return sets


@pytest.mark.parametrize("name", list(RELIN_RINGS))
@pytest.mark.parametrize("logn", [11, 15])
def test_ct_mul_relin_item_walks(oracle_lib, logn, name):
    """Batch 9 on every key-switch instantiation without added limbs (module docstring, A) under the option sets of
    relin_option_sets; ks_grid = 5 also with s_pre = [q-1 ...].  ks_map = 1 at L = 3 and 5 must give the control's words."""
    import alchemy_amd as A
    qs, bal, q30 = RELIN_RINGS[name]
    n, L, batch = 1 << logn, len(qs), BATCH
    assert (is_balanced(qs), is_q30(qs)) == (bal, q30)
    assert ks_items(batch, L) == 32 * L
    o = oracle_lib.Ring(n, qs)
    rng = np.random.default_rng(6100 + 16 * logn + L + 2 * q30 + bal)
    hint = alternating_words(rng, 2 * L, 1, n, qs)
    a, b = alternating_words(rng, batch, 2, n, qs), alternating_words(rng, batch, 2, n, qs)
    assert_distinct(a, b, batch)
    hints = list(hint)
    want = {s: per_ciphertext(lambda ct, s=s: o.ct_mul_relin(hints, a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1],
                                                             s_pre=_minus_one(qs) if s else None), batch) for s in (False, True)}
    control = None
    for opts, both_s in relin_option_sets(logn, L, batch):
        assert_walks(opts, batch, L, logn)
        g = A.Ring(2 * n, qs)                                    # a refusal raises: the test fails
        assert g.word_bytes == 4
        for k, v in opts.items():
            if k != "walk":
                g.set_option(k, v)
        ghint, ga, gb, gout = g.hint_load(hint), g.upload(a), g.upload(b), g.alloc(2 * batch)
        for s in ((False, True) if both_s else (False,)):
            gout.fill_uniform(77 + s)                             # no word of an earlier run survives in the result buffer
            g.ct_mul_relin(ghint, ga, gb, gout, batch, s_pre=_minus_one(qs) if s else None)
            got = gout.download()
            check_pairs(got, want[s], qs, f"{opts} s_minus_one={s}")
            if not opts:
                control = got
            if "ks_map" in opts and 8 % L:
                assert L in (3, 5) and np.array_equal(got, control), "ks_map = 1 is not ignored where L does not divide 8"
    assert control is not None


# ---- B. PT2CT's whole mul_ -------------------------------------------------------------------------------------------------------------
def rescale_kernel(logn, qs_h, l_out, opts, pow_out=False):
    """The closing modSwitch's kernel by OP_RESCALE_OUT's rule (run_call) and fill_drop_tab's `balanced`: 'half' (k_rescale_drop_half +
    k_rescale_keep_half), 'lin' (k_rescale_out_lin) or 'out' (k_rescale_out)."""
    source_has("const bool lin_serves = c.drop.ddn == 1 || (c.drop.ddn == 2 && c.drop.balanced);",
               "if (!c.pow_out && c.opts.rs_lin && (c.opts.rs_half || !lin_serves)) {", "if ((qu - 1) / 2 >= qt) d.balanced = 0;",
               "const unsigned grid = nitems < c.stash_slots ? nitems : c.stash_slots;", "const unsigned nitems = (unsigned)(c.nct * 2);",
               "const unsigned grp = blockIdx.x / (8u * (unsigned)Lo), rem = blockIdx.x % (8u * (unsigned)Lo);",
               "const size_t item = (size_t)grp * 8u + (rem & 7u);            // 2 ct + component")
    ddn = len(qs_h) - l_out
    drop_bal = all((qs_h[u] - 1) // 2 < qs_h[t] for u in range(ddn) for t in range(u + 1, len(qs_h)))
    lin_serves = ddn == 1 or (ddn == 2 and drop_bal)
    if logn == 15 and not pow_out and (opts.get("rs_half") or not lin_serves):
        return "half"
    return "lin" if not pow_out and lin_serves else "out"


# what each row's closing modSwitch must reach: (kernel at n = 2^11, kernel at n = 2^15, ddn, Lo)
FULL_REACHES = {"top-4-5-3": ("lin", "lin", 2, 3), "b30-4-5-3": ("lin", "lin", 2, 3), "mixed-4-5-3": ("out", "half", 2, 3),
                "top-7-8-5": ("out", "half", 3, 5), "top-3-4-1": ("out", "half", 3, 1), "top-4-5-4-half": (None, "half", 1, 4)}
FULL_CASES = ([(row, logn, BATCH) for row, spec in FULL_ROWS.items() for logn in spec[6]]
              + [("mixed-4-5-3", 11, 5), ("mixed-4-5-3", 15, 5)])         # 10 rescale items: 8 + 2


@pytest.mark.parametrize("row,logn,batch", FULL_CASES, ids=[f"{c[0]}-logn{c[1]}-batch{c[2]}" for c in FULL_CASES])
def test_ct_mul_full_item_walks(oracle_lib, row, logn, batch):
    """The key switch behind modSwitch up (UP instantiations) on five workgroups and the closing modSwitch on three, against default
    grids and the oracle (module docstring, B).  2 * batch rescale items: 18 = 8 + 8 + 2 or 10 = 8 + 2."""
    import alchemy_amd as A
    from alchemy_amd import capi
    qs_h, l_in, l_out, row_opts, bal, q30, _ = FULL_ROWS[row]
    n, L = 1 << logn, len(qs_h)
    qs_in, qs_out = qs_h[L - l_in:], qs_h[L - l_out:]
    assert (is_balanced(qs_h), is_q30(qs_h)) == (bal, q30) and L - l_in == 1        # dup = 1
    serves = rescale_kernel(logn, qs_h, l_out, row_opts)
    assert (serves, L - l_out, l_out) == (FULL_REACHES[row][logn == 15],) + FULL_REACHES[row][2:]
    walk = {"ks_grid": 5, "rs_slots": 3}
    assert_walks(walk, batch, L, logn)
    if serves != "half":
        assert walk["rs_slots"] < 2 * batch and 3 * walk["rs_slots"] <= 2 * batch
    else:
        assert 2 * batch > 8 and (2 * batch) % 8 == 2                              # k_rescale_keep_half: a ragged last group of items
    rng = np.random.default_rng(6300 + 16 * logn + 4 * L + l_out + batch)
    hint = alternating_words(rng, 2 * L, 1, n, qs_h)
    a, b = alternating_words(rng, batch, 2, n, qs_in), alternating_words(rng, batch, 2, n, qs_in)
    assert_distinct(a, b, batch)
    hints = list(hint)
    s_pre = _minus_one(qs_in) if batch == 5 else None
    want = per_ciphertext(lambda ct: oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, hints, a[2 * ct], a[2 * ct + 1], b[2 * ct],
                                                     b[2 * ct + 1], s_pre=s_pre), batch)
    for opts in ({}, walk):
        rings = A.Ring(2 * n, qs_in), A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_out)     # a refusal raises: the test fails
        for r in rings:
            assert r.word_bytes == 4
            for k, v in dict(row_opts, **opts).items():
                r.set_option(k, v)
        rin, rh, rout = rings
        gout = rout.alloc(2 * batch)
        gout.fill_uniform(78)
        capi.ct_mul_full(rh.hint_load(hint), rin.upload(a), rin.upload(b), gout, batch, s_pre=s_pre)     # a status other than OK raises
        check_pairs(gout.download(), want, qs_out, f"{row_opts} {opts}")


# ---- C. n = 2^16 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", [("TOP17_3", BATCH), ("TOP17_8", 2)])
def test_ct_mul_relin_n65536_item_groups(oracle_lib, name, batch):
    """k_tensor_crtinv_split + k_ks_accum_split<FROM_OPS> (split_fused = 2, the default) and the composed form around k_ks_accum_split
    (split_fused = 1): a second group of eight ciphertexts that holds one, and eight limbs."""
    import alchemy_amd as A
    source_has("const unsigned grp = blockIdx.x / per, rem = blockIdx.x % per, which = rem >> 3;", "if (ct >= nct) return;")
    qs = SPLIT_RINGS[name]
    n, L = 1 << 16, len(qs)
    assert is_balanced(qs) and not is_q30(qs)
    o = oracle_lib.Ring(n, qs)
    rng = np.random.default_rng(6500 + L)
    hint = alternating_words(rng, 2 * L, 1, n, qs)
    a, b = alternating_words(rng, batch, 2, n, qs), alternating_words(rng, batch, 2, n, qs)
    assert_distinct(a, b, batch)
    hints = list(hint)
    s_pre = _minus_one(qs) if L == 8 else None
    want = per_ciphertext(lambda ct: o.ct_mul_relin(hints, a[2 * ct], a[2 * ct + 1], b[2 * ct], b[2 * ct + 1], s_pre=s_pre), batch)
    for fused in (2, 1):
        g = A.Ring(2 * n, qs)
        assert g.word_bytes == 4
        g.set_option("split_fused", fused)
        gout = g.alloc(2 * batch)
        gout.fill_uniform(79)
        g.ct_mul_relin(g.hint_load(hint), g.upload(a), g.upload(b), gout, batch, s_pre=s_pre)
        check_pairs(gout.download(), want, qs, f"split_fused={fused}")
