"""GPU: what a resident-batch call writes, and nothing beyond (include/alchemy_hip.h, alch_buf_view).

Every range of one ring that a call takes is a view (alch_buf_view) of ONE parent buffer uploaded from uniform host words (never all
zero: a stray reduced word still differs).  Before the first range, between any two and after the last lie MARGIN = 3 elements: one
quadratic ciphertext, the most any call here writes for one extra batch item.  Views start at element offsets >= 1 and where the
entry point takes a `first` / `pub_index` of its own that is >= 1 as well, so both offsets add up.

An accepted row asserts (a) the written range bit for bit against the reference -- Python integers for the element-wise calls, the C
restatement (oracle_lib) for transforms and key switches, as the family's parity file does -- (b) assert_reduced on it and (c)
assert_parent_unchanged with exactly the written spans: every margin and every input range still holds the uploaded words.
A refused row gives a count one larger than a view holds (the parent has room behind it: the margin), or a call offset that moves
the range one element past the view's end: ALCH_E_INVALID, parent as uploaded.  No row passes a range that leaves its parent; an
over-long store therefore lands in a margin or a neighbouring operand and fails a comparison.

Families, the kernels their rows reach and how that is established:

  1. test_elementwise / test_elementwise_refused      alch_buf_mul / _add / _sub (k_pointwise<W, OP>, k_pointwise_scalar), alch_buf_scale
     (k_scale<W, VW>), alch_buf_mul_public (k_mul_bcast), alch_buf_add_public (k_add_bcast), alch_ct_add_public (k_scale_add_bcast<W, VW>),
     alch_buf_copy (a device copy), alch_buf_checksum_at (k_checksum; reads only -- alch_buf_checksum is not called: it is the same
     buf_checksum with first = 0 and the whole handle).  Rings: index 9 (n = 6: n % 4 != 0, the one-word
     forms), index 45 (n = 24: 16-byte packs), index 32 on two primes below 2^62 (8-byte words, packs of two).  Two sizes per ring:
     2 elements (fewer than 256 items: one partial workgroup) and the smallest even count whose vector items exceed EW_BLOCKS * EW_THREADS
     and are no multiple of EW_THREADS (the grid-stride walk wraps and ends ragged); alch_buf_add_public walks the c0 words only and takes
     twice the count that makes that walk wrap.  Every row asserts the item count of its own launch (assert_walk).  EW_BLOCKS,
     EW_THREADS and the pack widths are read from ew_grid, ALCH_LAUNCH_VW and Vec4 in the sources (source_constants), so a retune
     names the rows to move.
  2. test_transforms      alch_buf_crt / _crtinv with first = 1 on a view at offset 3, count 3: log n = 4 and 11 (k_crt), 15 at 4-byte words
     (k_crt_half by default, k_crt with crt_half 0: run_call's `if constexpr` on (word, LOGN) and opts.crt_half), 16 (split_ring: log n > 15 at
     4-byte words; asserted from the source), 14 at 8-byte words (k_crt_half / k_crt), 15 at 8-byte words (split_ring: log n > 14), and
     the general engine at index 45, 53760 (phi = 12288) and 21609 (phi = 12348, the first size above the fused key switch's bound).
  3. test_mul_relin       alch_ct_mul_relin, two-power: n = 2^11 (k_tensor_intt<11> + k_ks_accum_half<11>), n = 2^15 (k_tensor_intt_split
     with ti_split 1 and 7, k_tensor_intt<15> with ti_split 0; k_ks_accum_half<15>), q30 rings (the Harvey instantiations: c.q30 &&
     c.balanced) and rings above 2^30, n = 2^16 at 4-byte and 2^15 at 8-byte words (split_ring: split_fused 2, 1, 0), n = 2^14 at 8-byte
     words (k_tensor_intt<14, u64> + k_ks_accum).  Batch 3 with the default grids (every grid larger than the item count; the key-switch
     grid is rounded up to groups of 8 ciphertexts, so out comes FIRST in the parent and 16 elements behind its start still lie inside).
     Batch 11 with chunk 8 -> chunks of 8 and 3 (do_mul_relin rounds the chunk up to a multiple of 8, so a batch of 5 is ONE chunk),
     with ks_grid 5, ti_grid 3 / ti_split 7 below the item count and not dividing it.  CRT and Pow flags; BaseBGad 2 at n = 2^11
     (do_mul_relin_unfused); ALCH_POW_IN | ALCH_POW_OUT at n = 2^11, 2^15, 2^16 and at n = 2^14 on 8-byte words.
     The general engine, batch 5: index 53760 (phi = 12288 = GEN_KS_T * GEN_KS_NPT, read from kernel_gen.hpp: the largest size of
     the two fused launches, gen_ks_fused) with gen_fused 1 and 0, index 21609 (phi = 12348, the first composed size), index 53760 on
     8-byte words (never fused); scratch_mib 1 cuts the composed walk into chunks of 2, 2, 1 (asserted from ks_stage_plan's
     element count).
  4. test_ct_mul, test_key_switch_quad       alch_ct_mul (k_ct_tensor3<W, VW>) at n = 2^11 and 2^15, and with ALCH_POW_IN | ALCH_POW_OUT and
     scratch_mib 1 on a one-limb n = 2^15 ring: do_ct_mul's chunk is (1 MiB) / (4 elements of 128 KiB) = 2, batch 3 leaves a ragged last
     chunk of 1.  alch_ct_key_switch_quad always runs the composed stage (do_key_switch_quad: k_ct_split3, crtInv, k_decompose_triv,
     crt, k_hint_mac), in chunks of scratch_mib / (2 + L elements): 16 + 3 ciphertexts at n = 2^11, one at a time at n = 2^15.  Both
     calls on 8-byte words at n = 2^14 and 2^15 (k_ct_tensor3<u64, 2>, k_ct_split3<u64, 2>, the u64 composed stage whole and split).
  4b. test_mul_full       alch_ct_mul_full: do_mul_full (n = 2^11, 2^15: the fused pair and the closing modSwitch -- k_rescale_out_lin<., 1>
     and <., 2> for one and two balanced dropped limbs, k_rescale_out with rs_lin 0, k_rescale_drop_half + k_rescale_keep_half with
     rs_half 1; batch 11 with chunk 8 and rs_slots 3 below the 2 * nct items), do_mul_full_unfused (n = 2^16, and 2^15 at 8-byte words;
     one ciphertext per chunk under scratch_mib 1), mul_full_base2 at n = 2^11; operands and result on one suffix ring where L_in = L_out;
     do_mul_full<u64> at n = 2^14 (batch 3, and batch 11 with chunk 8 and rs_slots 3); ALCH_POW_OUT at n = 2^11, 2^15, 2^16 and 2^14 (u64).
     test_mul_full_general: the same entry point on indices 53760 (rs_lin 1 and 0) and 45, batch 5.  Families 4 and 4b also run on
     indices 45 and 53760 (alch_ct_mul and alch_ct_key_switch_quad with g in the product).
  4c. test_mod_switch     do_mod_switch's two chunk walks, each entered: the limb-at-a-time one (two-power rings; general rings with
     rs_lin 0) with 9 = 7 + 2 linear and 5 = 4 + 1 quadratic ciphertexts at n = 2^11 and one per chunk at n = 2^15, the CRT-resident
     one (general rings, rs_lin 1) with 11 = 10 + 1 at phi = 12288; one and two limbs dropped, degree 1 and 2, and up (k_rescale_up).
  4d. test_tunnel         25 -> 15 (private E' ring, pieces_ok) under the five option sets and with BaseBGad 2, 8 -> 12 (no E' ring),
     38400 -> 25600 under scratch_mib 1 (chunks of 2, 2, 1), 64 -> 32 with both gadgets and 2^12 -> 2^13 under scratch_mib 1 (11 = 8 + 3);
     whether a pair may have the E' ring is asserted from alch_tunnel_create's condition, pieces_ok is what
     tests/test_tunnel_table_host.py asserts for the same pair.  Every scratch_mib row restates its walk's bytes per ciphertext and
     asserts (source_has) that the restated expression, the walk's call of scratch_chunk and that rule's body (scratch_plan.hpp) still
     stand in the sources.
  4e. test_decrypt_side   alch_ct_error_term, alch_buf_lift, alch_ct_decrypt_lift: degree 1 and 2, L = 1, 3, 8, n = 32 (a wavefront per
     element), 256 and 2048 (a workgroup per element), index 45; batch 5 and 3.
  4f. test_between_index_methods      alch_buf_embed / _twace on the three bases and alch_buf_coeffs for (9, 45) and (32, 96).
  4g. test_pt_mul, test_pt_eval_lin, test_pt_rescale_and_add_bcast    n % 4 = 0 and != 0; scratch_mib 1 with 37 = 16 + 16 + 5 elements.
  4h. test_gauss_dec_and_ct_encrypt, test_ks_hint     indices 21 and 64, every offset argument >= 1, the hint cut inside a value.
  1b. test_ct_add, test_general_index_ops, test_rescale_building_blocks, test_walks_of_their_own_wrap     alch_ct_add at both sizes of
     family 1.  At the wrapping size, against Python integers, on indices 9 and 45, on 8-byte words at index 32 and (for g) index 45:
     alch_buf_rescale_drop0 (k_rescale_drop0, count * (L - 1) * n words), alch_buf_rescale_add0 (k_rescale_add0), alch_buf_add_bcast
     (k_pt_add_bcast<W, VW> on a CRT ring), alch_buf_mulg and alch_buf_divg on the CRT basis (k_mul_table) and alch_buf_tensor_op with
     ALCH_T_MULG_CRT (a device copy, then buf_mulg_divg).  At a few elements, against the C restatement: alch_buf_l / _linv and
     alch_buf_mulg / _divg on Pow and Dec, alch_buf_tensor_op's other ops, alch_buf_decompose_triv, and the rescale blocks once more.
  5. test_view_free_is_not_pooled, test_pool_reuse_leaves_a_queued_view_call_alone       alch_buf_free on a view; the ring's buffer pool.

Left out, none for leaving a parent:
  - alch_buf_l / _linv, alch_buf_mulg / _divg on Pow and Dec and alch_buf_tensor_op with ALCH_T_L / _LINV / _MULG_POW / _MULG_DEC / _DIVG_* at
    the wrapping size: do_columns launches one workgroup per limb-polynomial (npoly = count * L from first_poly), not ew_grid; no
    count changes the shape of that launch below 2^30 / L elements, and the reference is one C-restatement call per element.
  - alch_buf_tensor_op with ALCH_T_CRT / _CRTINV at other sizes than index 9 and 45: it calls do_crt as alch_buf_crt (family 2) does.
  - alch_buf_decompose_triv at a wrapping size: one source element per call, L * L * n items; they pass 2048 * 256 only for L^2 n > 2^19.
  - ALCH_POW_IN / ALCH_POW_OUT of alch_ct_mul_relin on general indices; alch_ct_mul_full with L_out = L (no closing modSwitch).
Deviations from the issue's table: batch 5 with chunk 8 is ONE chunk (the chunk is rounded up to 8 ciphertexts), so the chunked rows
use 11 = 8 + 3; split_fused 2 / 1 / 0 is read by the split rings only (split_ring: log n > 15 at 4-byte, > 14 at 8-byte words), so
those rows stand at n = 2^16 and at n = 2^15 on 8-byte words, not at n = 2^15 on 4-byte words."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import CFG3_QS, Q30_QS, ROOT
from helpers import assert_parent_unchanged, assert_reduced, carve, oracle_mul_relin_base2, primes_below

pytestmark = pytest.mark.gpu

CSRC = os.path.join(ROOT, "alchemy_amd", "csrc")
MARGIN = 3
Q62_16 = [1152921504606584833, 1152921504598720513]          # = 1 mod 2^16, 60-bit: the 8-byte rings at n = 2^14 and 2^15
QS_17 = [2147352577, 2146959361]                             # = 1 mod 2^17: n = 2^16


def gapped(counts, margin=MARGIN):
    """([(first, count)], total): ranges with `margin` elements before the first, between any two and after the last."""
    spans, at = [], margin
    for c in counts:
        spans.append((at, c))
        at += c + margin
    return spans, at


def words(seed, count, n, qs):
    """(count, n, L) uniform residues; no element is zero everywhere."""
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2))
    assert all(e.any() for e in x)
    return x


def cut(host, span):
    return host[span[0]:span[0] + span[1]]


def refuse(call, parents):
    """ALCH_E_INVALID, and every parent (buffer, host words) as uploaded."""
    from alchemy_amd import capi
    with pytest.raises(capi.AlchemyError) as err:
        call()
    assert err.value.code == capi.ALCH_E_INVALID, str(err.value)
    for parent, host in parents:
        assert_parent_unchanged(parent, host)


@functools.lru_cache(maxsize=None)
def source_constants():
    """ew_grid's cap and workgroup size, the pack widths and split_ring's bounds, read from the sources."""
    lib = open(os.path.join(CSRC, "alchemy_hip.hip")).read()
    eng = open(os.path.join(CSRC, "ntt_engine.hpp")).read()
    body = lib[lib.index("static inline unsigned ew_grid(size_t items) {"):]
    body = body[:body.index("\n}\n")]
    (add, per), = re.findall(r"size_t g = \(items \+ (\d+)\) / (\d+);", body)
    (cap, cap2), = re.findall(r"if \(g > (\d+)\) g = (\d+);", body)
    assert int(add) + 1 == int(per) and cap == cap2
    assert "dim3(ew_grid((items) / VL_)), dim3(%s)" % per in lib and "dim3(ew_grid(items)), dim3(%s)" % per in lib      # ALCH_LAUNCH_VW
    assert "if ((ringp)->n % VL_ == 0)" in lib
    lanes = {4: int(re.findall(r"struct Vec4<u32> \{.*LANES = (\d+);", eng)[0]), 8: int(re.findall(r"struct Vec4<u64> \{.*LANES = (\d+);", eng)[0])}
    (s4, s8), = re.findall(r"static inline bool split_ring\(const alch_ring\* r\) \{ return r->logn > \(r->word == 4 \? (\d+) : (\d+)\); \}", lib)
    return {"blocks": int(cap), "threads": int(per), "lanes": lanes, "split_above": {4: int(s4), 8: int(s8)}}


@functools.lru_cache(maxsize=None)
def lib_source():
    return open(os.path.join(CSRC, "alchemy_hip.hip")).read() + open(os.path.join(CSRC, "scratch_plan.hpp")).read()


# the one rule every walk's chunk comes from (scratch_plan.hpp); the rows pin their walk's call of it and its bytes per item
SCRATCH_CHUNK = ("inline size_t scratch_chunk(size_t budget_bytes, size_t batch, size_t per_item_bytes) {\n"
                 "    return std::min(batch, std::max<size_t>(1, budget_bytes / per_item_bytes));\n}")


def source_has(*expressions):
    """The chunk sizes below restate what the library computes; each restated expression must still stand in the source, so that a
    retune of a walk's scratch per ciphertext fails here and names the rows to resize."""
    for e in (SCRATCH_CHUNK,) + expressions:
        assert e in lib_source(), e


KS_STAGE_ELEMS = "s.elems = (have_c2 ? 0 : 2) + (s.no_digits ? 0 : s.D);"             # ks_stage_plan: c2 in both bases, the digits


# ---- 1. element-wise walks ----------------------------------------------------------------------------------------------------------
EW_RINGS = {"G9": (9, 1 << 31, 4, 6), "G45": (45, 1 << 31, 4, 24), "W8": (32, 1 << 62, 8, 16)}
# 8-byte words on a general index: the calls that multiply by g launch nothing on a two-power one
WALK_RINGS = dict(EW_RINGS, G45W8=(45, 1 << 62, 8, 24))


@functools.lru_cache(maxsize=None)
def ew_ring(name):
    import alchemy_amd as A
    m, hi, word, n = WALK_RINGS[name]
    qs = primes_below(m, 2, hi)
    ring = A.Ring(m, qs)
    assert (ring.word_bytes, ring.n, ring.L) == (word, n, 2), name
    return ring, qs


def wrap_count(per_elem, even=False):
    """The smallest (even) element count at which every walk of the call -- `per_elem` lists its items per element, one figure per
    launch form -- exceeds the EW_BLOCKS * EW_THREADS grid (the grid-stride loop wraps) and is no multiple of EW_THREADS (it ends
    ragged)."""
    c = source_constants()
    full = c["blocks"] * c["threads"]
    count = full // min(per_elem) + 1
    while (even and count % 2) or any(count * p % c["threads"] == 0 for p in per_elem):
        count += 1
    assert all(count * p > full for p in per_elem)
    return count


def ew_pack(ring):
    """Words per item of the ALCH_LAUNCH_VW kernels and of k_pointwise on this ring."""
    vl = source_constants()["lanes"][ring.word_bytes]
    return vl if ring.n % vl == 0 else 1


def ew_count(name, size, op=None):
    """Elements per range: 2 (fewer items than one workgroup), or the smallest even count whose items wrap the grid and end ragged --
    both as vector items (the ALCH_LAUNCH_VW kernels, k_pointwise) and as single words (k_mul_bcast, k_checksum).  alch_buf_add_public
    walks the words of the c0 components only, half the range's: its rows take twice the count that makes THAT walk wrap."""
    c = source_constants()
    ring, _ = ew_ring(name)
    pack = ew_pack(ring)
    assert pack == {"G9": 1, "G45": 4, "W8": 2, "G45W8": 2}[name]
    words_per = ring.n * ring.L
    if size == "small":
        assert 2 * words_per < c["threads"]
        return 2
    if op == "add_public":
        return 2 * wrap_count([words_per])
    count = wrap_count([words_per // pack, words_per], even=True)
    assert count * words_per // pack < 2 * c["blocks"] * c["threads"]          # the walk wraps once; the second round is partial
    return count


def assert_walk(items, size):
    """The item count of one launch, as the entry point computes it: below one workgroup, or past the grid and ragged."""
    c = source_constants()
    if size == "small":
        assert 0 < items < c["threads"], items
    else:
        assert items > c["blocks"] * c["threads"] and items % c["threads"], items


def ints(a, qs):
    """Residues below 2^31 multiply inside int64; 8-byte rings go through Python integers."""
    return np.asarray(a).astype(object) if max(qs) >= (1 << 31) else np.asarray(a)


def qvec(vals, qs):
    return np.array([int(v) for v in vals], dtype=object if max(qs) >= (1 << 31) else np.int64)


def i64(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64))


def half(qs):
    return [(q + 1) // 2 for q in qs]


class EwCase:
    """Parent = margin, X, margin, Y, margin, D, margin (count elements each); the public element is Y's second one, given by its
    index in the parent."""

    def __init__(self, name, size, seed, op=None):
        self.ring, self.qs = ew_ring(name)
        self.count = ew_count(name, size, op)
        (self.xs, self.ys, self.ds), total = gapped([self.count] * 3)
        self.host = words(seed, total, self.ring.n, self.qs)
        self.pub = self.ys[0] + 1
        self.fresh()

    def fresh(self):
        """A new upload and new views."""
        self.parent, (self.x, self.y, self.d) = carve(self.ring, self.host, self.xs, self.ys, self.ds)

    def words(self, elems): return elems * self.ring.n * self.ring.L
    def packs(self, elems): return self.words(elems) // ew_pack(self.ring)

    def X(self): return ints(cut(self.host, self.xs), self.qs)
    def Y(self): return ints(cut(self.host, self.ys), self.qs)
    def D(self): return ints(cut(self.host, self.ds), self.qs)
    def P(self): return ints(self.host[self.pub], self.qs)
    def q(self): return qvec(self.qs, self.qs)
    def s(self): return qvec(half(self.qs), self.qs)


def _ct_add_public_ref(c):
    out = c.X() * c.s() % c.q()
    out[0::2] = (out[0::2] + c.P()) % c.q()
    return out


def _add_public_ref(c):
    return (c.D()[0::2] + c.P()) % c.q()


# name -> (run(case, count), reference(case) on the whole written range, written spans(case), the launch's items(case) as the entry
# point computes them -- None where no kernel walks: alch_buf_copy is a device copy)
whole_d = lambda c: [c.ds]
packs = lambda c: c.packs(c.count)
EW_OPS = {
    "mul": (lambda c, k: c.d.mul(c.x, c.y, k), lambda c: c.X() * c.Y() % c.q(), whole_d, packs),
    "add": (lambda c, k: c.d.add(c.x, c.y, k), lambda c: (c.X() + c.Y()) % c.q(), whole_d, packs),
    "sub": (lambda c, k: c.d.sub(c.x, c.y, k), lambda c: (c.X() - c.Y()) % c.q(), whole_d, packs),
    "scale": (lambda c, k: c.d.scale(c.x, k, half(c.qs)), lambda c: c.X() * c.s() % c.q(), whole_d, packs),
    "mul_public": (lambda c, k: c.d.mul_public(c.x, c.parent, c.pub, k), lambda c: c.X() * c.P() % c.q(), whole_d, lambda c: c.words(c.count)),
    "ct_add_public": (lambda c, k: c.d.ct_add_public(c.x, k // 2, half(c.qs), c.parent, c.pub), _ct_add_public_ref, whole_d, packs),
    # in place on D, the c0 components (even elements) only
    "add_public": (lambda c, k: c.d.add_public(c.parent, c.pub, k // 2), _add_public_ref,
                   lambda c: [(c.ds[0] + 2 * i, 1) for i in range(c.count // 2)], lambda c: c.words(c.count // 2)),
    # count - 1 elements from X[1:] to D[1:]: both offsets >= 1 on views at offsets >= 1
    "copy": (lambda c, k: c.d.copy_from(c.x, k - 1, dst_first=1, src_first=1), lambda c: c.X()[1:], lambda c: [(c.ds[0] + 1, c.count - 1)],
             lambda c: None),
}


@pytest.mark.parametrize("op", list(EW_OPS))
@pytest.mark.parametrize("size", ["small", "wrap"])
@pytest.mark.parametrize("name", list(EW_RINGS))
def test_elementwise(name, size, op):
    """One element-wise call on views X, Y -> D of a gapped parent: D's written elements equal Python integers, every other word of the
    parent (X, Y, the margins, the c1 components alch_buf_add_public leaves alone) is as uploaded."""
    c = EwCase(name, size, 100 + len(op), op)
    run, ref, written, items = EW_OPS[op]
    if items(c) is not None:
        assert_walk(items(c), size)
    run(c, c.count)
    spans = written(c)
    got = assert_parent_unchanged(c.parent, c.host, spans)
    keep = np.zeros(len(c.host), dtype=bool)
    for f, k in spans:
        keep[f:f + k] = True
    want = i64(ref(c))
    assert_reduced(want, c.qs)
    assert want.shape == got[keep].shape and np.array_equal(got[keep], want), (name, size, op)
    assert_reduced(got[keep], c.qs)


@pytest.mark.parametrize("op", list(EW_OPS))
@pytest.mark.parametrize("name", list(EW_RINGS))
def test_elementwise_refused(name, op):
    """count + 1 elements (one more ciphertext for the ciphertext calls) on views of `count`: refused although the parent has the room;
    and for alch_buf_copy an offset one further with the count that just fitted."""
    c = EwCase(name, "small", 200 + len(op))
    run = EW_OPS[op][0]
    refuse(lambda: run(c, c.count + (2 if "public" in op and op != "mul_public" else 1)), [(c.parent, c.host)])
    if op == "copy":
        refuse(lambda: c.d.copy_from(c.x, c.count - 1, dst_first=2, src_first=1), [(c.parent, c.host)])
        refuse(lambda: c.d.copy_from(c.x, c.count - 1, dst_first=1, src_first=2), [(c.parent, c.host)])
    if "public" in op:                                                   # the public element's index one past its buffer's end
        pub = c.parent.view(c.ys[0], c.count)
        calls = {"mul_public": lambda: c.d.mul_public(c.x, pub, c.count, c.count),
                 "ct_add_public": lambda: c.d.ct_add_public(c.x, c.count // 2, half(c.qs), pub, c.count),
                 "add_public": lambda: c.d.add_public(pub, c.count, c.count // 2)}
        refuse(calls[op], [(c.parent, c.host)])


@pytest.mark.parametrize("size", ["small", "wrap"])
@pytest.mark.parametrize("name", list(EW_RINGS))
def test_checksum_reads_its_range_only(name, size):
    """alch_buf_checksum_at over elements [1, count) of the view X equals the sum over a separate copy of those elements at the same
    position; the parent is as uploaded; a first one further with the same count is refused."""
    c = EwCase(name, size, 300)
    assert_walk(c.words(c.count - 1), size)
    sep = c.ring.upload(cut(c.host, c.xs)[1:])
    assert c.x.checksum(1, c.count - 1, position=5) == sep.checksum(0, c.count - 1, position=5)
    assert c.x.checksum(1, c.count - 1, position=5) != c.x.checksum(0, c.count - 1, position=5)
    assert_parent_unchanged(c.parent, c.host)
    refuse(lambda: c.x.checksum(2, c.count - 1), [(c.parent, c.host)])
    refuse(lambda: c.x.checksum(0, c.count + 1), [(c.parent, c.host)])


@pytest.mark.parametrize("size", ["small", "wrap"])
@pytest.mark.parametrize("name", list(EW_RINGS))
def test_ct_add(name, size):
    """alch_ct_add of linear a (scaled by s_a) and quadratic b, no g-power: out = (s_a a_0 + b_0, s_a a_1 + b_1, b_2) per ciphertext
    in Python integers; out, a, b views of one gapped parent; batch + 1 refused."""
    from alchemy_amd.ctadd import ct_add_raw
    ring, qs = ew_ring(name)
    batch = ew_count(name, size)                # launch_ct_add: one item per pack of a ciphertext's element, batch * L * n / pack of them
    assert_walk(batch * ring.n * ring.L // ew_pack(ring), size)
    (outs, as_, bs), total = gapped([3 * batch, 2 * batch, 3 * batch])
    host = words(350, total, ring.n, qs)
    parent, (out, a, b) = carve(ring, host, outs, as_, bs)
    ct_add_raw(out, batch, a, 1, half(qs), 0, b, 2, None, 0)
    got = assert_parent_unchanged(parent, host, [outs])
    q, s = qvec(qs, qs), qvec(half(qs), qs)
    want = ints(cut(host, bs), qs).reshape(batch, 3, ring.n, ring.L).copy()
    want[:, :2] = (want[:, :2] + ints(cut(host, as_), qs).reshape(batch, 2, ring.n, ring.L) * s % q) % q
    assert np.array_equal(cut(got, outs), i64(want).reshape(3 * batch, ring.n, ring.L)), (name, size)
    assert_reduced(cut(got, outs), qs)
    refuse(lambda: ct_add_raw(out, batch + 1, a, 1, half(qs), 0, b, 2, None, 0), [])
    assert np.array_equal(parent.download(), got)


@pytest.mark.parametrize("name", ["G9", "G45"])
def test_general_index_ops(oracle_lib, name):
    """The in-place calls with a `first` (alch_buf_mulg / _divg on the CRT basis, alch_buf_l / _linv) on elements [1, 3) of a
    three-element view at offset 3, alch_buf_tensor_op between two views (dst_first = src_first = 1) and alch_buf_decompose_triv with the
    source given by its index in the parent: against the C restatement; every other element as uploaded; a range one element past a
    view's end is refused.  alch_buf_mulg on the CRT basis once more at the wrapping size (k_mul_table), against x times crt(g)."""
    from alchemy_amd import capi
    ring, qs = ew_ring(name)
    o = oracle_lib.GenRing(ring.m, qs)
    (vs, ws), total = gapped([3, 3 + ring.L])
    host = words(360 + ring.n, total, ring.n, qs)
    written = (vs[0] + 1, 2)
    src = cut(host, written)
    inplace = [("mulg", lambda v, f, k: v.mulg(capi.ALCH_BASIS_CRT, f, k), o.mulg_crt), ("l", lambda v, f, k: v.l(f, k), o.l),
               ("linv", lambda v, f, k: v.linv(f, k), o.linv), ("mulg_pow", lambda v, f, k: v.mulg(capi.ALCH_BASIS_POW, f, k), o.mulg_pow),
               ("mulg_dec", lambda v, f, k: v.mulg(capi.ALCH_BASIS_DEC, f, k), o.mulg_dec)]
    for what, run, ref in inplace:
        parent, (v,) = carve(ring, host, vs)
        run(v, 1, 2)
        got = assert_parent_unchanged(parent, host, [written])
        assert np.array_equal(cut(got, written), np.stack([ref(e) for e in src])), (name, what)
        assert_reduced(cut(got, written), qs)
        refuse(lambda: run(v, 2, 2), [])
        refuse(lambda: run(v, 1, 3), [])
        assert np.array_equal(parent.download(), got)
    # alch_buf_divg on the CRT basis: of g x, so that it divides
    gx = host.copy()
    gx[written[0]:written[0] + 2] = np.stack([o.mulg_crt(e) for e in src])
    parent, (v,) = carve(ring, gx, vs)
    assert v.divg(capi.ALCH_BASIS_CRT, 1, 2) is True
    got = assert_parent_unchanged(parent, gx, [written])
    assert np.array_equal(cut(got, written), src), name
    refuse(lambda: v.divg(capi.ALCH_BASIS_CRT, 2, 2), [])
    assert np.array_equal(parent.download(), got)
    # alch_buf_tensor_op: view ws[1:3] = op(view vs[1:3])
    dst_written = (ws[0] + 1, 2)
    for op, ref in ((capi.ALCH_T_CRT, o.crt), (capi.ALCH_T_L, o.l), (capi.ALCH_T_MULG_CRT, o.mulg_crt)):
        parent, (v, w) = carve(ring, host, vs, ws)
        assert w.tensor_op(v, op, count=2, dst_first=1, src_first=1) is True
        got = assert_parent_unchanged(parent, host, [dst_written])
        assert np.array_equal(cut(got, dst_written), np.stack([ref(e) for e in src])), (name, op)
        refuse(lambda: w.tensor_op(v, op, count=2, dst_first=1, src_first=2), [])
        refuse(lambda: w.tensor_op(v, op, count=3 + ring.L, dst_first=1, src_first=0), [])
        assert np.array_equal(parent.download(), got)
    # alch_buf_decompose_triv: L digits into ws[1 : 1 + L] from the parent's element vs[0] + 1
    parent, (w,) = carve(ring, host, ws)
    parent.decompose_triv_into(vs[0] + 1, w, 1)
    got = assert_parent_unchanged(parent, host, [(ws[0] + 1, ring.L)])
    assert np.array_equal(cut(got, (ws[0] + 1, ring.L)), np.stack(o.decompose_triv(host[vs[0] + 1]))), name
    refuse(lambda: parent.decompose_triv_into(vs[0] + 1, w, 4), [])
    refuse(lambda: w.decompose_triv_into(3 + ring.L, w, 1), [])
    assert np.array_equal(parent.download(), got)
    # alch_buf_mulg on the CRT basis at the wrapping size
    count = ew_count(name, "wrap")
    (bs_,), total = gapped([count + 1])
    big = words(361 + ring.n, total, ring.n, qs)
    parent, (v,) = carve(ring, big, bs_)
    v.mulg(capi.ALCH_BASIS_CRT, 1, count)
    wrote = (bs_[0] + 1, count)
    got = assert_parent_unchanged(parent, big, [wrote])
    g_crt = o.mulg_crt(np.ones((ring.n, ring.L), dtype=np.int64))
    assert np.array_equal(cut(got, wrote), cut(big, wrote) * g_crt % np.array(qs, dtype=np.int64)), name


@pytest.mark.parametrize("name", ["G9", "G45", "W8"])
def test_rescale_building_blocks(oracle_lib, name):
    """alch_buf_rescale_drop0 from a view of the two-limb ring's parent into a view of the one-limb ring's, and alch_buf_rescale_add0
    back: the C restatement's rescale_drop0, and (0, q_0 x) in Python integers; count + 1 refused."""
    import alchemy_amd as A
    ring, qs = ew_ring(name)
    small = A.Ring(ring.m, qs[1:])
    o = oracle_lib.GenRing(ring.m, qs) if name != "W8" else oracle_lib.Ring(ring.n, qs)
    count = 5
    (bs_, us), total = gapped([count, count])
    host = words(370 + ring.n, total, ring.n, qs)
    (ss,), total_s = gapped([count])
    host_s = words(371 + ring.n, total_s, small.n, qs[1:])
    pbig, (bv, uv) = carve(ring, host, bs_, us)
    psmall, (sv,) = carve(small, host_s, ss)
    bv.rescale_drop0_into(sv, count)
    got = assert_parent_unchanged(psmall, host_s, [ss])
    assert_parent_unchanged(pbig, host)
    assert np.array_equal(cut(got, ss), np.stack([o.rescale_drop0(e) for e in cut(host, bs_)])), name
    assert_reduced(cut(got, ss), qs[1:])
    refuse(lambda: bv.rescale_drop0_into(sv, count + 1), [(pbig, host)])
    assert np.array_equal(psmall.download(), got)
    sv.rescale_add0_into(uv, count)
    up = assert_parent_unchanged(pbig, host, [us])
    assert np.array_equal(psmall.download(), got)
    assert not cut(up, us)[:, :, 0].any()
    assert np.array_equal(cut(up, us)[:, :, 1], i64(cut(got, ss)[:, :, 0].astype(object) * qs[0] % qs[1])), name
    refuse(lambda: sv.rescale_add0_into(uv, count + 1), [])
    assert np.array_equal(pbig.download(), up)


@pytest.mark.parametrize("name", list(WALK_RINGS))
def test_walks_of_their_own_wrap(oracle_lib, name):
    """The element-wise entry points that launch a kernel of their own with a total of their own, each at a count whose items wrap
    the grid and end ragged, against Python integers: alch_buf_rescale_drop0 (count * (L - 1) * n single words) and
    alch_buf_rescale_add0 (count * L * n) between views of a two-limb and a one-limb parent, alch_buf_add_bcast (k_pt_add_bcast, packs)
    on the CRT ring with the literal given by its index in the parent, and on a general index alch_buf_divg and alch_buf_mulg on the
    CRT basis (k_mul_table, single words; first = 1) and alch_buf_tensor_op with ALCH_T_MULG_CRT (a copy, then the same launch)."""
    import alchemy_amd as A
    from alchemy_amd import capi
    from alchemy_amd.plaintext import add_bcast
    ring, qs = ew_ring(name)
    n, L = ring.n, ring.L
    q = qvec(qs, qs)
    small = A.Ring(ring.m, qs[1:])
    # alch_buf_rescale_drop0: dst = q_0^-1 (x_1 - centred(x_0)) mod q_1; alch_buf_rescale_add0 back: (0, q_0 y mod q_1)
    count = wrap_count([n * (L - 1), n * L])
    assert_walk(count * (L - 1) * n, "wrap")
    assert_walk(count * L * n, "wrap")
    (bs_, us), total = gapped([count, count])
    host = words(380 + n, total, n, qs)
    (ss,), total_s = gapped([count])
    host_s = words(381 + n, total_s, n, qs[1:])
    pbig, (bv, uv) = carve(ring, host, bs_, us)
    psmall, (sv,) = carve(small, host_s, ss)
    bv.rescale_drop0_into(sv, count)
    got = assert_parent_unchanged(psmall, host_s, [ss])
    assert_parent_unchanged(pbig, host)
    x = ints(cut(host, bs_), qs)
    z = np.where(x[:, :, 0] > (qs[0] - 1) // 2, x[:, :, 0] - qs[0], x[:, :, 0])
    want = i64((x[:, :, 1] - z) % qs[1] * pow(qs[0], -1, qs[1]) % qs[1])
    assert np.array_equal(cut(got, ss)[:, :, 0], want), name
    assert_reduced(cut(got, ss), qs[1:])
    sv.rescale_add0_into(uv, count)
    up = assert_parent_unchanged(pbig, host, [us])
    assert np.array_equal(psmall.download(), got)
    assert not cut(up, us)[:, :, 0].any()
    assert np.array_equal(cut(up, us)[:, :, 1], i64(ints(want, qs) * (qs[0] % qs[1]) % qs[1])), name
    # alch_buf_add_bcast: dst = src + the parent's element `lit`
    count = ew_count(name, "wrap")
    assert_walk(count * n * L // ew_pack(ring), "wrap")
    (ss, ds), total = gapped([count, count])
    host = words(382 + n, total, n, qs)
    parent, (src, dst) = carve(ring, host, ss, ds)
    lit = ss[0] + 1
    add_bcast(dst, src, parent, lit, count)
    got = assert_parent_unchanged(parent, host, [ds])
    assert np.array_equal(cut(got, ds), i64((ints(cut(host, ss), qs) + ints(host[lit], qs)) % q)), name
    assert_reduced(cut(got, ds), qs)
    refuse(lambda: add_bcast(dst, src, parent, lit, count + 1), [])
    refuse(lambda: add_bcast(dst, src, src, count, count), [])
    assert np.array_equal(parent.download(), got)
    if ring.m & (ring.m - 1) == 0:
        return                                                  # g = 1: buf_mulg_divg and alch_buf_tensor_op launch nothing of their own
    # k_mul_table on elements [1, 1 + count) of a view: x -> g x, back by alch_buf_divg, and g x into a second view
    o = oracle_lib.GenRing(ring.m, qs)
    g_crt = ints(o.mulg_crt(np.ones((n, L), dtype=np.int64)), qs)
    assert_walk(count * n * L, "wrap")
    (vs, ws), total = gapped([count + 1, count + 1])
    host = words(383 + n, total, n, qs)
    wrote, copied = (vs[0] + 1, count), (ws[0] + 1, count)
    gx = i64(ints(cut(host, wrote), qs) * g_crt % q)
    parent, (v, w) = carve(ring, host, vs, ws)
    v.mulg(capi.ALCH_BASIS_CRT, 1, count)
    got = assert_parent_unchanged(parent, host, [wrote])
    assert np.array_equal(cut(got, wrote), gx), name
    assert_reduced(cut(got, wrote), qs)
    assert v.divg(capi.ALCH_BASIS_CRT, 1, count) is True
    assert_parent_unchanged(parent, host)                       # g^-1 (g x) = x: the parent is as uploaded again
    refuse(lambda: v.divg(capi.ALCH_BASIS_CRT, 2, count), [(parent, host)])
    refuse(lambda: v.divg(capi.ALCH_BASIS_CRT, 1, count + 1), [(parent, host)])
    assert w.tensor_op(v, capi.ALCH_T_MULG_CRT, count=count, dst_first=1, src_first=1) is True
    got = assert_parent_unchanged(parent, host, [copied])
    assert np.array_equal(cut(got, copied), gx), name
    refuse(lambda: w.tensor_op(v, capi.ALCH_T_MULG_CRT, count=count, dst_first=2, src_first=1), [])
    assert np.array_equal(parent.download(), got)


# ---- 2. transforms --------------------------------------------------------------------------------------------------------------------
# name -> (index, moduli or (count, bound), word bytes, options)
CRT_ROWS = {
    "p4": (32, CFG3_QS[:2], 4, {}), "p11": (1 << 12, CFG3_QS[:2], 4, {}),
    "p15_half": (1 << 16, CFG3_QS[:2], 4, {"crt_half": 1}), "p15_whole": (1 << 16, CFG3_QS[:2], 4, {"crt_half": 0}),
    "p16_split": (1 << 17, QS_17, 4, {}),
    "w14_half": (1 << 15, Q62_16, 8, {"crt_half": 1}), "w14_whole": (1 << 15, Q62_16, 8, {"crt_half": 0}), "w15_split": (1 << 16, Q62_16, 8, {}),
    "g45": (45, (2, 1 << 31), 4, {}), "g53760": (53760, (2, 1 << 31), 4, {}), "g21609": (21609, (2, 1 << 31), 4, {}),
}


def make_ring(oracle_lib, m, qs, word, opts):
    """(ring, C restatement, moduli): two-power indices through oracle_lib.Ring, others through GenRing."""
    import alchemy_amd as A
    if isinstance(qs, tuple):
        qs = primes_below(m, *qs)
    ring = A.Ring(m, qs)
    assert ring.word_bytes == word
    for k, v in opts.items():
        ring.set_option(k, v)
    o = oracle_lib.Ring(m // 2, qs) if m & (m - 1) == 0 else oracle_lib.GenRing(m, qs)
    return ring, o, qs


@pytest.mark.parametrize("row", list(CRT_ROWS))
def test_transforms(oracle_lib, row):
    """alch_buf_crt and alch_buf_crtinv of elements [1, 4) of a five-element view at offset 3 of an 11-element parent: parent elements
    [4, 7) equal the C restatement, the view's first and last element and both margins are as uploaded.  first + count one past the
    view's end, by the count and by the offset, is refused."""
    m, qs, word, opts = CRT_ROWS[row]
    ring, o, qs = make_ring(oracle_lib, m, qs, word, opts)
    c = source_constants()
    logn = ring.n.bit_length() - 1
    if row.endswith("_split"):
        assert logn > c["split_above"][word]
    elif row[0] in "pw":
        assert logn <= c["split_above"][word]
    if "half" in row or "whole" in row:
        assert logn == c["split_above"][word]                           # the 128-KiB polynomial: the size with both forms
    (vs,), total = gapped([5])
    host = words(400 + len(row), total, ring.n, qs)
    for inverse in (False, True):
        parent, (v,) = carve(ring, host, vs)
        (v.crtinv if inverse else v.crt)(1, 3)
        got = assert_parent_unchanged(parent, host, [(vs[0] + 1, 3)])
        for e in range(vs[0] + 1, vs[0] + 4):
            assert np.array_equal(got[e], (o.crtinv if inverse else o.crt)(host[e])), (row, inverse, e)
        assert_reduced(got[vs[0] + 1:vs[0] + 4], qs)
        fn = v.crtinv if inverse else v.crt
        refuse(lambda: fn(1, 5), [])
        refuse(lambda: fn(3, 3), [])
        refuse(lambda: fn(0, 6), [])
        assert np.array_equal(parent.download(), got)


# ---- 3. alch_ct_mul_relin ---------------------------------------------------------------------------------------------------------------
PIECES = {"chunk": 8, "ks_grid": 5, "ti_grid": 3}
RELIN_ROWS = {
    "p11": (1 << 12, CFG3_QS[:2], 4, 3, {}, "crt"), "p11_q30": (1 << 12, Q30_QS[:2], 4, 3, {}, "crt"),
    "p11_chunks": (1 << 12, CFG3_QS[:2], 4, 11, PIECES, "crt"), "p11_pow": (1 << 12, CFG3_QS[:2], 4, 3, {}, "pow"),
    "p11_base2": (1 << 12, CFG3_QS[:2], 4, 3, {}, "base2"),
    "p15_pow": (1 << 16, CFG3_QS[:2], 4, 3, {}, "pow"), "p16_fused2_pow": (1 << 17, QS_17, 4, 3, {"split_fused": 2}, "pow"),
    "w14_pow": (1 << 15, Q62_16, 8, 3, {}, "pow"),
    "p15": (1 << 16, CFG3_QS[:2], 4, 3, {}, "crt"), "p15_q30": (1 << 16, Q30_QS[:2], 4, 3, {}, "crt"),
    "p15_whole_chunks": (1 << 16, CFG3_QS[:2], 4, 11, dict(PIECES, ti_split=0), "crt"),
    "p15_persistent": (1 << 16, CFG3_QS[:2], 4, 5, {"ti_split": 7, "ks_grid": 3}, "crt"),
    "p16_fused2": (1 << 17, QS_17, 4, 3, {"split_fused": 2}, "crt"), "p16_fused1": (1 << 17, QS_17, 4, 3, {"split_fused": 1}, "crt"),
    "p16_fused0": (1 << 17, QS_17, 4, 3, {"split_fused": 0}, "crt"),
    "w14": (1 << 15, Q62_16, 8, 3, {}, "crt"),
    "w15_fused2": (1 << 16, Q62_16, 8, 3, {"split_fused": 2}, "crt"), "w15_fused0": (1 << 16, Q62_16, 8, 3, {"split_fused": 0}, "crt"),
    # general engine, batch 5: phi = 12288 (the largest fused size) with gen_fused 1 and 0, phi = 12348 (the first composed size);
    # scratch_mib 1 cuts the composed walk (do_mul_relin_unfused) into chunks of 2, 2 and 1
    "g53760_fused": (53760, (2, 1 << 31), 4, 5, {"scratch_mib": 1}, "crt"),
    "g53760_composed": (53760, (2, 1 << 31), 4, 5, {"gen_fused": 0, "scratch_mib": 1}, "crt"),
    "g21609_composed": (21609, (2, 1 << 31), 4, 5, {"scratch_mib": 1}, "crt"),
    "g53760_w8": (53760, (2, 1 << 62), 8, 5, {"scratch_mib": 1}, "crt"),
}


def gen_ks_bound():
    """phi up to which the general key switch runs as two fused launches (gen_ks_fused), from the sources."""
    gen = open(os.path.join(CSRC, "kernel_gen.hpp")).read()
    lib = open(os.path.join(CSRC, "alchemy_hip.hip")).read()
    assert "r->n <= (u32)(GEN_KS_T * GEN_KS_NPT)" in lib
    return int(re.findall(r"constexpr int GEN_KS_T = (\d+);", gen)[0]) * int(re.findall(r"constexpr int GEN_KS_NPT = (\d+);", gen)[0])


def relin_layout(batch, n, qs, seed):
    """out first, then a and b: 16 elements (a key-switch group of 8 ciphertexts) behind out's start lie inside the parent."""
    (outs, as_, bs), total = gapped([2 * batch] * 3)
    assert outs[0] + 16 <= total
    return outs, as_, bs, words(seed, total, n, qs)


@pytest.mark.parametrize("row", list(RELIN_ROWS))
def test_mul_relin(oracle_lib, row):
    """alch_ct_mul_relin with out, a and b views of one gapped parent: out equals the C restatement, a, b and the margins are as
    uploaded; batch + 1 on views of 2 * batch elements is refused."""
    from alchemy_amd import capi
    m, qs, word, batch, opts, kind = RELIN_ROWS[row]
    ring, o, qs = make_ring(oracle_lib, m, qs, word, opts)
    c = source_constants()
    gen = m & (m - 1) != 0
    if gen:
        fused = word == 4 and ring.n <= gen_ks_bound() and opts.get("gen_fused", 1)         # gen_ks_fused
        assert bool(fused) == ("fused" in row) and (ring.n > gen_ks_bound()) == (m == 21609)
        source_has(KS_STAGE_ELEMS, "const size_t per_ct = s.elems * elem_bytes(r);",
                   "const size_t chunk = scratch_chunk(r->scratch_mib << 20, batch, per_ct);")
        chunk = (1 << 20) // ((2 + (0 if fused else ring.L)) * ring.n * ring.L * word)      # ks_stage_plan's elems, do_mul_relin_unfused's chunk
        assert (chunk >= batch) if fused else (chunk == (2 if word == 4 else 1) and batch % 2 == 1)   # 4-byte words: a ragged last chunk
    else:
        assert (ring.n.bit_length() - 1 > c["split_above"][word]) == ("fused" in row)
    if "q30" in row:
        assert max(qs) < (1 << 30)
    else:
        assert max(qs) > (1 << 30)
    if "chunk" in opts:
        assert opts["chunk"] % 8 == 0 and opts["chunk"] < batch < 2 * opts["chunk"]                      # two chunks, the last one ragged
        assert opts["ks_grid"] < 16 * ring.L and (16 * ring.L) % opts["ks_grid"] and opts["ti_grid"] < 3 * ring.L
    gadget = capi.ALCH_GAD_BASE2 if kind == "base2" else capi.ALCH_GAD_TRIV
    hint_host = words(500 + len(row), 2 * ring.gadget_digits(gadget), ring.n, qs)
    hint = ring.hint_load(hint_host, gadget)
    outs, as_, bs, host = relin_layout(batch, ring.n, qs, 501 + len(row))
    parent, (out, a, b) = carve(ring, host, outs, as_, bs)
    flags = (capi.ALCH_POW_IN | capi.ALCH_POW_OUT) if kind == "pow" else 0
    ring.ct_mul_relin(hint, a, b, out, batch, flags=flags)
    got = assert_parent_unchanged(parent, host, [outs])
    A_, B_ = cut(host, as_), cut(host, bs)
    for ct in range(batch):
        ops = (A_[2 * ct], A_[2 * ct + 1], B_[2 * ct], B_[2 * ct + 1])
        if kind == "base2":
            w0, w1 = oracle_mul_relin_base2(oracle_lib, ring.n, qs, list(hint_host), *ops)
        else:
            w0, w1 = o.ct_mul_relin(list(hint_host), *ops, **({"pow_basis": True} if kind == "pow" else {}))
        assert np.array_equal(got[outs[0] + 2 * ct], w0) and np.array_equal(got[outs[0] + 2 * ct + 1], w1), (row, ct)
    assert_reduced(cut(got, outs), qs)
    refuse(lambda: ring.ct_mul_relin(hint, a, b, out, batch + 1, flags=flags), [])
    assert np.array_equal(parent.download(), got)


# ---- 4. alch_ct_mul, alch_ct_key_switch_quad ---------------------------------------------------------------------------------------------
def tensor3(A_, B_, qs):
    """SymmSHE (*) on a two-power index (g = 1) in Python integers: (a0 b0, a0 b1 + a1 b0, a1 b1) per ciphertext."""
    q = qvec(qs, qs)
    A_, B_ = ints(A_, qs), ints(B_, qs)
    out = []
    for ct in range(len(A_) // 2):
        a0, a1, b0, b1 = A_[2 * ct], A_[2 * ct + 1], B_[2 * ct], B_[2 * ct + 1]
        out += [a0 * b0 % q, (a0 * b1 % q + a1 * b0 % q) % q, a1 * b1 % q]
    return i64(np.stack(out))


# name -> (index, moduli, batch, word bytes)
STEP_ROWS = {"p11": (1 << 12, CFG3_QS[:2], 3, 4), "p11_q30": (1 << 12, Q30_QS[:2], 3, 4), "p15": (1 << 16, CFG3_QS[:2], 3, 4),
             # 8-byte words: k_ct_tensor3<u64, 2> / k_ct_split3<u64, 2> and the u64 composed stage, whole (n = 2^14) and split (2^15)
             "w14": (1 << 15, Q62_16, 3, 8), "w15": (1 << 16, Q62_16, 3, 8),
             # general indices: (*) multiplies every product coefficient by g (the C restatement's mulg_crt)
             "g45": (45, (2, 1 << 31), 5, 4), "g53760": (53760, (2, 1 << 31), 3, 4)}


def quad_want(o, m, A_, B_, qs):
    """The quadratic ciphertexts a (x) b, times g on a general index."""
    want = tensor3(A_, B_, qs)
    return np.stack([o.mulg_crt(e) for e in want]) if m & (m - 1) else want


@pytest.mark.parametrize("row", list(STEP_ROWS) + ["p15_pow_chunks"])
def test_ct_mul(oracle_lib, row):
    """alch_ct_mul: out (3 * batch elements) first in the parent, then a and b.  p15_pow_chunks: one limb, Pow basis in and out,
    scratch_mib 1 -> do_ct_mul stages two ciphertexts at a time and the last chunk holds one."""
    from alchemy_amd import capi
    from alchemy_amd.mulsteps import ct_mul
    pow_row = row == "p15_pow_chunks"
    m, qs, batch, word = (1 << 16, CFG3_QS[:1], 3, 4) if pow_row else STEP_ROWS[row]
    ring, o, qs = make_ring(oracle_lib, m, qs, word, {"scratch_mib": 1} if pow_row else {})
    if row[0] == "w":
        assert (ring.n.bit_length() - 1 > source_constants()["split_above"][8]) == (row == "w15")
    if pow_row:
        source_has("chunk = scratch_chunk(r->scratch_mib << 20, batch, 4 * eb);")       # do_ct_mul, pow_in
        chunk = (1 << 20) // (4 * ring.n * ring.L * ring.word_bytes)
        assert chunk == 2 and batch % chunk == 1
    (outs, as_, bs), total = gapped([3 * batch, 2 * batch, 2 * batch])
    host = words(600 + len(row), total, ring.n, qs)
    parent, (out, a, b) = carve(ring, host, outs, as_, bs)
    flags = (capi.ALCH_POW_IN | capi.ALCH_POW_OUT) if pow_row else 0
    ct_mul(a, b, batch, flags=flags, out=out)
    got = assert_parent_unchanged(parent, host, [outs])
    A_, B_ = cut(host, as_), cut(host, bs)
    if pow_row:
        A_, B_ = np.stack([o.crt(e) for e in A_]), np.stack([o.crt(e) for e in B_])
    want = quad_want(o, m, A_, B_, qs)
    if pow_row:
        want = np.stack([o.crtinv(e) for e in want])
    assert np.array_equal(cut(got, outs), want), row
    assert_reduced(cut(got, outs), qs)
    refuse(lambda: ct_mul(a, b, batch + 1, flags=flags, out=out), [])
    assert np.array_equal(parent.download(), got)


# alch_ct_key_switch_quad runs the composed stage (do_key_switch_quad: k_ct_split3, crtInv, digit transforms, hint products) in chunks
# of scratch_mib / ((2 + L) elements: c2 in both bases and L digits): 16 ciphertexts at n = 2^11 and one at n = 2^15 under scratch_mib 1, two limbs
KSQ_ROWS = dict(STEP_ROWS, p11_chunks=(1 << 12, CFG3_QS[:2], 19, 4), p15_chunks=(1 << 16, CFG3_QS[:2], 3, 4))


@pytest.mark.parametrize("row", list(KSQ_ROWS))
def test_key_switch_quad(oracle_lib, row):
    """alch_ct_key_switch_quad on the quadratic ciphertexts a (x) b (Python integers), a view of 3 * batch elements behind out:
    out equals the C restatement's ct_mul_relin of a and b, the quadratic ciphertexts and the margins are as uploaded."""
    from alchemy_amd.mulsteps import key_switch_quad
    m, qs, batch, word = KSQ_ROWS[row]
    ring, o, qs = make_ring(oracle_lib, m, qs, word, {"scratch_mib": 1} if "chunks" in row else {})
    if "chunks" in row:
        # do_key_switch_quad: have_c2, so ks_stage_plan's elems are the L digits; CRT input
        source_has(KS_STAGE_ELEMS, "const size_t stage_elems = 2 + s.elems;", "const size_t per_ct = (stage_elems + (pow_in ? 3 : 0)) * eb;",
                   "const size_t chunk = scratch_chunk(r->scratch_mib << 20, batch, per_ct);")
        chunk = max(1, (1 << 20) // ((2 + ring.L) * ring.n * ring.L * 4))
        assert chunk < batch and (batch % chunk or chunk == 1) and (chunk > 1) == (row == "p11_chunks")
    hint_host = words(700 + len(row), 2 * ring.L, ring.n, qs)
    hint = ring.hint_load(hint_host)
    A_, B_ = words(701, 2 * batch, ring.n, qs), words(702, 2 * batch, ring.n, qs)
    (outs, ins), total = gapped([2 * batch, 3 * batch])
    assert outs[0] + 16 <= total
    host = words(703, total, ring.n, qs)
    host[ins[0]:ins[0] + ins[1]] = quad_want(o, m, A_, B_, qs)
    parent, (out, quad) = carve(ring, host, outs, ins)
    key_switch_quad(hint, quad, batch, out=out)
    got = assert_parent_unchanged(parent, host, [outs])
    for ct in range(batch):
        w0, w1 = o.ct_mul_relin(list(hint_host), A_[2 * ct], A_[2 * ct + 1], B_[2 * ct], B_[2 * ct + 1])
        assert np.array_equal(got[outs[0] + 2 * ct], w0) and np.array_equal(got[outs[0] + 2 * ct + 1], w1), (row, ct)
    assert_reduced(cut(got, outs), qs)
    refuse(lambda: key_switch_quad(hint, quad, batch + 1, out=out), [])
    assert np.array_equal(parent.download(), got)


# ---- 4b. alch_ct_mul_full -----------------------------------------------------------------------------------------------------------------
SIX_QS = [2147352577, 2146959361, 2146041857, 2144468993, 2142502913, 2135818241]          # = 1 mod 2^17
Q62_16x3 = Q62_16 + [1152921504597016577]
FULL_PIECES = dict(PIECES, rs_slots=3)
# name -> (log n, the hint's moduli, L_in, L_out, word, batch, options, gadget)
FULL_ROWS = {
    "f11": (11, SIX_QS[:3], 2, 2, 4, 3, {}, "triv"), "f11_chunks": (11, SIX_QS[:3], 2, 1, 4, 11, FULL_PIECES, "triv"),
    "f11_base2": (11, SIX_QS[:3], 2, 2, 4, 3, {}, "base2"), "f11_rs_lin0_chunks": (11, SIX_QS[:3], 2, 1, 4, 11, dict(FULL_PIECES, rs_lin=0), "triv"),
    "f15": (15, SIX_QS[:3], 2, 2, 4, 3, {}, "triv"), "f15_q30": (15, Q30_QS[:3], 2, 1, 4, 3, {}, "triv"),
    "f15_rs_lin0": (15, SIX_QS[:3], 2, 1, 4, 3, {"rs_lin": 0}, "triv"), "f15_rs_half": (15, SIX_QS[:3], 2, 1, 4, 3, {"rs_half": 1}, "triv"),
    "f15_chunks": (15, SIX_QS[:3], 2, 2, 4, 11, dict(FULL_PIECES, ti_split=0), "triv"),
    "f16_unfused": (16, SIX_QS[:3], 2, 1, 4, 3, {"scratch_mib": 1}, "triv"),
    "w15_unfused": (15, Q62_16x3, 2, 1, 8, 3, {"scratch_mib": 1}, "triv"),
    # 8-byte words below the split: do_mul_full<u64>, the fused pair and the k_rescale_out* closing, one and two limbs dropped
    "w14": (14, Q62_16x3, 2, 1, 8, 3, {}, "triv"), "w14_chunks": (14, Q62_16x3, 2, 2, 8, 11, FULL_PIECES, "triv"),
    # ALCH_POW_OUT: the closing writes the powerful basis (do_mul_full's pow_out; do_mod_switch's in do_mul_full_unfused)
    "f11_pow_out": (11, SIX_QS[:3], 2, 1, 4, 3, {}, "triv"), "f15_pow_out": (15, SIX_QS[:3], 2, 2, 4, 3, {}, "triv"),
    "f16_unfused_pow_out": (16, SIX_QS[:3], 2, 1, 4, 3, {"scratch_mib": 1}, "triv"), "w14_pow_out": (14, Q62_16x3, 2, 2, 8, 3, {}, "triv"),
}


@pytest.mark.parametrize("row", list(FULL_ROWS))
def test_mul_full(oracle_lib, row):
    """alch_ct_mul_full: a and b views of one parent on the operands' ring, out a view in the interior of a parent on the result's
    ring -- the same parent where L_in = L_out (one suffix ring serves both sides).  out equals the C restatement's composition
    (helpers.oracle_full_mul); a, b and every margin are as uploaded; batch + 1 is refused."""
    import alchemy_amd as A
    from alchemy_amd import capi
    from helpers import oracle_full_mul
    logn, qs_h, l_in, l_out, word, batch, opts, gadget = FULL_ROWS[row]
    n, L = 1 << logn, len(qs_h)
    rh, rin = A.Ring(2 * n, qs_h), A.Ring(2 * n, qs_h[L - l_in:])
    rout = rin if l_in == l_out else A.Ring(2 * n, qs_h[L - l_out:])
    assert rh.word_bytes == word
    c = source_constants()
    assert (logn > c["split_above"][word]) == ("unfused" in row)                 # do_mul_full_unfused serves the split rings
    for k, v in opts.items():
        rh.set_option(k, v)
    if "chunk" in opts:
        assert opts["chunk"] < batch < 2 * opts["chunk"] and opts["rs_slots"] < 2 * (batch - opts["chunk"])
    if "unfused" in row:                                                         # (2 + elems + 4) hint-ring elements per ciphertext
        source_has(KS_STAGE_ELEMS, "const size_t per_ct = (2 + s.elems + 4) * eb;",
                   "const size_t chunk = scratch_chunk(rh->scratch_mib << 20, batch, per_ct);")
        assert (1 << 20) // ((2 + 4) * n * L * word) == 0                         # even without s.elems: below one ciphertext, one per chunk
    g = capi.ALCH_GAD_BASE2 if gadget == "base2" else capi.ALCH_GAD_TRIV
    hint_host = words(900 + len(row), 2 * rh.gadget_digits(g), n, qs_h)
    hint = rh.hint_load(hint_host, g)
    if rout is rin:
        (outs, as_, bs), total = gapped([2 * batch] * 3)
        host_in = host_out = words(901 + len(row), total, n, rin.qs)
        pin, (out, a, b) = carve(rin, host_in, outs, as_, bs)
        pout = pin
        parents = [(pin, host_in, [outs])]
    else:
        (as_, bs), total = gapped([2 * batch] * 2)
        host_in = words(901 + len(row), total, n, rin.qs)
        pin, (a, b) = carve(rin, host_in, as_, bs)
        outs = (MARGIN, 2 * batch)
        # behind out: the 16 elements of a key-switch group of 8 ciphertexts, counted from where the last chunk may start
        host_out = words(902 + len(row), MARGIN + 2 * batch + 16, n, rout.qs)
        pout, (out,) = carve(rout, host_out, outs)
        parents = [(pin, host_in, []), (pout, host_out, [outs])]
    flags = capi.ALCH_POW_OUT if "pow_out" in row else 0
    capi.ct_mul_full(hint, a, b, out, batch, flags=flags)
    got = None
    for parent, host, written in parents:
        d = assert_parent_unchanged(parent, host, written)
        if parent is pout:
            got = d
    A_, B_ = cut(host_in, as_), cut(host_in, bs)
    for ct in range(batch):
        w0, w1 = oracle_full_mul(oracle_lib, n, qs_h, l_in, l_out, list(hint_host), A_[2 * ct], A_[2 * ct + 1], B_[2 * ct], B_[2 * ct + 1],
                                 pow_out=bool(flags), gadget=gadget)
        assert np.array_equal(got[outs[0] + 2 * ct], w0) and np.array_equal(got[outs[0] + 2 * ct + 1], w1), (row, ct)
    assert_reduced(cut(got, outs), rout.qs)
    refuse(lambda: capi.ct_mul_full(hint, a, b, out, batch + 1, flags=flags), [])
    for parent, host, written in parents:
        assert_parent_unchanged(parent, host, written)
    assert np.array_equal(pout.download(), got)


@pytest.mark.parametrize("m,rs_lin", [(53760, 1), (53760, 0), (45, 1)])
def test_mul_full_general(oracle_lib, m, rs_lin):
    """alch_ct_mul_full on a general index (do_mul_full_unfused: the key-switch stage, then rescale_down_crt with rs_lin 1 or the
    limb-at-a-time form with rs_lin 0), hint on three limbs, operands on two, result on one, batch 5; scratch_mib 1 leaves one
    ciphertext per chunk at phi = 12288.  Against helpers.oracle_full_mul_general."""
    import alchemy_amd as A
    from alchemy_amd import capi
    from helpers import oracle_full_mul_general
    qs_h = primes_below(m, 3, 1 << 31)
    rh, rin, rout = A.Ring(m, qs_h), A.Ring(m, qs_h[1:]), A.Ring(m, qs_h[2:])
    rh.set_option("rs_lin", rs_lin)
    rh.set_option("scratch_mib", 1)
    batch, n = 5, rh.n
    if m == 53760:
        source_has(KS_STAGE_ELEMS, "const size_t per_ct = (2 + s.elems + 4) * eb;")
        assert n == gen_ks_bound() and (1 << 20) // (8 * n * 3 * 4) == 0          # at least (2 + 2 + 4) hint-ring elements per ciphertext: one per chunk
    hint_host = words(950 + m, 2 * rh.L, n, qs_h)
    hint = rh.hint_load(hint_host)
    (as_, bs), total = gapped([2 * batch] * 2)
    host_in = words(951 + m, total, n, rin.qs)
    outs = (MARGIN, 2 * batch)
    host_out = words(952 + m, MARGIN + 2 * batch + 16, n, rout.qs)
    pin, (a, b) = carve(rin, host_in, as_, bs)
    pout, (out,) = carve(rout, host_out, outs)
    capi.ct_mul_full(hint, a, b, out, batch)
    got = assert_parent_unchanged(pout, host_out, [outs])
    assert_parent_unchanged(pin, host_in)
    A_, B_ = cut(host_in, as_), cut(host_in, bs)
    for ct in range(batch):
        w0, w1 = oracle_full_mul_general(oracle_lib, m, qs_h, 2, 1, list(hint_host), A_[2 * ct], A_[2 * ct + 1], B_[2 * ct], B_[2 * ct + 1])
        assert np.array_equal(got[outs[0] + 2 * ct], w0) and np.array_equal(got[outs[0] + 2 * ct + 1], w1), (m, rs_lin, ct)
    assert_reduced(cut(got, outs), rout.qs)
    refuse(lambda: capi.ct_mul_full(hint, a, b, out, batch + 1), [(pin, host_in)])
    assert np.array_equal(pout.download(), got)


# ---- 4c. alch_ct_mod_switch, alch_ct_mod_switch_deg -----------------------------------------------------------------------------------------
# name -> (index, moduli of the big ring or (count, bound), limbs dropped, degree, batch, options)
SWITCH_ROWS = {
    # two-power, do_mod_switch's limb-at-a-time walk: 3 * per * (element bytes) of scratch per ciphertext
    "p11_d1": (1 << 12, SIX_QS[:3], 1, 1, 9, {"scratch_mib": 1}), "p11_d2_two": (1 << 12, SIX_QS[:3], 2, 2, 5, {"scratch_mib": 1}),
    "p15_d1": (1 << 16, SIX_QS[:2], 1, 1, 3, {"scratch_mib": 1}), "p15_d2": (1 << 16, SIX_QS[:3], 2, 2, 3, {}),
    # general index: the CRT-resident walk (rs_lin 1: per * ddn * n words per ciphertext) and the limb-at-a-time one (rs_lin 0)
    "g53760_lin": (53760, (2, 1 << 31), 1, 1, 11, {"scratch_mib": 1}), "g53760_limbs": (53760, (2, 1 << 31), 1, 1, 3, {"scratch_mib": 1, "rs_lin": 0}),
    "g45_d2_two": (45, (3, 1 << 31), 2, 2, 5, {}),
}


def switch_down_want(oracle_lib, m, qs, drop, per, x):
    """SymmSHE modSwitch down on CRT-basis elements, `per` per ciphertext: c0 through the decoding basis on a general index, every
    other component on the powerful basis, one limb at a time (tests/test_gpu_general_index.py)."""
    gen = m & (m - 1) != 0
    mk = (lambda q: oracle_lib.GenRing(m, q)) if gen else (lambda q: oracle_lib.Ring(m // 2, q))
    ob, osm = mk(qs), mk(qs[drop:])
    steps = [mk(qs[u:]) for u in range(drop)]
    want = []
    for e, elem in enumerate(x):
        cur = ob.crtinv(elem)
        if e % per == 0 and gen:
            cur = ob.linv(cur)
        for s in steps:
            cur = s.rescale_drop0(cur)
        if e % per == 0 and gen:
            cur = osm.l(cur)
        want.append(osm.crt(cur))
    return np.stack(want)


@pytest.mark.parametrize("row", list(SWITCH_ROWS))
def test_mod_switch(oracle_lib, row):
    """modSwitch down from a view of one ring's parent into a view of the smaller ring's parent (alch_ct_mod_switch for degree 1,
    alch_ct_mod_switch_deg for degree 2) and up again into a second view of the big ring's parent.  Down equals the C restatement,
    up is (0, .., 0, q_a x) in Python integers; both parents are as uploaded outside the written views; batch + 1 is refused both ways."""
    import alchemy_amd as A
    from alchemy_amd import capi
    from alchemy_amd.mulsteps import mod_switch
    m, qs, drop, degree, batch, opts = SWITCH_ROWS[row]
    big, _, qs = make_ring(oracle_lib, m, qs, 4, opts)
    small = A.Ring(m, qs[drop:])
    per, gen = degree + 1, m & (m - 1) != 0
    eb = big.n * big.L * 4
    if "scratch_mib" in opts:                                                     # which walk, and how it cuts the batch
        source_has("const size_t per_b = P * (size_t)ddn * n * sizeof(W);", "const size_t chunk = scratch_chunk(rin->scratch_mib << 20, batch, per_b);",
                   "const size_t per_ct = 3 * P * eb;", "const size_t chunk = scratch_chunk(rin->scratch_mib << 20, batch, per_ct);")
        lin = gen and opts.get("rs_lin", 1)
        chunk = max(1, (1 << 20) // (per * drop * big.n * 4 if lin else 3 * per * eb))
        assert chunk < batch and (batch % chunk or chunk == 1), (chunk, batch)
        assert row not in ("p11_d1", "p11_d2_two", "g53760_lin") or (chunk > 1 and batch % chunk)      # these rows: a ragged last chunk
    (ins, ups), total = gapped([per * batch] * 2)
    host_big = words(1000 + len(row), total, big.n, qs)
    (downs,), total_s = gapped([per * batch])
    host_small = words(1001 + len(row), total_s, small.n, qs[drop:])
    pbig, (src, up) = carve(big, host_big, ins, ups)
    psmall, (down,) = carve(small, host_small, downs)
    switch = (lambda i, o, k: capi.ct_mod_switch(i, o, k)) if degree == 1 else (lambda i, o, k: mod_switch(i, o.ring, k, degree=2, out=o))
    switch(src, down, batch)
    got = assert_parent_unchanged(psmall, host_small, [downs])
    assert_parent_unchanged(pbig, host_big)
    want = switch_down_want(oracle_lib, m, qs, drop, per, cut(host_big, ins))
    assert np.array_equal(cut(got, downs), want), row
    assert_reduced(cut(got, downs), qs[drop:])
    refuse(lambda: switch(src, down, batch + 1), [(pbig, host_big)])
    assert np.array_equal(psmall.download(), got)
    # and up
    switch(down, up, batch)
    got_up = assert_parent_unchanged(pbig, host_big, [ups])
    assert np.array_equal(psmall.download(), got)
    mult = 1
    for q in qs[:drop]:
        mult *= q
    up_got = cut(got_up, ups)
    assert not up_got[:, :, :drop].any()
    kept = np.array(qs[drop:], dtype=object)
    assert np.array_equal(up_got[:, :, drop:], i64(want.astype(object) * mult % kept)), row
    refuse(lambda: switch(down, up, batch + 1), [])
    assert np.array_equal(pbig.download(), got_up)


# ---- 4d. alch_ct_tunnel ---------------------------------------------------------------------------------------------------------------------
# (tunnel_ep, tunnel_fused, tunnel_mac): the five option sets of tests/test_gpu_tunnel_structure.py
TUNNEL_OPTION_SETS = ((1, 2, 1), (1, 4, 1), (1, 0, 1), (1, 0, 0), (0, 2, 1))
# name -> ((r', s'), L, moduli rule, gadget, batch, option set, scratch_mib)
TUNNEL_ROWS = {f"g25to15_{'_'.join(map(str, o))}": ((25, 15), 3, "top31", "triv", 5, o, None) for o in TUNNEL_OPTION_SETS}
TUNNEL_ROWS.update({
    "g25to15_base2": ((25, 15), 2, "top31", "base2", 5, (1, 0, 1), None),
    "g8to12_no_e_ring": ((8, 12), 3, "top31", "triv", 5, (1, 0, 1), None),
    # 38400 -> 25600: 491520 bytes of scratch per ciphertext on the composed path -> chunks of 2, 2, 1 (test_7_chunked_trivgad_at_phi_10240)
    "g38400to25600_chunks": ((38400, 25600), 2, "top31", "triv", 5, (1, 0, 1), 1),
    "p64to32": ((64, 32), 3, "above29", "triv", 5, None, None), "p64to32_base2": ((64, 32), 3, "above29", "base2", 5, None, None),
    # 2^12 -> 2^13 at three limbs, CRT input (c0 read in place): eight ciphertexts per chunk under scratch_mib 1, 11 = 8 + 3
    "p4096to8192_chunks": ((1 << 12, 1 << 13), 3, "above29", "triv", 11, None, 1),
})


@pytest.mark.parametrize("row", list(TUNNEL_ROWS))
def test_tunnel(oracle_lib, row):
    """alch_ct_tunnel from a view in the interior of an R' parent into a view in the interior of an S' parent: out equals the C
    restatement's composition (helpers.oracle_tunnel), both parents are as uploaded elsewhere; batch + 1 is refused."""
    import math
    import alchemy_amd as A
    from alchemy_amd import capi
    from helpers import oracle_tunnel, primes_1_mod
    (rp, sp), L, rule, gadget, batch, opts, mib = TUNNEL_ROWS[row]
    lcm = rp * sp // math.gcd(rp, sp)
    qs = primes_below(lcm, L, 1 << 31) if rule == "top31" else primes_1_mod(lcm, L, 1 << 29)
    gr, gs = A.Ring(rp, qs), A.Ring(sp, qs)
    assert gr.word_bytes == gs.word_bytes == 4
    if opts is not None:
        for name, v in zip(("tunnel_ep", "tunnel_fused", "tunnel_mac"), opts):
            gs.set_option(name, v)
    if mib is not None:
        gs.set_option("scratch_mib", mib)
    g = capi.ALCH_GAD_BASE2 if gadget == "base2" else capi.ALCH_GAD_TRIV
    ep, d_rel = A.Tunnel.info(gr, gs)
    if row == "g38400to25600_chunks":
        source_has("const size_t per_ct = 2 * ebr + 2 * (size_t)D * ebx + (fused ? 0 : (size_t)D * GD * ebd);",
                   "const size_t chunk = scratch_chunk(rs->scratch_mib << 20, batch, per_ct);")
        ebr, ebx = L * gr.n * 4, L * 5120 * 4                                 # do_tunnel: Pow copy of the input, x0, x1, digits at phi(e') = 5120
        assert gr.n == 10240 and d_rel == 2 and (1 << 20) // (2 * ebr + 2 * d_rel * ebx + d_rel * L * ebx) == 2 and batch % 2
    if row == "p4096to8192_chunks":
        # do_tunnel_pow2, up with CRT input and TrivGad: no x0, no x1, d_rel * L digits of L limb-polynomials at dimension n_r
        source_has("const size_t x0_b = c0_in_place ? 0 : (size_t)d * Lin * pd, x1_b = base2 ? (size_t)d * L * pd : 0, dig_b = (size_t)d * GD * L * pd;",
                   "const size_t per_ct = 2 * ebr + x0_b + x1_b + dig_b;", "const bool c0_in_place = up && !pin;")
        chunk = (1 << 20) // (2 * L * gr.n * 4 + d_rel * L * L * gr.n * 4)
        assert d_rel == 1 and 1 < chunk < batch and batch % chunk, chunk
    if row.startswith("g"):
        # alch_tunnel_create gives the tunnel a ring of its own for E' when E' is smaller than S' and has a general-index ring with
        # phi(e') % 4 = 0 (and tunnel_ep is on); pieces_ok for 25 -> 15 is what tests/test_tunnel_table_host.py asserts for that pair
        source_has("if (ep != rs->m && rs->opts.tunnel_ep) {",
                   "re->gen && re->word == rs->word && re->n % 4 == 0 && rs->n % 4 == 0) {")
        phi_e = sum(1 for k in range(1, ep + 1) if math.gcd(k, ep) == 1)
        may = ep != sp and ep & (ep - 1) != 0 and phi_e % 4 == 0 and gs.n % 4 == 0
        assert may == ("no_e_ring" not in row), (ep, phi_e)
    D = gs.gadget_digits(g)
    lin, ks = words(1100 + len(row), d_rel, gs.n, qs), words(1101 + len(row), 2 * d_rel * D, gs.n, qs)
    tun = A.Tunnel(gr, gs, gs.upload(lin), gs.upload(ks), gadget=g)
    (ins,), total_r = gapped([2 * batch])
    host_r = words(1102 + len(row), total_r, gr.n, qs)
    outs = (MARGIN, 2 * batch)
    host_s = words(1103 + len(row), MARGIN + 2 * batch + 16, gs.n, qs)          # a tile of ciphertexts behind the last one still lies inside
    pr, (src,) = carve(gr, host_r, ins)
    ps, (out,) = carve(gs, host_s, outs)
    tun.apply(src, out, batch)
    got = assert_parent_unchanged(ps, host_s, [outs])
    assert_parent_unchanged(pr, host_r)
    cts = cut(host_r, ins)
    for ct in range(batch):
        w0, w1 = oracle_tunnel(oracle_lib, rp, sp, qs, list(lin), list(ks), cts[2 * ct], cts[2 * ct + 1], None, gadget=gadget)
        assert np.array_equal(got[outs[0] + 2 * ct], w0) and np.array_equal(got[outs[0] + 2 * ct + 1], w1), (row, ct)
    assert_reduced(cut(got, outs), qs)
    refuse(lambda: tun.apply(src, out, batch + 1), [(pr, host_r)])
    assert np.array_equal(ps.download(), got)


# ---- 4e. the decrypt side ---------------------------------------------------------------------------------------------------------------------
# name -> (index, L, degree, batch): n = 32 (a wave per element), n = 256 and 2048 (a workgroup per element), a general index
DECRYPT_ROWS = {"p64_L1_d2": (64, 1, 2, 5), "p512_L3_d1": (512, 3, 1, 5), "p4096_L8_d2": (1 << 12, 8, 2, 3), "g45_L3_d1": (45, 3, 1, 5)}
P_LIFT = 1 << 30


def horner_want(o, general, comps, sk):
    """c(s) on the decoding basis from CRT-basis components (tests/test_gpu_decrypt.py: oracle_error_term)."""
    acc = comps[-1]
    for c in reversed(comps[:-1]):
        acc = o.add(o.mul(acc, sk), c)
    acc = o.crtinv(np.ascontiguousarray(acc))
    return o.linv(acc) if general else acc


def lifted_ints(elem, qs):
    """The centred lift mod Q = prod q_j of every coefficient of one (n, L) element, as Python integers."""
    Q = 1
    for q in qs:
        Q *= q
    coef = [Q // q * pow(Q // q, -1, q) for q in qs]
    out = []
    for row in elem:
        x = sum(int(r) * c for r, c in zip(row, coef)) % Q
        out.append(x - Q if x > (Q - 1) // 2 else x)
    return out


def to_digits(x, qs):
    out = []
    for q in qs:
        out.append(x % q)
        x //= q
    return out


@pytest.mark.parametrize("row", list(DECRYPT_ROWS))
def test_decrypt_side(oracle_lib, row):
    """alch_ct_error_term, alch_buf_lift and alch_ct_decrypt_lift with ciphertexts, key element and c(s) as ranges of one ring parent
    and the lifted residues in the interior of a Z_p parent of the same index; out_first = dst_first = first = 1 on views at offset 3,
    the key given by its index in the parent.  c(s) equals the C restatement's Horner form, the residues and the digit vectors of
    max |lift| Python integers; nothing else changes in either parent; one ciphertext more, or an offset one further, is refused."""
    import alchemy_amd as A
    from alchemy_amd.decrypt import decrypt_lift, error_term, lift
    m, L, degree, batch = DECRYPT_ROWS[row]
    ring, o, qs = make_ring(oracle_lib, m, (L, 1 << 31), 4, {})
    general = m & (m - 1) != 0
    per, p = degree + 1, P_LIFT
    zp = A.Ring(m, [p], nocrt=True)
    (cs, ks_, es), total = gapped([per * batch, 1, batch + 1])
    host = words(1200 + len(row), total, ring.n, qs)
    (zs,), total_z = gapped([batch + 1])
    host_z = words(1201 + len(row), total_z, zp.n, [p])
    sk_index = ks_[0]
    cts = cut(host, cs)
    want_e = np.stack([horner_want(o, general, [cts[per * b + c] for c in range(per)], host[sk_index]) for b in range(batch)])
    e_written, z_written = (es[0] + 1, batch), (zs[0] + 1, batch)
    # alch_ct_error_term
    parent, (ct_v, e_v) = carve(ring, host, cs, es)
    error_term(ct_v, batch, parent, degree=degree, out=e_v, out_first=1, sk_index=sk_index)
    got = assert_parent_unchanged(parent, host, [e_written])
    assert np.array_equal(cut(got, e_written), want_e), row
    assert_reduced(cut(got, e_written), qs)
    refuse(lambda: error_term(ct_v, batch, parent, degree=degree, out=e_v, out_first=2, sk_index=sk_index), [])
    refuse(lambda: error_term(ct_v, batch + 1, parent, degree=degree, out=e_v, out_first=0, sk_index=sk_index), [])
    refuse(lambda: error_term(ct_v, batch, e_v, degree=degree, out=e_v, out_first=1, sk_index=batch + 1), [])
    assert np.array_equal(parent.download(), got)
    # alch_buf_lift of uploaded words: elements [1, 1 + batch) of the view es into elements [1, 1 + batch) of the view zs
    src_words = cut(host, es)[1:]
    lifted = [lifted_ints(e, qs) for e in src_words]
    want_z = np.array([[v * (p - 1) % p for v in x] for x in lifted], dtype=np.int64)
    want_digits = [to_digits(max(abs(v) for v in x), qs) for x in lifted]
    parent, (e_v,) = carve(ring, host, es)
    pz, (z_v,) = carve(zp, host_z, zs)
    digits = lift(e_v, z_v, l=p - 1, want_max=True, first=1, count=batch, dst_first=1)
    got_z = assert_parent_unchanged(pz, host_z, [z_written])
    assert_parent_unchanged(parent, host)
    assert np.array_equal(cut(got_z, z_written)[:, :, 0], want_z) and digits == want_digits, row
    assert_reduced(cut(got_z, z_written), [p])
    for first, count, dst_first in ((2, batch, 1), (1, batch, 2), (1, batch + 1, 0), (0, batch + 1, 1)):
        refuse(lambda: lift(e_v, z_v, l=1, first=first, count=count, dst_first=dst_first), [(parent, host)])
    assert np.array_equal(pz.download(), got_z)
    # alch_ct_decrypt_lift
    lifted = [lifted_ints(e, qs) for e in want_e]
    want_z = np.array([[v * (p - 1) % p for v in x] for x in lifted], dtype=np.int64)
    parent, (ct_v,) = carve(ring, host, cs)
    pz, (z_v,) = carve(zp, host_z, zs)
    digits = decrypt_lift(ct_v, batch, parent, degree=degree, dst=z_v, l=p - 1, want_max=True, dst_first=1, sk_index=sk_index)
    got_z = assert_parent_unchanged(pz, host_z, [z_written])
    assert_parent_unchanged(parent, host)
    assert np.array_equal(cut(got_z, z_written)[:, :, 0], want_z), row
    assert digits == [to_digits(max(abs(v) for v in x), qs) for x in lifted], row
    refuse(lambda: decrypt_lift(ct_v, batch, parent, degree=degree, dst=z_v, dst_first=2, sk_index=sk_index), [(parent, host)])
    refuse(lambda: decrypt_lift(ct_v, batch + 1, parent, degree=degree, dst=z_v, dst_first=0, sk_index=sk_index), [(parent, host)])
    assert np.array_equal(pz.download(), got_z)


# ---- 4f. the methods between two indices ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,mb", [(9, 45), (32, 96)])
def test_between_index_methods(m, mb):
    """alch_buf_embed and alch_buf_twace on every basis and alch_buf_coeffs (d_rel * count output elements), count 3, between a view
    in the interior of the small ring's parent and one in the interior of the big ring's: the written view equals the model limb by
    limb (oracle.model_gen, as tests/test_gpu_resident_edges.py), both parents are as uploaded elsewhere; count + 1 is refused."""
    import alchemy_amd as A
    from alchemy_amd import capi
    from oracle import model_gen as G
    qs = primes_below(mb, 2, 1 << 31)
    s, b = G.Index(m), G.Index(mb)
    rs, rb = A.Ring(m, qs), A.Ring(mb, qs)
    assert (rs.n, rb.n, rs.word_bytes) == (s.n, b.n, 4)
    count, d_rel = 3, b.n // s.n
    (ss, cs), total_s = gapped([count, d_rel * count])
    (bs,), total_b = gapped([count])
    host_s, host_b = words(1300 + m, total_s, s.n, qs), words(1301 + m, total_b, b.n, qs)
    xs, ys = cut(host_s, ss), cut(host_b, bs)

    def limbs(src, f):
        """f(limb values as Python integers, q) applied to every limb of every element."""
        return np.stack([np.stack([np.array(f(e[:, j].tolist(), q), dtype=np.int64) for j, q in enumerate(qs)], axis=1) for e in src])

    P, D, C = capi.ALCH_BASIS_POW, capi.ALCH_BASIS_DEC, capi.ALCH_BASIS_CRT
    to_big = [(P, lambda v, q: G.embed_pow(v, s, b)), (D, lambda v, q: G.embed_dec_def(v, s, b, q)), (C, lambda v, q: G.embed_crt_def(v, s, b))]
    to_small = [(P, lambda v, q: G.twace_pow_dec(v, s, b)), (D, lambda v, q: G.twace_pow_dec(v, s, b)), (C, lambda v, q: G.twace_crt_def(v, s, b, q))]
    for basis, f in to_big:
        ps, (sv,) = carve(rs, host_s, ss)
        pb, (bv,) = carve(rb, host_b, bs)
        bv.embed_from(sv, count, basis)
        got = assert_parent_unchanged(pb, host_b, [bs])
        assert_parent_unchanged(ps, host_s)
        assert np.array_equal(cut(got, bs), limbs(xs, f)), ("embed", basis)
        assert_reduced(cut(got, bs), qs)
        refuse(lambda: bv.embed_from(sv, count + 1, basis), [(ps, host_s)])
        assert np.array_equal(pb.download(), got)
    for basis, f in to_small:
        ps, (sv,) = carve(rs, host_s, ss)
        pb, (bv,) = carve(rb, host_b, bs)
        sv.twace_from(bv, count, basis)
        got = assert_parent_unchanged(ps, host_s, [ss])
        assert_parent_unchanged(pb, host_b)
        assert np.array_equal(cut(got, ss), limbs(ys, f)), ("twace", basis)
        assert_reduced(cut(got, ss), qs)
        refuse(lambda: sv.twace_from(bv, count + 1, basis), [(pb, host_b)])
        assert np.array_equal(ps.download(), got)
    ps, (cv,) = carve(rs, host_s, cs)
    pb, (bv,) = carve(rb, host_b, bs)
    cv.coeffs_from(bv, count)
    got = assert_parent_unchanged(ps, host_s, [cs])
    assert_parent_unchanged(pb, host_b)
    rows = cut(got, cs).reshape(count, d_rel, s.n, len(qs))
    for e in range(count):
        for j in range(len(qs)):
            assert [c[:, j].tolist() for c in rows[e]] == G.coeffs(ys[e][:, j].tolist(), s, b), (e, j)
    assert_reduced(cut(got, cs), qs)
    refuse(lambda: cv.coeffs_from(bv, count + 1), [(pb, host_b)])
    assert np.array_equal(ps.download(), got)
    short = ps.view(cs[0], d_rel * count - 1)                                 # one element short of d_rel * count
    refuse(lambda: short.coeffs_from(bv, count), [(pb, host_b)])
    assert np.array_equal(ps.download(), got)


# ---- 4g. the plaintext side -----------------------------------------------------------------------------------------------------------------
def negacyclic(a, b, p):
    """The product in Z_p[x] / (x^n + 1) of two coefficient vectors (the powerful basis of a two-power index)."""
    n = len(a)
    full = np.convolve(a, b)
    out = full[:n].copy()
    out[:n - 1] -= full[n:]
    return out % p


def lift_two31(m):
    import alchemy_amd as A
    from helpers import primes_1_mod
    return A.Ring(m, primes_1_mod(m, 2, 1 << 30))


@pytest.mark.parametrize("m,p,batch,mib", [(45, 7, 5, None), (9, 7, 5, None), (8192, 32, 37, 1)])
def test_pt_mul(m, p, batch, mib):
    """alch_pt_mul on views a, b -> dst of one gapped Z_p parent: n % 4 = 0 and != 0 against the ring product by definition
    (oracle.model_gen), and n = 4096 under scratch_mib 1 -- 16 lifted elements per chunk, 37 = 16 + 16 + 5 -- against the negacyclic
    convolution.  a, b and the margins are as uploaded; count + 1 is refused."""
    import alchemy_amd as A
    from alchemy_amd.plaintext import pt_mul
    from oracle import model_gen as G
    r, lift = A.Ring(m, [p], nocrt=True), lift_two31(m)
    assert (r.n % 4 == 0) == (m != 9)
    if mib:
        lift.set_option("scratch_mib", mib)
        source_has("const size_t chunk = scratch_chunk(lift->scratch_mib << 20, count, 2 * eb);")                 # do_pt_mul
        chunk = (1 << 20) // (2 * lift.n * lift.L * lift.word_bytes)
        assert chunk > 1 and batch > 2 * chunk and batch % chunk
    (as_, bs, ds), total = gapped([batch] * 3)
    host = words(1400 + m, total, r.n, [p])
    parent, (a, b, d) = carve(r, host, as_, bs, ds)
    pt_mul(lift, d, a, b, batch)
    got = assert_parent_unchanged(parent, host, [ds])
    A_, B_ = cut(host, as_)[:, :, 0], cut(host, bs)[:, :, 0]
    if mib:
        want = np.stack([negacyclic(x, y, p) for x, y in zip(A_, B_)])
    else:
        idx = G.Index(m)
        want = np.array([G.ring_mul_def(x.tolist(), y.tolist(), idx, p) for x, y in zip(A_, B_)], dtype=np.int64)
    assert np.array_equal(cut(got, ds)[:, :, 0], want), m
    assert_reduced(cut(got, ds), [p])
    refuse(lambda: pt_mul(lift, d, a, b, batch + 1), [])
    assert np.array_equal(parent.download(), got)


@pytest.mark.parametrize("r_,s_,p,batch,mib", [(45, 75, 4, 5, None), (9, 8, 32, 5, None), (4096, 8192, 32, 37, 1)])
def test_pt_eval_lin(r_, s_, p, batch, mib):
    """alch_pt_eval_lin from a view of a Z_p parent over index r into a view of one over index s: phi(s) % 4 = 0 with d_rel = 3 and
    d_rel = 6 from a ring with phi(r) % 4 != 0, against the model's evalLin; 2048 -> 4096 (d_rel = 1: y_0 times the embedded input)
    under scratch_mib 1 with a ragged last chunk, against the negacyclic convolution."""
    import math
    import alchemy_amd as A
    from alchemy_amd.plaintext import pt_linear
    from oracle import model_gen as G
    rr, rs, lift = A.Ring(r_, [p], nocrt=True), A.Ring(s_, [p], nocrt=True), lift_two31(s_)
    if mib:
        lift.set_option("scratch_mib", mib)
        source_has("const size_t chunk = scratch_chunk(lift->scratch_mib << 20, count, (D + 1) * eb);")           # do_pt_eval_lin; d_rel = 1 here
        chunk = (1 << 20) // (2 * lift.n * lift.L * lift.word_bytes)
        assert chunk > 1 and batch > 2 * chunk and batch % chunk
    E, R, S = G.Index(math.gcd(r_, s_)), G.Index(r_), G.Index(s_)
    d_rel = R.n // E.n
    ys = words(1500 + r_, d_rel, rs.n, [p])
    f = pt_linear(lift, rs.upload(ys), r_)
    (ss,), total_r = gapped([batch])
    (ds,), total_s = gapped([batch])
    host_r, host_s = words(1501 + r_, total_r, rr.n, [p]), words(1502 + r_, total_s, rs.n, [p])
    pr, (src,) = carve(rr, host_r, ss)
    ps, (dst,) = carve(rs, host_s, ds)
    f.apply(src, dst, batch)
    got = assert_parent_unchanged(ps, host_s, [ds])
    assert_parent_unchanged(pr, host_r)
    xs = cut(host_r, ss)[:, :, 0]
    if mib:
        assert d_rel == 1 and 2 * rr.n == rs.n
        emb = np.zeros((batch, rs.n), dtype=np.int64)
        emb[:, 0::2] = xs                                                      # zeta_r = zeta_s^2
        want = np.stack([negacyclic(ys[0, :, 0], e, p) for e in emb])
    else:
        yl = [y[:, 0].tolist() for y in ys]
        want = np.array([G.eval_lin_dec(yl, G.linv_def(x.tolist(), R, p), E, R, S, p) for x in xs], dtype=np.int64)
    assert np.array_equal(cut(got, ds)[:, :, 0], want), (r_, s_)
    assert_reduced(cut(got, ds), [p])
    refuse(lambda: f.apply(src, dst, batch + 1), [(pr, host_r)])
    assert np.array_equal(ps.download(), got)


@pytest.mark.parametrize("m,p,p2", [(45, 4, 2), (9, 32, 16)])
def test_pt_rescale_and_add_bcast(m, p, p2):
    """alch_pt_rescale from a view of a Z_p parent into a view of a Z_p' parent (multiples of p / p': the exact quotients), and
    alch_buf_add_bcast with the literal given by its index in the parent; count + 1 refused."""
    import alchemy_amd as A
    from alchemy_amd.plaintext import add_bcast, pt_rescale
    r, r2 = A.Ring(m, [p], nocrt=True), A.Ring(m, [p2], nocrt=True)
    batch, d = 5, p // p2
    (ss, ds), total = gapped([batch, batch])
    host = d * words(1600 + m, total, r.n, [p2])
    (d2s,), total2 = gapped([batch])
    host2 = words(1601 + m, total2, r2.n, [p2])
    parent, (src, dst) = carve(r, host, ss, ds)
    p2parent, (dst2,) = carve(r2, host2, d2s)
    assert pt_rescale(src, dst2, batch) is True
    got2 = assert_parent_unchanged(p2parent, host2, [d2s])
    assert_parent_unchanged(parent, host)
    assert np.array_equal(cut(got2, d2s), cut(host, ss) // d)
    refuse(lambda: pt_rescale(src, dst2, batch + 1), [(parent, host)])
    assert np.array_equal(p2parent.download(), got2)
    lit = ss[0] + 1                                                            # an element of src, by its index in the parent
    add_bcast(dst, src, parent, lit, batch)
    got = assert_parent_unchanged(parent, host, [ds])
    assert np.array_equal(cut(got, ds), (cut(host, ss) + host[lit]) % p)
    refuse(lambda: add_bcast(dst, src, parent, lit, batch + 1), [])
    refuse(lambda: add_bcast(dst, src, src, batch, batch), [])                  # the literal's index one past its buffer
    assert np.array_equal(parent.download(), got)


# ---- 4h. the encrypt side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [21, 64])
def test_gauss_dec_and_ct_encrypt(m):
    """alch_buf_gauss_dec (errorCoset: the coset a view of a Z_7 parent, first = coset_first = 1, elem0 = 11) against tests/gauss_model.py
    and alch_ct_encrypt (err_first = 1, the key by its index in the parent, ct0 = 3) against Python integers, the uniform words being
    those alch_buf_fill_uniform writes.  Every offset one further, and one element / ciphertext more, is refused."""
    import math
    import alchemy_amd as A
    import gauss_model as GM
    from alchemy_amd import encrypt as E
    from helpers import primes_1_mod
    qs = primes_1_mod(m, 2, 1 << 29)
    ring, zp, p, count = A.Ring(m, qs), A.Ring(m, [7], nocrt=True), 7, 5
    svar = 3.0 / math.sqrt(GM.totient(m)) * p * p
    (gs,), total = gapped([count + 1])
    host, host_z = words(1700 + m, total, ring.n, qs), words(1701 + m, total, zp.n, [p])
    parent, (g,) = carve(ring, host, gs)
    pz, (cv,) = carve(zp, host_z, gs)
    seed, elem0 = 0xF00D + m, 11
    E.gauss_dec(g, svar, seed, 1, count, cv, 1, elem0)
    written = (gs[0] + 1, count)
    got = assert_parent_unchanged(parent, host, [written])
    assert_parent_unchanged(pz, host_z)
    cw = cut(host_z, written)[:, :, 0]
    z = GM.gauss_dec(m, svar, seed, elem0, count, p, cw)
    assert np.array_equal(cut(got, written), GM.words(z, qs)) and np.array_equal(np.mod(z, p), cw)
    assert_reduced(cut(got, written), qs)
    for first, k, cfirst in ((2, count, 1), (1, count + 1, 0), (1, count, 2), (0, count + 1, 1)):
        refuse(lambda: E.gauss_dec(g, svar, seed, first, k, cv, cfirst, elem0), [(pz, host_z)])
    assert np.array_equal(parent.download(), got)
    # alch_ct_encrypt
    B, ct0 = 5, 3
    (outs, errs, sks), total = gapped([2 * B, B + 1, 2])
    host = words(1702 + m, total, ring.n, qs)
    parent, (out, err) = carve(ring, host, outs, errs)
    uni = ring.alloc(2 * (ct0 + B))
    uni.fill_uniform(seed)
    u = uni.download()
    sk_index = sks[0] + 1
    E.ct_encrypt(out, B, err, parent, seed, err_first=1, sk_index=sk_index, ct0=ct0)
    got = assert_parent_unchanged(parent, host, [outs])
    q = np.array(qs, dtype=np.int64)
    for b in range(B):
        a = u[2 * (ct0 + b) + 1]
        assert np.array_equal(got[outs[0] + 2 * b + 1], a), (m, b)
        assert np.array_equal(got[outs[0] + 2 * b], (host[errs[0] + 1 + b] - a * host[sk_index] % q) % q), (m, b)
    assert_reduced(cut(got, outs), qs)
    refuse(lambda: E.ct_encrypt(out, B + 1, err, parent, seed, err_first=0, sk_index=sk_index, ct0=ct0), [])
    refuse(lambda: E.ct_encrypt(out, B, err, parent, seed, err_first=2, sk_index=sk_index, ct0=ct0), [])
    refuse(lambda: E.ct_encrypt(out, B, err, err, seed, err_first=1, sk_index=B + 1, ct0=ct0), [])
    assert np.array_equal(parent.download(), got)


@pytest.mark.parametrize("gadget", ["triv", "base2"])
@pytest.mark.parametrize("m", [21, 64])
def test_ks_hint(m, gadget):
    """alch_ct_ks_hint for two values (out_first = v_first = err_first = 1, the key by its index in the parent, ct0 = 3) and the same
    hint by alch_ct_ks_hint_part in two parts cut INSIDE the second value (not at a value boundary), all ranges views of one parent:
    against Python integers (tests/test_gpu_hints.py: expected_pairs).  One entry more, or an offset one further, is refused."""
    import alchemy_amd as A
    from alchemy_amd import capi
    from alchemy_amd import hints as H
    from helpers import primes_1_mod
    from test_gpu_hints import expected_pairs
    qs = primes_1_mod(m, 2, 1 << 29)
    ring = A.Ring(m, qs)
    gad = capi.ALCH_GAD_BASE2 if gadget == "base2" else capi.ALCH_GAD_TRIV
    D, n_v, ct0, seed = ring.gadget_digits(gad), 2, 3, 0xBEEF + m
    total = n_v * D
    split = D + D // 2
    assert D < split < total and split % D
    (outs, vs, errs, sks), count = gapped([2 * total + 1, n_v + 1, total + 1, 2])
    host = words(1800 + m + D, count, ring.n, qs)
    sk_index = sks[0] + 1
    uni = ring.alloc(2 * (ct0 + total))
    uni.fill_uniform(seed)
    u = uni.download()
    want = expected_pairs(qs, gad, cut(host, vs)[1:], cut(host, errs)[1:], host[sk_index], lambda e: u[2 * (ct0 + e) + 1])
    written = (outs[0] + 1, 2 * total)

    def check(parent):
        got = assert_parent_unchanged(parent, host, [written])
        for e, (b, a) in enumerate(want):
            assert np.array_equal(got[written[0] + 2 * e + 1].astype(object), a), (m, e)
            assert np.array_equal(got[written[0] + 2 * e].astype(object), b), (m, e)
        assert_reduced(cut(got, written), qs)
        return got

    parent, (out, v, err) = carve(ring, host, outs, vs, errs)
    H.ct_ks_hint(out, gad, n_v, v, err, parent, seed, out_first=1, v_first=1, err_first=1, sk_index=sk_index, ct0=ct0)
    got = check(parent)
    refuse(lambda: H.ct_ks_hint(out, gad, n_v, v, err, parent, seed, out_first=2, v_first=1, err_first=1, sk_index=sk_index, ct0=ct0), [])
    refuse(lambda: H.ct_ks_hint(out, gad, n_v, v, err, parent, seed, out_first=1, v_first=2, err_first=1, sk_index=sk_index, ct0=ct0), [])
    refuse(lambda: H.ct_ks_hint(out, gad, n_v, v, err, parent, seed, out_first=1, v_first=1, err_first=2, sk_index=sk_index, ct0=ct0), [])
    refuse(lambda: H.ct_ks_hint(out, gad, n_v + 1, v, err, parent, seed, out_first=0, v_first=0, err_first=0, sk_index=sk_index, ct0=ct0), [])
    assert np.array_equal(parent.download(), got)
    parent, (out, v, err) = carve(ring, host, outs, vs, errs)
    H.ct_ks_hint_part(out, gad, 0, split, v, err, parent, seed, out_first=1, v_first=1, err_first=1, sk_index=sk_index, ct0=ct0)
    assert_parent_unchanged(parent, host, [(written[0], 2 * split)])                # the first part's entries only
    H.ct_ks_hint_part(out, gad, split, total - split, v, err, parent, seed, out_first=1 + 2 * split, v_first=1, err_first=1 + split,
                      sk_index=sk_index, ct0=ct0 + split)
    got = check(parent)
    refuse(lambda: H.ct_ks_hint_part(out, gad, split, total - split + 1, v, err, parent, seed, out_first=1 + 2 * split, v_first=1,
                                     err_first=1 + split, sk_index=sk_index, ct0=ct0 + split), [])
    refuse(lambda: H.ct_ks_hint_part(out, gad, split, total - split, v, err, parent, seed, out_first=2 + 2 * split, v_first=1,
                                     err_first=1 + split, sk_index=sk_index, ct0=ct0 + split), [])
    assert np.array_equal(parent.download(), got)


# ---- 5. pool and view lifetime ------------------------------------------------------------------------------------------------------------
def test_view_free_is_not_pooled():
    """alch_buf_free on a view returns nothing to the ring's pool: a buffer of the same element count allocated next lies outside the
    parent's bytes, and words written through it leave the parent as uploaded."""
    ring, qs = ew_ring("G45")
    host = words(800, 9, ring.n, qs)
    parent = ring.upload(host)
    base, size = parent.device_ptr()
    for first in (0, 3):                                        # a view at the parent's own address, and one inside
        parent.view(first, 3).free()
        fresh = ring.alloc(3)
        addr, nbytes = fresh.device_ptr()
        assert addr + nbytes <= base or base + size <= addr, "the pool handed out bytes of the view's parent"
        other = words(801 + first, 3, ring.n, qs)
        fresh.upload(other)
        assert np.array_equal(fresh.download(), other)
        assert_parent_unchanged(parent, host)


def test_pool_reuse_leaves_a_queued_view_call_alone():
    """A pooled buffer is freed and allocated again (the same pointer, stream-ordered reuse) and written while a call on views of a
    parent is queued: the call's result is exact, the rest of the parent as uploaded, the new buffer holds its own words."""
    c = EwCase("G45", "wrap", 810)
    spare = c.ring.alloc(4)
    spare_addr = spare.device_ptr()[0]
    c.d.mul(c.x, c.y, c.count)
    spare.free()
    again = c.ring.alloc(4)
    assert again.device_ptr()[0] == spare_addr                 # the pool's entry, not a new allocation
    other = words(811, 4, c.ring.n, c.qs)
    again.upload(other)
    got = assert_parent_unchanged(c.parent, c.host, [c.ds])
    assert np.array_equal(cut(got, c.ds), i64(c.X() * c.Y() % c.q()))
    assert np.array_equal(again.download(), other)
