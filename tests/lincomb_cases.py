"""What tests/test_gpu_automorph_lincomb.py and tests/test_gpu_slot_linear.py share: the modulus classes and unit sets of
tests/test_gpu_automorph_hoisted.py (the few lines are copied: test files are not imported from one another), and the reference of
alch_ct_automorph_lincomb -- the composition of existing calls the header names."""
import math
import os
import random
import re

import numpy as np

import alchemy_amd as A
from conftest import ROOT
from helpers import lazy_group, primes_1_mod, primes_below


def kernel_constants():
    """(ROWS, TILE) as alchemy_amd/csrc/kernel_lincomb.hpp is built."""
    src = open(os.path.join(ROOT, "alchemy_amd", "csrc", "kernel_lincomb.hpp")).read()
    return tuple(int(re.search(rf"constexpr int LINCOMB_{k} = (\d+);", src).group(1)) for k in ("ROWS", "TILE"))


def moduli(m, kind):
    if kind == "top31":                                          # two 31-bit limbs at the top of 2^31: K = 0, product-at-a-time
        qs = primes_below(m, 2, 1 << 31)
        assert all(lazy_group(q) == 0 for q in qs)
        return qs
    if kind == "top31x4":
        return primes_below(m, 4, 1 << 31)
    if kind == "p28":                                            # the first primes above 2^28: lazy groups of 8
        qs = primes_1_mod(m, 2, 1 << 28)
        assert all(lazy_group(q) == 8 for q in qs)
        return qs
    if kind == "p29":                                            # three 29-bit limbs: room for a key switch's noise
        return primes_1_mod(m, 3, 1 << 28)
    if kind == "top62":                                          # one prime just below 2^62: 8-byte words
        return primes_below(m, 1, 1 << 62)
    if kind == "mix64":                                          # 62 + 17 + 32 bits
        qs = [primes_below(m, 1, 1 << 62)[0], primes_1_mod(m, 1, 1 << 16)[0], primes_1_mod(m, 1, 1 << 31)[0]]
        assert [(q - 1).bit_length() for q in qs] == [62, 17, 32]
        return qs
    raise AssertionError(kind)


WORD_BYTES = {"top31": 4, "top31x4": 4, "p28": 4, "p29": 4, "top62": 8, "mix64": 8}


def uniform(rng, count, n, qs):
    return np.ascontiguousarray(np.stack([rng.integers(0, q, size=(count, n), dtype=np.int64) for q in qs], axis=2))


def all_units(m):
    return [j for j in range(1, m) if math.gcd(j, m) == 1] if m > 1 else [1]


def unit_set(m, name):
    us = all_units(m)
    rnd = random.Random(m)
    if name == "one":
        return [1]
    if name == "three":                                          # two-power: {5, m - 1, 25}
        return [5, m - 1, 25] if m & (m - 1) == 0 else [us[1], m - 1, rnd.choice(us[2:-1])]
    if name == "rep":                                            # a repeated unit, one of them unreduced
        j = rnd.choice(us[1:])
        return [j, us[1], j + m]
    if name == "r32":
        return [rnd.choice(us) for _ in range(32)]
    raise AssertionError(name)


def reference(ring, aset, weights, w_first, n_out, cts, batch, s_pre):
    """(n_out, 2 * batch, n, L): alch_ct_automorph_hoisted without the sum flag, alch_buf_mul_public per (row, rotation) and the sum
    mod q_j -- the words are below 2^62, so the int64 sum of two does not wrap."""
    R = len(aset.js)
    rot = A.ct_automorph_hoisted(aset, cts, batch, s_pre=s_pre)
    tmp = ring.alloc(2 * batch)
    qv = np.array(ring.qs, dtype=np.int64)
    out = np.zeros((n_out, 2 * batch, ring.n, ring.L), dtype=np.int64)
    for g in range(n_out):
        for r in range(R):
            tmp.mul_public(rot.view(2 * batch * r, 2 * batch), weights, w_first + g * R + r, 2 * batch)
            out[g] = (out[g] + tmp.download(0, 2 * batch)) % qv
    return out
