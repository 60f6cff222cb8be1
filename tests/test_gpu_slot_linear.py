"""GPU: a matrix over Z_p applied to the CRT slots of encrypted plaintexts, end to end (alchemy_amd/slotlinear.py):

    gen_sk -> SlotLinear (baby hints, giant hints, weights) -> encrypt_batch -> apply -> decrypt_batch

Every ciphertext decrypts to the plaintext whose slot vector -- the oracle's by-definition crt mod p (oracle/model_gen.py), used in
the test only -- is M . slots(pt) mod p.  `apply` (the rows of the giants from one alch_ct_automorph_lincomb call, or from the
composition where the recorded table says it is faster; then the giants) must give, on either route, the words of the composed path
(alch_ct_automorph_hoisted, alch_buf_mul_public, alch_buf_add, the same giants); the error rates of both are printed, not asserted."""
import random

import numpy as np
import pytest

import alchemy_amd as A
from alchemy_amd import capi
from alchemy_amd import encrypt as E
from alchemy_amd import slotlinear
from alchemy_amd.ctadd import ct_add_raw
from lincomb_cases import all_units, kernel_constants, moduli
from oracle import model_gen as G

pytestmark = pytest.mark.gpu

TRIV, BASE2 = capi.ALCH_GAD_TRIV, capi.ALCH_GAD_BASE2
SETUPS = {
    "m16-whole-triv": (64, 16, 17, None, TRIV),                  # baby = (Z/16)^*: 8 rotations, one row
    "m16-sub5-base2": (64, 16, 17, [1, 5, 9, 13], BASE2),        # baby = <5>, giants {1, 3}: two rows and one giant key switch
    "m16-sub5-triv": (64, 16, 17, [1, 5, 9, 13], TRIV),
    "m9-whole-triv": (45, 9, 19, None, TRIV),                    # the general engine: 6 rotations
    "m16-one-triv": (64, 16, 17, [1], TRIV),                     # baby = {1}: 8 rows, two row blocks of the kernel
    "m16-one-base2": (64, 16, 17, [1], BASE2),                   #   ... where the recorded table sends the rows to the composition
}
ROUTES = {"m16-whole-triv": "lincomb", "m16-sub5-base2": "lincomb", "m16-sub5-triv": "lincomb", "m9-whole-triv": "lincomb",
          "m16-one-triv": "lincomb", "m16-one-base2": "composition"}


def matrix(kind, n, p, rnd):
    if kind == "identity":
        return [[int(r == c) for c in range(n)] for r in range(n)]
    if kind == "permutation":
        perm = list(range(n))
        rnd.shuffle(perm)
        assert perm != list(range(n))
        return [[int(perm[r] == c) for c in range(n)] for r in range(n)]
    return [[rnd.randrange(p) for _ in range(n)] for _ in range(n)]


def composed(sl, cts, batch, s_pre):
    """The same operator from calls that exist without alch_ct_automorph_lincomb."""
    ring, R = sl.ring, len(sl.baby)
    rot = A.ct_automorph_hoisted(sl.aset, cts, batch, s_pre=s_pre)
    tmp, total = ring.alloc(2 * batch), None
    for gi in range(len(sl.giant)):
        row = ring.alloc(2 * batch)
        for r in range(R):
            dst = row if r == 0 else tmp
            dst.mul_public(rot.view(2 * batch * r, 2 * batch), sl.weights, gi * R + r, 2 * batch)
            if r:
                row.add(row, tmp, 2 * batch)
        if gi == 0:
            total = row
        else:
            moved = A.ct_automorph(sl.autos[gi - 1], row, batch)
            ct_add_raw(total, batch, total, 1, None, 0, moved, 1, None, 0)
    return total


@pytest.mark.parametrize("kind", ["dense", "permutation", "identity"])
@pytest.mark.parametrize("setup", sorted(SETUPS))
def test_encrypt_apply_decrypt_multiplies_the_slots_by_m(setup, kind):
    mp, m, p, baby, gadget = SETUPS[setup]
    batch, seed = 4, 7000 + mp + len(kind)
    qs = moduli(mp, "p29")
    big, sm = G.Index(mp), G.Index(m)
    svar = 3.0 / np.sqrt(float(big.n))
    ring = A.Ring(mp, qs)
    assert ring.word_bytes == 4
    zp_big, zp_small = A.Ring(mp, [p], nocrt=True), A.Ring(m, [p], nocrt=True)
    sk = E.gen_sk(ring, svar, seed)
    rnd = random.Random(seed)
    M = matrix(kind, sm.n, p, rnd)
    baby = all_units(m) if baby is None else baby
    sl = A.SlotLinear(ring, m, p, M, sk, baby, gadget=gadget, svar=svar, seed=seed + 10)
    assert len(sl.baby) * len(sl.giant) == sm.n and len(sl.autos) == len(sl.giant) - 1
    if setup.startswith("m16-sub5"):
        assert sl.giant == [1, 3]
    assert slotlinear.LINCOMB_ROWS == kernel_constants()[0] and sl.route == ROUTES[setup]
    pts = np.array([[[rnd.randrange(p)] for _ in range(sm.n)] for _ in range(batch)], dtype=np.int64)
    cts = E.encrypt_batch(ring, sk, zp_small.upload(pts), zp_small, zp_big, svar, seed + 3)
    cts_host = cts.download()
    to_msd, to_lsd = [pow(p, -1, q) for q in qs], [p % q for q in qs]
    out = sl.apply(cts, batch, s_pre=to_msd)
    assert np.array_equal(cts.download(), cts_host)
    ref = composed(sl, cts, batch, to_msd)
    print(f"m'={mp} m={m} p={p} {setup} {kind}: error rates apply {A.error_rates(out, batch, sk, s_pre=to_lsd)}"
          f" / composed {A.error_rates(ref, batch, sk, s_pre=to_lsd)}")
    assert np.array_equal(out.download(0, 2 * batch), ref.download(0, 2 * batch))
    for route in ("lincomb", "composition"):                     # the same words whichever way the rows are made
        assert np.array_equal(sl.apply(cts, batch, s_pre=to_msd, route=route).download(0, 2 * batch), ref.download(0, 2 * batch)), route
    with pytest.raises(ValueError):
        sl.apply(cts, batch, route="other")
    got = A.decrypt_batch(out, batch, sk, zp_big, zp_small, 0, 1, s_pre=to_lsd).download(0, batch)
    for b in range(batch):
        slots = G.crt_def([int(x) for x in pts[b, :, 0]], sm, p)
        want = [sum(M[r][c] * slots[c] for c in range(sm.n)) % p for r in range(sm.n)]
        assert G.crt_def([int(x) for x in got[b, :, 0]], sm, p) == want, (setup, kind, b)
    sl.free()
