"""CPU: the host-only entry points of the encrypt path (alch_gauss_table, alch_gauss_plan) against the Python model written from the
definition (tests/gauss_model.py), bit for bit, and the model's own distribution: the sample covariance of its coefficients against
the toolkit's kron_p ((p I - J) (x) I_{m_p'}).

On the parent commit the library exports neither symbol, so the first three tests fail there."""
import ctypes as C
import math

import numpy as np
import pytest

import gauss_model as GM
from alchemy_amd import capi

PLAN_INDICES = [16, 64, 21, 45, 60, 91, 1365, 11648, 20475]


def svars(m):
    phi = GM.totient(m)
    return [3.0 / math.sqrt(phi), 5.0 / math.sqrt(phi) * 32.0 ** 2]


def lib_plan(m, svar_bits):
    lib = capi.load_library()
    scale, n = C.c_uint64(), C.c_size_t(0)
    rc = lib.alch_gauss_plan(m, svar_bits, C.byref(scale), None, C.byref(n))
    if rc != 0:
        return rc, None, None
    arr = (C.c_uint64 * max(1, n.value))()
    assert lib.alch_gauss_plan(m, svar_bits, C.byref(scale), arr, C.byref(n)) == 0
    return 0, int(scale.value), [int(arr[i]) for i in range(n.value)]


def test_table_equals_the_definition():
    lib = capi.load_library()
    n = C.c_size_t(0)
    assert lib.alch_gauss_table(None, C.byref(n)) == 0
    T = GM.table()
    assert n.value == len(T) == 582
    arr = (C.c_uint64 * n.value)()
    assert lib.alch_gauss_table(arr, C.byref(n)) == 0
    assert [int(v) for v in arr] == list(T)
    assert T[0] == 57493641771463300 and T[580] == 2 ** 63 - 2 and T[581] == 2 ** 63 - 1
    assert all(a <= b for a, b in zip(T, T[1:])) and all(a < b for a, b in zip(T[:500], T[1:501]))
    short = C.c_size_t(581)                                   # an array one entry short is refused, nothing written past it
    assert lib.alch_gauss_table(arr, C.byref(short)) == capi.ALCH_E_INVALID
    assert lib.alch_gauss_table(None, None) == capi.ALCH_E_INVALID


@pytest.mark.parametrize("m", PLAN_INDICES)
def test_plan_equals_the_model_bit_for_bit(m):
    for svar in svars(m):
        rc, scale, chol = lib_plan(m, GM.bits(svar))
        assert rc == 0
        n, want_scale, axes = GM.plan(m, svar)
        assert scale == GM.bits(want_scale), (m, svar)
        want = [GM.bits(v) for _, _, _, Lc in axes for row in Lc for v in row]
        assert chol == want, (m, svar)
        assert len(chol) == sum((p - 1) ** 2 for p, e in GM.factor(m) if p != 2)


def test_plan_statuses():
    lib = capi.load_library()
    n = C.c_size_t(0)
    for bad in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        assert lib.alch_gauss_plan(21, GM.bits(bad), None, None, C.byref(n)) == capi.ALCH_E_INVALID, bad
    assert lib.alch_gauss_plan(0, GM.bits(1.0), None, None, C.byref(n)) == capi.ALCH_E_INVALID
    assert lib.alch_gauss_plan(21, GM.bits(5e-324), None, None, C.byref(n)) == 0 and n.value == 4 + 36     # the smallest positive double
    arr, short = (C.c_uint64 * 40)(), C.c_size_t(39)
    assert lib.alch_gauss_plan(21, GM.bits(1.0), None, arr, C.byref(short)) == capi.ALCH_E_INVALID
    assert lib.alch_gauss_plan(21, GM.bits(1.0), None, arr, None) == capi.ALCH_E_INVALID
    assert lib.alch_gauss_plan(16, GM.bits(1.0), None, None, C.byref(n)) == 0 and n.value == 0              # no odd prime


def expected_covariance(m):
    """kron over the primes of m (ascending, first outermost) of (p I - J) (x) I_{m_p'}; p = 2 gives I."""
    E = np.ones((1, 1))
    for p, e in GM.factor(m):
        h, mp = p - 1, p ** (e - 1)
        E = np.kron(E, np.kron(p * np.eye(h) - np.ones((h, h)), np.eye(mp)))
    return E


@pytest.mark.parametrize("m", [7, 9, 21])
def test_covariance_of_the_model_is_the_toolkits(m):
    """20 000 elements of a fixed seed: every entry of the sample covariance / sigma^2 within 5 standard errors
    sqrt((C_ii C_jj + C_ij^2) / N) of the expected matrix."""
    N, svar = 20000, 4.0
    x = GM.raw(m, svar, seed=0x5EED0000 + m, elem0=0, count=N)
    rad = 1
    for p, _ in GM.factor(m):
        rad *= p
    sigma2 = svar * (m // rad) / (2.0 * math.pi)
    S = (x.T @ x) / N / sigma2                               # the mean is zero by construction
    Cx = expected_covariance(m)
    se = np.sqrt((np.outer(np.diag(Cx), np.diag(Cx)) + Cx ** 2) / N)
    dev = np.abs(S - Cx) / se
    print("m = %d: largest deviation %.2f standard errors" % (m, dev.max()))
    assert dev.max() <= 5.0, dev.max()
    assert abs(x.mean()) <= 5.0 * math.sqrt(sigma2 * Cx.diagonal().max() / x.size)
