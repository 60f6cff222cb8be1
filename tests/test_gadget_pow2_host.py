"""CPU: the BaseBGad 2^w gadget (ALCH_GAD_BASEPOW2(w), 1 <= w <= 16) where it needs no GPU.

The closed form of the digits that the three digit loaders use (alchemy_amd/csrc/hint_gadget.hpp: pow2_offset, pow2_digit) against a
sequential divModCent in __int128, and the layout, in a stand-alone program (tests/sanitize/gadget_pow2_harness.cpp) built with
AddressSanitizer and UndefinedBehaviorSanitizer; alch_select_limbs with the library's own KSPNoise rule for the new codes; the codes
that are refused."""
import os
import subprocess

import pytest

import alchemy_amd as A
from alchemy_amd import capi
from conftest import ROOT

RLWR = [1543651201, 689270401, 718099201, 720720001, 1556755201, 1567238401]      # examples/HomomRLWR.hs:37-43


def test_closed_form_digits_and_layout_are_exact_and_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "gadget_pow2_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "sanitize", "gadget_pow2_harness.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("OK: 0 failed expectation(s)")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_the_macro_and_the_header_agree():
    assert capi.ALCH_GAD_BASEPOW2(1) == 0x101 and capi.ALCH_GAD_BASEPOW2(16) == 0x110
    text = open(os.path.join(ROOT, "include", "alchemy_hip.h")).read()
    assert "#define ALCH_GAD_BASEPOW2(w) (0x100 | (w))" in text
    for sym in ("alch_gadget_digits", "alch_decompose_baseb"):
        assert sym in capi.SYMBOLS and hasattr(A.load_library(), sym)


@pytest.mark.parametrize("gadget,want", [
    (capi.ALCH_GAD_BASE2, (4, 3, 3)), (capi.ALCH_GAD_BASEPOW2(1), (4, 3, 3)), (capi.ALCH_GAD_BASEPOW2(2), (4, 4, 3)),
    (capi.ALCH_GAD_BASEPOW2(8), (4, 4, 3)), (capi.ALCH_GAD_BASEPOW2(16), (4, 4, 3)), (capi.ALCH_GAD_TRIV, (4, 5, 3)),
])
def test_select_limbs_with_the_base_pow2_rule(gadget, want):
    """ks_units = p + KSAccumPNoise + ceil((w - 1) / 6.1) on the HomomRLWR moduli at p = 11 (units 5, 4, 4, 4, 5, 5):
    w = 1 needs 13 units (3 limbs), w = 2 and w = 8 need 14 and 15, w = 16 needs 16 (4 limbs each), TrivGad 18 (5 limbs)."""
    assert capi.select_limbs(RLWR, 11, capi.ALCH_OP_MUL, gadget)[:3] == want


@pytest.mark.parametrize("gadget", [capi.ALCH_GAD_BASEPOW2(0), capi.ALCH_GAD_BASEPOW2(17), 2])
def test_select_limbs_refuses_unknown_codes(gadget):
    with pytest.raises(A.AlchemyError) as e:
        capi.select_limbs(RLWR, 11, capi.ALCH_OP_MUL, gadget)
    assert e.value.code == capi.ALCH_E_INVALID and "alch_select_limbs" in str(e.value)
