"""CPU: the step entry points of mul_ (alch_ct_mul, alch_ct_key_switch_quad, alch_ct_mod_switch_deg) exist at every layer a host
reaches them through -- the C header, the built library, the ctypes binding and its Python wrappers, the Haskell FFI module -- with
one signature.  None of the three names exists anywhere before the feature, so each test fails on the parent commit."""
import ctypes as C
import os
import re

from conftest import ROOT

STEPS = {
    "alch_ct_mul": ["alch_ring*", "alch_buf*", "alch_buf*", "alch_buf*", "size_t", "uint64_t*", "unsigned"],
    "alch_ct_key_switch_quad": ["alch_hint*", "alch_buf*", "alch_buf*", "size_t", "uint64_t*", "unsigned"],
    "alch_ct_mod_switch_deg": ["alch_buf*", "alch_buf*", "size_t", "int", "unsigned"],
}


def test_header_declares_the_three_entry_points():
    from test_haskell_shim import header_prototypes
    protos = header_prototypes()
    for name, params in STEPS.items():
        assert protos.get(name) == ("int", params), (name, protos.get(name))
    text = open(os.path.join(ROOT, "include", "alchemy_hip.h")).read()
    assert re.search(r"added\s+WITHIN\s+1\.8", text) and "probes for the symbols" in text


def test_library_exports_them_and_capi_binds_them():
    from alchemy_amd import capi
    lib = capi.load_library()
    ctype = {"alch_ring*": C.c_void_p, "alch_buf*": C.c_void_p, "alch_hint*": C.c_void_p, "size_t": C.c_size_t,
             "uint64_t*": C.POINTER(C.c_uint64), "unsigned": C.c_uint, "int": C.c_int}
    for name, params in STEPS.items():
        assert name in capi.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [ctype[p] for p in params], name
    assert lib.alch_version() == (1 << 16) | 8


def test_package_exports_the_step_functions():
    import alchemy_amd as A
    from alchemy_amd import mulsteps
    for name in ("ct_mul", "key_switch_quad", "mod_switch", "mul_steps"):
        assert getattr(A, name) is getattr(mulsteps, name)


def test_null_handles_are_refused_without_a_device():
    """The argument checks come before any device work: null handles give ALCH_E_INVALID and a message on a machine without a GPU."""
    from alchemy_amd import capi
    lib = capi.load_library()
    assert lib.alch_ct_mul(None, None, None, None, 1, None, 0) == capi.ALCH_E_INVALID and lib.alch_last_error()
    assert lib.alch_ct_key_switch_quad(None, None, None, 1, None, 0) == capi.ALCH_E_INVALID
    assert lib.alch_ct_mod_switch_deg(None, None, 1, 2, 0) == capi.ALCH_E_INVALID


def test_backend_hs_imports_them():
    from test_haskell_shim import CTYPE, haskell_imports
    imps = haskell_imports()
    for name, params in STEPS.items():
        assert name in imps, name
        safety, sig = imps[name]
        assert safety == "safe" and sig == [CTYPE[p] for p in params] + ["IO CInt"], (name, sig)


def test_host_mirror_and_replay_use_them():
    hpp = open(os.path.join(ROOT, "alchemy_amd", "host", "symmshe.hpp")).read()
    for fn, sym in (("ctMulBatch", "alch_ct_mul("), ("keySwitchQuadBatch", "alch_ct_key_switch_quad("), ("modSwitchDegBatch", "alch_ct_mod_switch_deg(")):
        assert fn in hpp and sym in hpp, fn
    cpp = open(os.path.join(ROOT, "examples", "arithmetic_replay.cpp")).read()
    assert '"--steps"' in cpp
