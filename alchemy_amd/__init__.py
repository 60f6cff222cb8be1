"""alchemy_amd -- MI355X (gfx950) ciphertext-arithmetic backend for ALCHEMY's PT2CT-lowered evaluator.

The product is the C-ABI shared library ``alchemy_amd/lib/libalchemy_hip.so`` (sources in
``alchemy_amd/csrc``, interface in ``include/alchemy_hip.h``).  This package is the thin ctypes binding
used by the tests and bench.py; the host-side mirror of the SymmSHE operations ALCHEMY's evaluator calls is
the C++ header ``alchemy_amd/host/symmshe.hpp`` (the reference's host code is compiled Haskell, so the mirror is
compiled code too).  There is no CPU fallback: importing works anywhere, but every compute
call raises unless the HIP library is built and a gfx950 device is present.
"""
from .capi import AlchemyError, Buf, Hint, Ring, Tunnel, lib_path, load_library  # noqa: F401
from .automorph import (Automorph, AutomorphSet, automorph_hint, automorph_set_hints, automorph_table, buf_automorph,  # noqa: F401
                        ct_automorph, ct_automorph_hoisted, ct_automorph_lincomb)
from .ctadd import CtMeta, align, ct_add, ct_add_raw, ct_neg, ct_sub  # noqa: F401
from .decrypt import decrypt_batch, decrypt_lift, digits_to_int, error_rates, error_term, lift  # noqa: F401
from .encrypt import ct_encrypt, encrypt_batch, gauss_dec, gauss_plan, gauss_table, gen_sk  # noqa: F401
from .hints import ct_ks_hint, ct_ks_hint_part, ks_hint, ks_quad_circ_hint, tunnel_hint, tunnel_values  # noqa: F401
from .mulsteps import ct_mul, key_switch_quad, mod_switch, mul_steps  # noqa: F401
from .slotlinear import SlotLinear, lift_unit, slot_diagonals, unit_split  # noqa: F401
from .plaintext import PtLinear, add_bcast, coeff_bound, pt_eval_lin, pt_linear, pt_mul, pt_rescale, ring_round_plain  # noqa: F401
