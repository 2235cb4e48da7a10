"""The whole launch table of every gadget (one-limb-digit) key-switch call: the
launch count of EVERY kernel name the profiler knows, after one warm run, on
one ring per host branch -- 2^9 (four-step, untiled: the rescaling multiply's
two-temporary fallback), 2^12 (whole-plane: `ks_whole`, the composed bodies),
2^14 (tiled four-step: the fused rescale epilogue, the fused bodies) and 2^16
(matrix cores) -- chunked, with the rotation's sigma(c0) gather fused and not,
and with steps that are all zero.  These tables pin which kernels a call runs
and how often, so a rewrite of the host pipeline that adds, drops or repeats a
launch fails here.  Chunked (1 MiB of key-switch workspace, three ciphertexts,
where a ciphertext's S alone is 9 * 2^14 * 4 B = 576 KiB), every sizing formula
of a full-basis call floors at one ciphertext a chunk, and its `ks_decompose`
count is a multiple of the three chunks; rnt_keyswitch_ext, whose S has only
L - 1 target limbs here, runs two chunks (2 + 1 ciphertexts).  `copy_rows` is a memcpy and not a counted launch; the
bit-exact suites cover it.

The expected tables are literals.  They were recorded with `record()` of
test_gpu_hybrid_launch_tables on the commit BEFORE the gadget calls were moved
onto shared stage helpers (commit a954674, "Add ModRaise, X^k products and
CoeffToSlot / SlotToCoeff transforms"), never from the rewritten code; a
kernel that is not named in a table ran zero times.  `ct_mul_relin` is pinned
in test_gpu_hybrid_launch_tables.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import test_gpu_bsgs
import test_gpu_hoist
import test_gpu_linear
from test_gpu_hybrid_launch_tables import record

pytestmark = pytest.mark.gpu

L, BITS = 3, 31


# The fixtures, one of each kind per (ring, batch, environment): the contexts
# read RNT_KS_WS_MB and RNT_ROT_FUSE when they are created.
@functools.lru_cache(maxsize=None)
def _linear(rn, log_n, B, env, steps=tuple(test_gpu_linear.STEPS)):
    return test_gpu_linear.Case(rn, log_n, L, B, BITS, steps=list(steps), seed=11)


@functools.lru_cache(maxsize=None)
def _bsgs_case(rn, log_n, B, env):
    baby, giant = test_gpu_bsgs.SMALL if log_n >= 16 else (test_gpu_bsgs.BABY, test_gpu_bsgs.GIANT)
    return test_gpu_bsgs.Case(rn, log_n, L, B, BITS, baby=baby, giant=giant, seed=11)


@functools.lru_cache(maxsize=None)
def _hoist(rn, log_n, B, env, steps=None):
    if steps is None:
        steps = test_gpu_hoist.SMALL if log_n >= 16 else test_gpu_hoist.STEPS
    return test_gpu_hoist.Case(rn, log_n, L, B, BITS, steps=list(steps), seed=11)


@functools.lru_cache(maxsize=None)
def _bsgs_hoist(rn, log_n, B, env):
    baby, giant = test_gpu_hoist.SMALL_BSGS if log_n >= 16 else (test_gpu_hoist.BABY, test_gpu_hoist.GIANT)
    return test_gpu_hoist.BsgsCase(rn, log_n, L, B, BITS, baby=baby, giant=giant, seed=11)


# call -> (basis, run) on the fixtures of (rn, log_n, B, env)
def _keyswitch(rn, *a):
    c = _linear(rn, *a)
    return c.basis, lambda: rn.keyswitch(c.ct.c1, c.gk[1])


def _keyswitch_ext(rn, *a):
    """L - 1 target limbs (a limb shard) over the L source limbs."""
    c = _linear(rn, *a)
    if not hasattr(c, "ext"):
        Lt = L - 1
        Bt = rn.RnsBasis(c.mod[:Lt], c.n)
        ka, kb = c.keys[1]
        key_t = rn.RnsGadgetKey.from_channels(np.ascontiguousarray(ka[:, :Lt]), np.ascontiguousarray(kb[:, :Lt]), Bt)
        c.ext = (Bt, key_t, rn.RnsPoly(Bt, c.B), rn.RnsPoly(Bt, c.B))
    Bt, key_t, o0, o1 = c.ext
    ptr, _ = c.ct.c1.device_ptr()
    return Bt, lambda: rn.keyswitch_ext(ptr, L, key_t, Bt, c.B, out0=o0, out1=o1)


def _rotate(rn, *a):
    c = _linear(rn, *a)
    return c.basis, lambda: rn.rotate_ciphertext(c.ct, c.gk[2])  # step -3


def _mul_rescale(rn, *a):
    c = _linear(rn, *a)
    ct2 = rn.Ciphertext(c.ct.c1, c.ct.c0)
    return c.basis, lambda: rn.mul_ciphertexts_gadget_rescale(c.ct, ct2, c.gk[1])


def _linear_transform(rn, *a):
    c = _linear(rn, *a)
    return c.basis, lambda: rn.linear_transform(c.ct, c.d, c.keyset)


def _linear_zero(rn, *a):
    c = _linear(rn, *a, steps=(0, 0))  # no keys at all
    return c.basis, lambda: rn.linear_transform(c.ct, c.d, c.keyset)


def _hoisted(rn, *a):
    c = _hoist(rn, *a)
    return c.basis, c.run


def _hoisted_zero(rn, *a):
    c = _hoist(rn, *a, steps=(0, 0))  # no keys at all
    return c.basis, c.run


def _bsgs(rn, *a):
    c = _bsgs_case(rn, *a)
    return c.basis, c.run


def _bsgs_hoisted(rn, *a):
    c = _bsgs_hoist(rn, *a)
    return c.basis, c.run


CALLS = {
    "keyswitch": _keyswitch, "keyswitch_ext": _keyswitch_ext, "ct_rotate": _rotate,
    "ct_mul_relin_rescale": _mul_rescale, "ct_linear": _linear_transform, "ct_rotate_hoisted": _hoisted,
    "ct_linear_bsgs": _bsgs, "ct_linear_bsgs_hoisted": _bsgs_hoisted,
    "ct_linear(zero steps)": _linear_zero, "ct_rotate_hoisted(zero steps)": _hoisted_zero,
}

CHUNKED = (("RNT_KS_WS_MB", "1"),)
UNFUSED = (("RNT_ROT_FUSE", "0"),)
# (call, log_n, B, environment)
CASES = [(call, log_n, 2, ()) for log_n in (9, 12, 14, 16) for call in list(CALLS)[:8]]
# one ciphertext: sigma(c0) is gathered by the key-switch inverse (fuse0), or not
CASES += [("ct_rotate", 14, 1, ()), ("ct_rotate", 14, 1, UNFUSED)]
# 1 MiB of key-switch workspace, three ciphertexts: three chunks of one
CASES += [(call, 14, 3, CHUNKED) for call in list(CALLS)[:8]]
CASES += [("ct_linear(zero steps)", 14, 2, ()), ("ct_rotate_hoisted(zero steps)", 14, 2, ())]


def case_id(case):
    call, log_n, B, env = case
    return f"{call}-2^{log_n}-B{B}" + "".join(f"-{k}={v}" for k, v in env)


EXPECTED = {
    "keyswitch-2^9-B2": {"col_inv": 2, "ks_decompose": 1, "ks_rows": 1},
    "keyswitch_ext-2^9-B2": {"col_inv": 2, "ks_decompose": 1, "ks_rows": 1},
    "ct_rotate-2^9-B2": {"col_inv": 2, "automorphism": 2, "ks_decompose": 1, "ks_rows": 1},
    "ct_mul_relin_rescale-2^9-B2": {"col_fwd": 2, "col_inv": 3, "rescale": 2, "ks_decompose": 1, "ks_rows": 1,
                                    "tensor_rows": 1},
    "ct_linear-2^9-B2": {"col_fwd": 6, "row_fwd": 6, "row_inv": 2, "col_inv": 4, "elementwise": 7, "automorphism": 8,
                         "ks_decompose": 4, "ks_rows": 4},
    "ct_rotate_hoisted-2^9-B2": {"col_fwd": 1, "row_fwd": 1, "row_inv": 10, "col_inv": 10, "automorphism": 10,
                                 "copy": 12, "hoist_digits": 1, "hoist_mac": 2},
    "ct_linear_bsgs-2^9-B2": {"col_fwd": 11, "row_fwd": 11, "row_inv": 8, "col_inv": 16, "elementwise": 5,
                              "automorphism": 12, "ks_decompose": 6, "ks_rows": 6, "bsgs_mac": 1},
    "ct_linear_bsgs_hoisted-2^9-B2": {"col_fwd": 12, "row_fwd": 12, "row_inv": 14, "col_inv": 16, "elementwise": 5,
                                      "automorphism": 12, "ks_decompose": 3, "ks_rows": 3, "bsgs_mac": 1,
                                      "hoist_digits": 1, "hoist_mac": 1},
    "keyswitch-2^12-B2": {"ks_whole": 1},
    "keyswitch_ext-2^12-B2": {"ks_whole": 1},
    "ct_rotate-2^12-B2": {"automorphism": 2, "ks_whole": 1},
    "ct_mul_relin_rescale-2^12-B2": {"rescale": 2, "ks_whole": 1, "tensor_whole": 1},
    "ct_linear-2^12-B2": {"elementwise": 11, "automorphism": 8, "whole_fwd": 10, "whole_inv": 2, "ks_whole": 4},
    "ct_rotate_hoisted-2^12-B2": {"elementwise": 5, "automorphism": 10, "copy": 12, "whole_fwd": 1, "whole_inv": 10,
                                  "hoist_digits": 1, "hoist_mac": 2},
    "ct_linear_bsgs-2^12-B2": {"elementwise": 7, "automorphism": 12, "whole_fwd": 8, "whole_inv": 8, "ks_whole": 6,
                               "bsgs_mac": 1},
    "ct_linear_bsgs_hoisted-2^12-B2": {"elementwise": 10, "automorphism": 12, "whole_fwd": 9, "whole_inv": 14,
                                       "ks_whole": 3, "bsgs_mac": 1, "hoist_digits": 1, "hoist_mac": 1},
    "keyswitch-2^14-B2": {"col_inv": 2, "ks_decompose": 1, "ks_rows": 1},
    "keyswitch_ext-2^14-B2": {"col_inv": 2, "ks_decompose": 1, "ks_rows": 1},
    "ct_rotate-2^14-B2": {"col_inv": 2, "automorphism": 2, "ks_decompose": 1, "ks_rows": 1},
    "ct_mul_relin_rescale-2^14-B2": {"col_fwd": 2, "col_inv": 5, "ks_decompose": 1, "ks_rows": 1, "tensor_rows": 1},
    "ct_linear-2^14-B2": {"col_inv": 2, "elementwise": 7, "automorphism": 8, "ks_decompose": 4, "ks_rows": 4,
                          "whole_fwd": 6, "whole_inv": 2},
    "ct_rotate_hoisted-2^14-B2": {"elementwise": 5, "automorphism": 10, "copy": 12, "whole_fwd": 1, "whole_inv": 10,
                                  "hoist_digits": 1, "hoist_mac": 2},
    "ct_linear_bsgs-2^14-B2": {"col_inv": 8, "elementwise": 5, "automorphism": 12, "ks_decompose": 6, "ks_rows": 6,
                               "whole_fwd": 11, "whole_inv": 8, "bsgs_mac": 1},
    "ct_linear_bsgs_hoisted-2^14-B2": {"col_inv": 2, "elementwise": 8, "automorphism": 12, "ks_decompose": 3,
                                       "ks_rows": 3, "whole_fwd": 12, "whole_inv": 14, "bsgs_mac": 1,
                                       "hoist_digits": 1, "hoist_mac": 1},
    "keyswitch-2^16-B2": {"col_inv": 2, "ks_decompose": 1, "ks_rows": 1},
    "keyswitch_ext-2^16-B2": {"col_inv": 2, "ks_decompose": 1, "ks_rows": 1},
    "ct_rotate-2^16-B2": {"col_inv": 2, "automorphism": 2, "ks_decompose": 1, "ks_rows": 1},
    "ct_mul_relin_rescale-2^16-B2": {"col_inv": 4, "ks_decompose": 1, "ks_rows": 1, "mf_tensor": 1},
    "ct_linear-2^16-B2": {"col_inv": 2, "elementwise": 7, "automorphism": 8, "ks_decompose": 4, "ks_rows": 4,
                          "mf_ntt_fwd": 6, "mf_ntt_inv": 2},
    "ct_rotate_hoisted-2^16-B2": {"elementwise": 2, "automorphism": 4, "copy": 6, "mf_ntt_fwd": 1, "mf_ntt_inv": 4,
                                  "hoist_digits": 1, "hoist_mac": 1},
    "ct_linear_bsgs-2^16-B2": {"col_inv": 4, "elementwise": 4, "automorphism": 6, "ks_decompose": 3, "ks_rows": 3,
                               "mf_ntt_fwd": 6, "mf_ntt_inv": 6, "bsgs_mac": 1},
    "ct_linear_bsgs_hoisted-2^16-B2": {"col_inv": 2, "elementwise": 5, "automorphism": 6, "ks_decompose": 2,
                                       "ks_rows": 2, "mf_ntt_fwd": 7, "mf_ntt_inv": 8, "bsgs_mac": 1,
                                       "hoist_digits": 1, "hoist_mac": 1},
    # one ciphertext: fuse0, one automorphism launch, not two
    "ct_rotate-2^14-B1": {"col_inv": 2, "automorphism": 1, "ks_decompose": 1, "ks_rows": 1},
    "ct_rotate-2^14-B1-RNT_ROT_FUSE=0": {"col_inv": 2, "automorphism": 2, "ks_decompose": 1, "ks_rows": 1},
    # chunked: ks_decompose is a multiple of the three chunks.  rnt_keyswitch_ext alone runs two: its S is
    # [Lt][Ls] = 2 x 3 planes a ciphertext, 384 KiB, so two ciphertexts fit its first chunk (2 + 1)
    "keyswitch-2^14-B3-RNT_KS_WS_MB=1": {"col_inv": 6, "ks_decompose": 3, "ks_rows": 3},
    "keyswitch_ext-2^14-B3-RNT_KS_WS_MB=1": {"col_inv": 4, "ks_decompose": 2, "ks_rows": 2},
    "ct_rotate-2^14-B3-RNT_KS_WS_MB=1": {"col_inv": 6, "automorphism": 2, "ks_decompose": 3, "ks_rows": 3},
    "ct_mul_relin_rescale-2^14-B3-RNT_KS_WS_MB=1": {"col_fwd": 6, "col_inv": 15, "ks_decompose": 3, "ks_rows": 3,
                                                    "tensor_rows": 3},
    "ct_linear-2^14-B3-RNT_KS_WS_MB=1": {"col_inv": 6, "elementwise": 19, "automorphism": 24, "ks_decompose": 12,
                                         "ks_rows": 12, "whole_fwd": 18, "whole_inv": 6},
    "ct_rotate_hoisted-2^14-B3-RNT_KS_WS_MB=1": {"elementwise": 15, "automorphism": 30, "copy": 35, "whole_fwd": 3,
                                                 "whole_inv": 30, "hoist_digits": 3, "hoist_mac": 6},
    "ct_linear_bsgs-2^14-B3-RNT_KS_WS_MB=1": {"col_inv": 24, "elementwise": 11, "automorphism": 36,
                                              "ks_decompose": 18, "ks_rows": 18, "whole_fwd": 33, "whole_inv": 24,
                                              "bsgs_mac": 3},
    "ct_linear_bsgs_hoisted-2^14-B3-RNT_KS_WS_MB=1": {"col_inv": 6, "elementwise": 20, "automorphism": 36,
                                                      "ks_decompose": 9, "ks_rows": 9, "whole_fwd": 36,
                                                      "whole_inv": 42, "bsgs_mac": 3, "hoist_digits": 3,
                                                      "hoist_mac": 3},
    # every step zero, no keys: no key-switch at all
    "ct_linear(zero steps)-2^14-B2": {"elementwise": 5, "whole_fwd": 2, "whole_inv": 2},
    "ct_rotate_hoisted(zero steps)-2^14-B2": {"copy": 4},
}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_launch_table(gpu, monkeypatch, case):
    call, log_n, B, env = case
    for k, v in env:
        monkeypatch.setenv(k, v)  # read at rnt_ctx_create
    basis, run = CALLS[call](gpu, log_n, B, env)
    got = record(basis, run)
    print(case_id(case), got)
    assert got == EXPECTED[case_id(case)]


def test_every_case_has_a_table_and_every_table_a_case():
    assert sorted(EXPECTED) == sorted(case_id(c) for c in CASES)
