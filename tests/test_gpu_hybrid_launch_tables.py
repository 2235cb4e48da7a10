"""The whole launch table of every hybrid key-switch call, of the gadget
multiply and of the tensor: the launch count of EVERY kernel name the profiler
knows, after one warm run, at the smallest ring of each transform family
(2^9 four-step, 2^12 whole-plane, 2^16 matrix cores), chunked, with the
un-fused hoisted tail and with steps that are all zero.  The other launch-count
tests assert a few kernels each; these tables pin which kernels a call runs and
how often, so a rewrite of the host pipeline that adds, drops or repeats a
launch fails here.  Chunked, the number of `modup` launches is the number of
chunks, which pins the chunk size.

The expected tables are literals.  They were recorded with `record()` below on
the commit BEFORE the hybrid calls were moved onto shared stage helpers (commit
4e0ac60, "Test every op family on word-aligned buffers"), never from the
rewritten code; a kernel that is not named in a table ran zero times.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from test_gpu_dot_hybrid import DotCase
from test_gpu_hoist import SMALL as STEPS_SMALL
from test_gpu_hybrid import Case, _rand
from test_gpu_hybrid_hoist import BABY, GIANT, SMALL_BSGS, STEPS, BsgsCase
from test_gpu_hybrid_hoist import Case as HoistCase

pytestmark = pytest.mark.gpu

# kKernelNames (csrc/rnt_api.cpp); rnt_profile_read refuses a name it does not know
KERNELS = ("col_fwd", "row_fwd", "row_inv", "row_mul", "col_inv", "elementwise", "rescale", "automorphism",
           "ks_decompose", "ks_rows", "tensor_rows", "import", "export", "crt", "sfft", "sample", "copy", "plane_fused",
           "mf_ntt_fwd", "mf_ntt_inv", "whole_fwd", "whole_inv", "whole_mul", "ks_whole", "tensor_whole", "mf_tensor",
           "mf_mul", "bsgs_mac", "hoist_digits", "hoist_mac", "modup", "moddown", "moddown_auto", "moddown_rescale",
           "lincomb", "dot_tensor")

LV, K, ALPHA, BITS, N_TERMS = 3, 2, 2, 31, 3


def record(basis, run):
    """{kernel: launches} of one run after a warm one, zero counts left out."""
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in KERNELS}
    basis.profile_enable(False)
    return {k: v for k, v in counts.items() if v}


# The fixtures, one of each kind per (ring, batch, environment): the contexts
# read RNT_KS_WS_MB and RNT_MODDOWN_AUTO when they are created.
@functools.lru_cache(maxsize=None)
def _case(rn, log_n, B, env):
    return Case(rn, log_n, LV, K, ALPHA, B, BITS, seed=11)


@functools.lru_cache(maxsize=None)
def _dot(rn, log_n, B, env):
    return DotCase(rn, log_n, LV, K, ALPHA, B, BITS, N_TERMS, seed=11)


@functools.lru_cache(maxsize=None)
def _hoist(rn, log_n, B, env, steps):
    return HoistCase(rn, log_n, LV, K, ALPHA, B, BITS, steps=list(steps), seed=11)


@functools.lru_cache(maxsize=None)
def _bsgs(rn, log_n, B, env):
    baby, giant = SMALL_BSGS if log_n >= 16 else (BABY, GIANT)
    return BsgsCase(rn, log_n, LV, K, ALPHA, B, BITS, baby=baby, giant=giant, seed=11)


def _steps(log_n):
    return tuple(STEPS_SMALL if log_n >= 16 else STEPS)


def _gadget_key(c):
    rng = np.random.default_rng(90)
    return c.rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.Lv), _rand(rng, c.mod, c.n, c.Lv), c.basis)


# call -> (basis, run) on the fixtures of (rn, log_n, B, env)
def _keyswitch(rn, *a):
    c = _case(rn, *a)
    return c.basis, lambda: rn.keyswitch_hybrid(c.ct.c1, c.key)


def _rotate(rn, *a):
    c = _case(rn, *a)
    return c.basis, lambda: rn.rotate_ciphertext_hybrid(c.ct, c.key)  # step -3


def _mul(rn, *a):
    c = _case(rn, *a)
    return c.basis, lambda: rn.mul_ciphertexts_hybrid(c.ct, c.ctp, c.key)


def _mul_rescale(rn, *a):
    c = _case(rn, *a)
    low = c.basis.drop_last(1)
    return c.basis, lambda: rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key, out_basis=low)


def _dot_plain(rn, *a):
    c = _dot(rn, *a)
    return c.basis, lambda: rn.dot_ciphertexts_hybrid(c.ctx, c.cty, c.nt, c.key, rescale=False)


def _dot_rescale(rn, *a):
    c = _dot(rn, *a)
    low = c.basis.drop_last(1)
    return c.basis, lambda: rn.dot_ciphertexts_hybrid(c.ctx, c.cty, c.nt, c.key, rescale=True, out_basis=low)


def _hoisted(rn, log_n, B, env):
    c = _hoist(rn, log_n, B, env, _steps(log_n))
    return c.basis, c.run


def _hoisted_zero(rn, log_n, B, env):
    c = _hoist(rn, log_n, B, env, (0, 0))  # no keys at all
    assert c.kset.a is None and c.kset.b is None
    return c.basis, c.run


def _bsgs_plain(rn, *a):
    c = _bsgs(rn, *a)
    return c.basis, c.run


def _bsgs_rescale(rn, *a):
    c = _bsgs(rn, *a)
    return c.basis, lambda: rn.linear_transform_bsgs_hybrid_rescale(c.ct, c.d, c.bset, c.gset)


def _gadget_mul(rn, *a):
    c = _case(rn, *a)
    gk = _gadget_key(c)
    return c.basis, lambda: rn.mul_ciphertexts_gadget(c.ct, c.ctp, gk)


def _tensor(rn, *a):
    c = _case(rn, *a)
    return c.basis, lambda: rn.ct_tensor(c.ct.c0, c.ct.c1, c.ctp.c0, c.ctp.c1)


CALLS = {
    "keyswitch_hybrid": _keyswitch, "ct_rotate_hybrid": _rotate, "ct_mul_relin_hybrid": _mul,
    "ct_mul_relin_rescale_hybrid": _mul_rescale, "ct_dot_relin_hybrid": _dot_plain,
    "ct_dot_relin_rescale_hybrid": _dot_rescale, "ct_rotate_hybrid_hoisted": _hoisted,
    "ct_linear_bsgs_hybrid": _bsgs_plain, "ct_linear_bsgs_hybrid_rescale": _bsgs_rescale,
    "ct_mul_relin": _gadget_mul, "ct_tensor": _tensor, "ct_rotate_hybrid_hoisted(zero steps)": _hoisted_zero,
}

CHUNKED = (("RNT_KS_WS_MB", "1"),)
UNFUSED = (("RNT_MODDOWN_AUTO", "0"),)
# (call, log_n, B, environment)
CASES = [(call, log_n, 2, ()) for log_n in (9, 12, 16) for call in list(CALLS)[:11]]
# one chunked case per pipeline: 1 MiB of key-switch workspace, three ciphertexts
CASES += [(call, 12, 3, CHUNKED) for call in ("keyswitch_hybrid", "ct_mul_relin_hybrid", "ct_mul_relin_rescale_hybrid",
                                              "ct_dot_relin_hybrid", "ct_dot_relin_rescale_hybrid",
                                              "ct_rotate_hybrid_hoisted", "ct_linear_bsgs_hybrid",
                                              "ct_linear_bsgs_hybrid_rescale")]
CASES += [("ct_rotate_hybrid_hoisted", 12, 2, UNFUSED), ("ct_linear_bsgs_hybrid", 12, 2, UNFUSED),
          ("ct_rotate_hybrid_hoisted(zero steps)", 12, 2, ())]


def case_id(case):
    call, log_n, B, env = case
    return f"{call}-2^{log_n}-B{B}" + "".join(f"-{k}={v}" for k, v in env)


EXPECTED = {
    "keyswitch_hybrid-2^9-B2": {"col_fwd": 1, "row_fwd": 1, "row_inv": 2, "col_inv": 2, "hoist_mac": 1, "modup": 1,
                                "moddown": 2},
    "ct_rotate_hybrid-2^9-B2": {"col_fwd": 1, "row_fwd": 1, "row_inv": 2, "col_inv": 2, "automorphism": 2,
                                "hoist_mac": 1, "modup": 1, "moddown": 2},
    "ct_mul_relin_hybrid-2^9-B2": {"col_fwd": 3, "row_fwd": 1, "row_inv": 4, "col_inv": 5, "elementwise": 2,
                                   "tensor_rows": 1, "hoist_mac": 1, "modup": 1, "moddown": 2},
    "ct_mul_relin_rescale_hybrid-2^9-B2": {"col_fwd": 3, "row_fwd": 1, "row_inv": 2, "col_inv": 3, "tensor_rows": 1,
                                           "hoist_mac": 1, "modup": 1, "moddown_rescale": 2},
    "ct_dot_relin_hybrid-2^9-B2": {"col_fwd": 5, "row_fwd": 5, "row_inv": 5, "col_inv": 5, "elementwise": 3, "copy": 4,
                                   "hoist_mac": 1, "modup": 1, "moddown": 2, "dot_tensor": 1},
    "ct_dot_relin_rescale_hybrid-2^9-B2": {"col_fwd": 5, "row_fwd": 5, "row_inv": 3, "col_inv": 3, "elementwise": 1,
                                           "copy": 4, "hoist_mac": 1, "modup": 1, "moddown_rescale": 2,
                                           "dot_tensor": 1},
    "ct_rotate_hybrid_hoisted-2^9-B2": {"col_fwd": 1, "row_fwd": 1, "row_inv": 10, "col_inv": 10, "copy": 2,
                                        "hoist_mac": 2, "modup": 1, "moddown_auto": 10},
    "ct_linear_bsgs_hybrid-2^9-B2": {"col_fwd": 9, "row_fwd": 9, "row_inv": 12, "col_inv": 12, "elementwise": 3,
                                     "automorphism": 4, "bsgs_mac": 2, "hoist_mac": 3, "modup": 3, "moddown": 2,
                                     "moddown_auto": 4},
    "ct_linear_bsgs_hybrid_rescale-2^9-B2": {"col_fwd": 9, "row_fwd": 9, "row_inv": 12, "col_inv": 12,
                                             "elementwise": 3, "automorphism": 4, "bsgs_mac": 2, "hoist_mac": 3,
                                             "modup": 3, "moddown_auto": 4, "moddown_rescale": 2},
    "ct_mul_relin-2^9-B2": {"col_fwd": 2, "col_inv": 3, "ks_decompose": 1, "ks_rows": 1, "tensor_rows": 1},
    "ct_tensor-2^9-B2": {"col_fwd": 2, "col_inv": 1, "tensor_rows": 1},
    "keyswitch_hybrid-2^12-B2": {"whole_fwd": 1, "whole_inv": 2, "hoist_mac": 1, "modup": 1, "moddown": 2},
    "ct_rotate_hybrid-2^12-B2": {"automorphism": 2, "whole_fwd": 1, "whole_inv": 2, "hoist_mac": 1, "modup": 1,
                                 "moddown": 2},
    "ct_mul_relin_hybrid-2^12-B2": {"elementwise": 2, "whole_fwd": 1, "whole_inv": 4, "tensor_whole": 1,
                                    "hoist_mac": 1, "modup": 1, "moddown": 2},
    "ct_mul_relin_rescale_hybrid-2^12-B2": {"whole_fwd": 1, "whole_inv": 2, "tensor_whole": 1, "hoist_mac": 1,
                                            "modup": 1, "moddown_rescale": 2},
    "ct_dot_relin_hybrid-2^12-B2": {"elementwise": 3, "copy": 4, "whole_fwd": 5, "whole_inv": 5, "hoist_mac": 1,
                                    "modup": 1, "moddown": 2, "dot_tensor": 1},
    "ct_dot_relin_rescale_hybrid-2^12-B2": {"elementwise": 1, "copy": 4, "whole_fwd": 5, "whole_inv": 3,
                                            "hoist_mac": 1, "modup": 1, "moddown_rescale": 2, "dot_tensor": 1},
    "ct_rotate_hybrid_hoisted-2^12-B2": {"copy": 2, "whole_fwd": 1, "whole_inv": 10, "hoist_mac": 2, "modup": 1,
                                         "moddown_auto": 10},
    "ct_linear_bsgs_hybrid-2^12-B2": {"elementwise": 3, "automorphism": 4, "whole_fwd": 9, "whole_inv": 12,
                                      "bsgs_mac": 2, "hoist_mac": 3, "modup": 3, "moddown": 2, "moddown_auto": 4},
    "ct_linear_bsgs_hybrid_rescale-2^12-B2": {"elementwise": 3, "automorphism": 4, "whole_fwd": 9, "whole_inv": 12,
                                              "bsgs_mac": 2, "hoist_mac": 3, "modup": 3, "moddown_auto": 4,
                                              "moddown_rescale": 2},
    "ct_mul_relin-2^12-B2": {"ks_whole": 1, "tensor_whole": 1},
    "ct_tensor-2^12-B2": {"tensor_whole": 1},
    "keyswitch_hybrid-2^16-B2": {"mf_ntt_fwd": 1, "mf_ntt_inv": 2, "hoist_mac": 1, "modup": 1, "moddown": 2},
    "ct_rotate_hybrid-2^16-B2": {"automorphism": 2, "mf_ntt_fwd": 1, "mf_ntt_inv": 2, "hoist_mac": 1, "modup": 1,
                                 "moddown": 2},
    "ct_mul_relin_hybrid-2^16-B2": {"elementwise": 2, "mf_ntt_fwd": 1, "mf_ntt_inv": 4, "mf_tensor": 1,
                                    "hoist_mac": 1, "modup": 1, "moddown": 2},
    "ct_mul_relin_rescale_hybrid-2^16-B2": {"mf_ntt_fwd": 1, "mf_ntt_inv": 2, "mf_tensor": 1, "hoist_mac": 1,
                                            "modup": 1, "moddown_rescale": 2},
    "ct_dot_relin_hybrid-2^16-B2": {"elementwise": 3, "copy": 4, "mf_ntt_fwd": 5, "mf_ntt_inv": 5, "hoist_mac": 1,
                                    "modup": 1, "moddown": 2, "dot_tensor": 1},
    "ct_dot_relin_rescale_hybrid-2^16-B2": {"elementwise": 1, "copy": 4, "mf_ntt_fwd": 5, "mf_ntt_inv": 3,
                                            "hoist_mac": 1, "modup": 1, "moddown_rescale": 2, "dot_tensor": 1},
    "ct_rotate_hybrid_hoisted-2^16-B2": {"copy": 2, "mf_ntt_fwd": 1, "mf_ntt_inv": 4, "hoist_mac": 1, "modup": 1,
                                         "moddown_auto": 4},
    "ct_linear_bsgs_hybrid-2^16-B2": {"elementwise": 2, "automorphism": 2, "mf_ntt_fwd": 6, "mf_ntt_inv": 8,
                                      "bsgs_mac": 1, "hoist_mac": 2, "modup": 2, "moddown": 2, "moddown_auto": 2},
    "ct_linear_bsgs_hybrid_rescale-2^16-B2": {"elementwise": 2, "automorphism": 2, "mf_ntt_fwd": 6, "mf_ntt_inv": 8,
                                              "bsgs_mac": 1, "hoist_mac": 2, "modup": 2, "moddown_auto": 2,
                                              "moddown_rescale": 2},
    "ct_mul_relin-2^16-B2": {"col_inv": 2, "ks_decompose": 1, "ks_rows": 1, "mf_tensor": 1},
    "ct_tensor-2^16-B2": {"mf_tensor": 1},
    # chunked: modup = chunks (one of 3 ciphertexts; 2 + 1; 1 + 1 + 1 from the inner product on)
    "keyswitch_hybrid-2^12-B3-RNT_KS_WS_MB=1": {"whole_fwd": 1, "whole_inv": 2, "hoist_mac": 1, "modup": 1,
                                                "moddown": 2},
    "ct_mul_relin_hybrid-2^12-B3-RNT_KS_WS_MB=1": {"elementwise": 4, "whole_fwd": 2, "whole_inv": 8,
                                                   "tensor_whole": 2, "hoist_mac": 2, "modup": 2, "moddown": 4},
    "ct_mul_relin_rescale_hybrid-2^12-B3-RNT_KS_WS_MB=1": {"whole_fwd": 2, "whole_inv": 4, "tensor_whole": 2,
                                                           "hoist_mac": 2, "modup": 2, "moddown_rescale": 4},
    "ct_dot_relin_hybrid-2^12-B3-RNT_KS_WS_MB=1": {"elementwise": 9, "copy": 36, "whole_fwd": 15, "whole_inv": 15,
                                                   "hoist_mac": 3, "modup": 3, "moddown": 6, "dot_tensor": 3},
    "ct_dot_relin_rescale_hybrid-2^12-B3-RNT_KS_WS_MB=1": {"elementwise": 3, "copy": 36, "whole_fwd": 15,
                                                           "whole_inv": 9, "hoist_mac": 3, "modup": 3,
                                                           "moddown_rescale": 6, "dot_tensor": 3},
    "ct_rotate_hybrid_hoisted-2^12-B3-RNT_KS_WS_MB=1": {"copy": 2, "whole_fwd": 3, "whole_inv": 30, "hoist_mac": 6,
                                                        "modup": 3, "moddown_auto": 30},
    "ct_linear_bsgs_hybrid-2^12-B3-RNT_KS_WS_MB=1": {"elementwise": 7, "automorphism": 12, "whole_fwd": 27,
                                                     "whole_inv": 36, "bsgs_mac": 6, "hoist_mac": 9, "modup": 9,
                                                     "moddown": 6, "moddown_auto": 12},
    "ct_linear_bsgs_hybrid_rescale-2^12-B3-RNT_KS_WS_MB=1": {"elementwise": 7, "automorphism": 12, "whole_fwd": 27,
                                                             "whole_inv": 36, "bsgs_mac": 6, "hoist_mac": 9,
                                                             "modup": 9, "moddown_auto": 12, "moddown_rescale": 6},
    # the un-fused hoisted tail: k_moddown, the automorphism launch and a strided copy
    "ct_rotate_hybrid_hoisted-2^12-B2-RNT_MODDOWN_AUTO=0": {"automorphism": 10, "copy": 12, "whole_fwd": 1,
                                                            "whole_inv": 10, "hoist_mac": 2, "modup": 1,
                                                            "moddown": 10},
    "ct_linear_bsgs_hybrid-2^12-B2-RNT_MODDOWN_AUTO=0": {"elementwise": 3, "automorphism": 8, "copy": 4,
                                                         "whole_fwd": 9, "whole_inv": 12, "bsgs_mac": 2,
                                                         "hoist_mac": 3, "modup": 3, "moddown": 6},
    # every step zero, no keys: no ModUp, only the copies
    "ct_rotate_hybrid_hoisted(zero steps)-2^12-B2": {"copy": 4},
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
