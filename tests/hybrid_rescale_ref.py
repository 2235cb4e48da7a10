"""The CPU yardstick of the hybrid calls that end in a rescale
(rnt_ct_mul_relin_rescale_hybrid, rnt_ct_linear_bsgs_hybrid_rescale): the
un-rescaled yardstick (tests/hybrid_ref.py, tests/hybrid_hoist_ref.py) followed
by pyoracle.rescale per component -- the definition -- and a numpy restatement
of the per-coefficient formula k_moddown_rescale evaluates, which
tests/test_hybrid_rescale_ref.py pins against that definition.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc
from hybrid_hoist_ref import bsgs_hybrid_ref
from hybrid_ref import _mulmod, _obj, _u64, mul_relin_hybrid_ref


def rescale_pair(Bc, r0, r1):
    return orc.rescale(Bc, r0), orc.rescale(Bc, r1)


def mul_relin_rescale_hybrid_ref(Bc, Be, c0, c1, c0p, c1p, key_a, key_b, alpha):
    """mul_relin_hybrid_ref, then the rescale of either component: [Lv - 1][N]."""
    return rescale_pair(Bc, *mul_relin_hybrid_ref(Bc, Be, c0, c1, c0p, c1p, key_a, key_b, alpha))


def bsgs_hybrid_rescale_ref(Bc, Be, c0, c1, baby, giant, diag, bkeys, gkeys, alpha):
    """bsgs_hybrid_ref, then the rescale of either component."""
    return rescale_pair(Bc, *bsgs_hybrid_ref(Bc, Be, c0, c1, baby, giant, diag, bkeys, gkeys, alpha))


def lift_P_times(moduli, Lv, d):
    """P d over E for d over C ([Lv][N]): limb j < Lv is [P d_j]_{q_j}, the
    special limbs are 0 (P = 0 mod p_k).  [len(moduli)][N]."""
    P = 1
    for p in moduli[Lv:]:
        P *= int(p)
    d = np.asarray(d, dtype=np.uint64)
    out = np.zeros((len(moduli), d.shape[1]), dtype=np.uint64)
    for j in range(Lv):
        qj = int(moduli[j])
        out[j] = _mulmod(d[j], P % qj, qj)
    return out


def add_over(moduli, a, b):
    """a + b limb by limb over ``moduli`` (canonical residues, exact)."""
    m = np.array([int(x) for x in moduli], dtype=object)[:, None]
    return _u64((_obj(a) + _obj(b)) % m)


def moddown_rescale_fused(moduli, Lv, A, add=None):
    """What one lane of k_moddown_rescale computes, coefficient by coefficient,
    written out from the kernel's statements rather than composed from
    moddown_ref and a rescale:

        z_k    = [A_{p_k} (P/p_k)^-1]_{p_k}
        r_j    = [(A_j - sum_k z_k [P/p_k]_{q_j}) [P^-1]_{q_j}]_{q_j} (+ add_j)   for j = Lv - 1 first
        out_j  = [(r_j - [r_last]_{q_j}) [q_last^-1]_{q_j}]_{q_j}                  for j < Lv - 1

    A: [Lv + K][N] over E, add: [Lv][N] over C or None.  Returns [Lv - 1][N]."""
    ps = [int(p) for p in moduli[Lv:]]
    qs = [int(q) for q in moduli[:Lv]]
    P = 1
    for p in ps:
        P *= p
    A = _obj(A)
    z = [(A[Lv + k] * pow((P // p) % p, -1, p)) % p for k, p in enumerate(ps)]

    def limb(j):
        q = qs[j]
        conv = 0
        for k, p in enumerate(ps):
            conv = (conv + (z[k] * ((P // p) % q)) % q) % q
        r = ((A[j] - conv) % q) * pow(P % q, -1, q) % q
        if add is not None:
            r = (r + _obj(add[j])) % q
        return r

    q_last = qs[Lv - 1]
    r_last = limb(Lv - 1)
    out = np.zeros((Lv - 1, A.shape[1]), dtype=np.uint64)
    for j in range(Lv - 1):
        q = qs[j]
        out[j] = _u64(((limb(j) - r_last % q) % q) * pow(q_last % q, -1, q) % q)
    return out
