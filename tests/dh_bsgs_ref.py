"""The CPU yardstick of the double-hoisted baby-step giant-step transform on
hybrid keys (rnt_ct_linear_bsgs_hybrid_dh): literally the definition.

Notation as tests/hybrid_hoist_ref.py: C over q_0..q_{Lv-1}, E over those
followed by p_0..p_{K-1}, P = prod p_k, beta = ceil(Lv / alpha), sigma_k =
rotate_slots(., k).  diagE[j n1 + i] is the plaintext of (giant j, baby i)
reduced mod every modulus of E.  With D_d = ModUp_d(c1) over E, every product
negacyclic over E:

    b_i != 0:  T0_i = P c0 + sum_d D_d sigma_{b_i}^-1(key_b[i][d])
               T1_i =        sum_d D_d sigma_{b_i}^-1(key_a[i][d])
               Rt_i = (sigma_{b_i}(T0_i), sigma_{b_i}(T1_i))     over E, no ModDown
    b_i == 0:  Rt_i = (P c0, P c1)
    Vt_j = sum_i diagE[j n1 + i] Rt_i                            both components
    g_j != 0:  W_j = ModDown(Vt1_j)                              over C
    A0 = sum_{g_j = 0} Vt0_j + sum_{g_j != 0} (sigma_{g_j}(Vt0_j)
                                 + sum_d ModUp_d(sigma_{g_j}(W_j)) giant_key_b[j][d])
    A1 = sum_{g_j = 0} Vt1_j + sum_{g_j != 0} sum_d ModUp_d(sigma_{g_j}(W_j)) giant_key_a[j][d]
    out0 = ModDown(A0),  out1 = ModDown(A1)

P c0 is [P]_{q_j} c0 on the limb q_j and 0 on the special limbs.  There is no
special case: with every step 0 the result is ModDown(P x) = x.

Built from hybrid_ref.modup_ref / moddown_ref, hybrid_hoist_ref's
hybrid_hoisting_form_coeff / hoisted_sums, orc.mul, orc.add and
orc.rotate_slots.  tests/test_dh_bsgs_ref.py pins this file on the CPU; the GPU
tests compare the library with it word for word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc
from hybrid_hoist_ref import hoisted_sums, hybrid_hoisting_form_coeff
from hybrid_ref import _mulmod, moddown_ref, modup_ref, n_digits


def lift_times_p(moduli, Lv, x):
    """P x over E for x over C ([Lv][N]): [P]_{q_j} x_j on the limb q_j, 0 on
    the special limbs.  [Lv + K][N]."""
    P = 1
    for p in moduli[Lv:]:
        P *= int(p)
    x = np.asarray(x, dtype=np.uint64)
    out = np.zeros((len(moduli), x.shape[1]), dtype=np.uint64)
    for j in range(Lv):
        q = int(moduli[j])
        out[j] = _mulmod(x[j], P % q, q)
    return out


def plaintexts_over_e(plain, moduli):
    """Small signed plaintext polynomials (a list of integer coefficient
    vectors) reduced mod every modulus of E: [len(plain)][Lv + K][N]."""
    return np.array([[[int(v) % int(m) for v in p] for m in moduli] for p in plain], dtype=np.uint64)


def dh_bsgs_ref(Bc, Be, c0, c1, baby, giant, diagE_coeff, baby_keys, giant_keys, alpha, mul=None, pmap=map):
    """baby_keys[i], giant_keys[j]: (key_a, key_b) ORDINARY coefficient-domain
    hybrid keys ([beta][Lv + K][N]), or None for a step of 0;
    diagE_coeff[j n1 + i]: [Lv + K][N] coefficient-domain plaintexts over E.
    Returns (out0, out1), [Lv][N] each.  ``pmap``: a ``map`` over the babies,
    then over the giants, whose terms are independent (a thread pool's on the
    large rings: the oracle's calls release the interpreter lock); the sums
    over them are exact mod every modulus, so the order decides nothing."""
    Lv = Bc.L
    mod = Be.moduli
    emul = mul or (lambda u, v: orc.mul(Be, u, v))
    n1 = len(baby)
    pc0, pc1 = lift_times_p(mod, Lv, c0), lift_times_p(mod, Lv, c1)

    def acc(a, b, B):
        return b if a is None else orc.add(B, a, b)

    def baby_term(i):
        """Rt_i over E."""
        b = int(baby[i])
        if b == 0:
            return pc0, pc1
        ka, kb = baby_keys[i]
        ha = hybrid_hoisting_form_coeff(Be, ka, b)
        hb = hybrid_hoisting_form_coeff(Be, kb, b)
        s0, t1 = hoisted_sums(Be, Lv, c1, ha, hb, alpha, mul)
        t0 = orc.add(Be, pc0, s0)
        return orc.rotate_slots(Be, t0, b)[0], orc.rotate_slots(Be, t1, b)[0]

    rt = list(pmap(baby_term, range(n1)))

    def giant_term(j):
        """Giant j's share of (A0, A1) over E."""
        g = int(giant[j])
        v0 = v1 = None
        for i in range(n1):
            p = diagE_coeff[j * n1 + i]
            v0 = acc(v0, emul(rt[i][0], p), Be)
            v1 = acc(v1, emul(rt[i][1], p), Be)
        if g == 0:
            return v0, v1
        a0, a1 = orc.rotate_slots(Be, v0, g)[0], None
        x = orc.rotate_slots(Bc, moddown_ref(mod, Lv, v1), g)[0]
        ka, kb = giant_keys[j]
        for d in range(n_digits(Lv, alpha)):
            up = modup_ref(mod, Lv, alpha, d, x)
            a0 = acc(a0, emul(up, kb[d]), Be)
            a1 = acc(a1, emul(up, ka[d]), Be)
        return a0, a1

    A0 = A1 = None
    for a0, a1 in pmap(giant_term, range(len(giant))):
        A0 = acc(A0, a0, Be)
        A1 = acc(A1, a1, Be)
    return moddown_ref(mod, Lv, A0), moddown_ref(mod, Lv, A1)
