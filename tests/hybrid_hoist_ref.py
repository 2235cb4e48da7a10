"""The CPU yardstick of the hoisted hybrid rotation
(rnt_ct_rotate_hybrid_hoisted) and of the baby-step giant-step transform on
hybrid keys (rnt_ct_linear_bsgs_hybrid): literally the definitions.

Notation as tests/hybrid_ref.py: C over q_0..q_{Lv-1}, E over those followed by
p_0..p_{K-1}, beta = ceil(Lv / alpha), sigma_k = rotate_slots(., k) -- one
automorphism by g = rotation_exponent(k, N).  With D_d = ModUp_d(c1) over E and
the ordinary hybrid rotation key (key_a[d], key_b[d]) of step k != 0:

    out0 = sigma_k(c0 + ModDown(sum_d D_d sigma_k^-1(key_b[d])))
    out1 = sigma_k(     ModDown(sum_d D_d sigma_k^-1(key_a[d])))

sigma_k stands OUTSIDE ModDown: ModDown does not commute with negation.  The
transform, with R_i the hoisted rotation by baby step b_i:

    V_j  = sum_i diag[j n1 + i] R_i                       (over C)
    A0   = sum_{j: g_j != 0} sum_d ModUp_d(sigma_{g_j}(V1_j)) giant_key_b[j][d]
    out0 = sum_{g_j = 0} V0_j + sum_{g_j != 0} sigma_{g_j}(V0_j) + ModDown(A0)
    out1 = sum_{g_j = 0} V1_j                                    + ModDown(A1)

Built from hybrid_ref.modup_ref / moddown_ref, orc.mul, orc.add,
orc.automorphism, orc.rotate_slots and hoist_ref.rotation_exponent.
tests/test_hybrid_hoist_ref.py pins this file on the CPU; the GPU tests compare
the library with it word for word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc
from hoist_ref import rotation_exponent
from hybrid_ref import moddown_ref, modup_ref, n_digits


def hybrid_hoisting_form_coeff(Be, key, k):
    """sigma_k^-1(key) in the coefficient domain over E, [beta][Lv + K][N]:
    what rnt_key_prepare_hoisted transforms forward."""
    key = np.asarray(key, dtype=np.uint64)
    n = key.shape[-1]
    ginv = pow(rotation_exponent(k, n), -1, 2 * n)
    return np.stack([orc.automorphism(Be, key[d], ginv)[0] for d in range(key.shape[0])])


def hoisted_sums(Be, Lv, c1, hkey_a, hkey_b, alpha, mul=None):
    """(A0, A1) over E for keys ALREADY in hoisting form (coefficient domain):
    A0 = sum_d ModUp_d(c1) hkey_b[d]."""
    mul = mul or (lambda u, v: orc.mul(Be, u, v))
    A0 = A1 = None
    for d in range(n_digits(Lv, alpha)):
        up = modup_ref(Be.moduli, Lv, alpha, d, c1)
        p0, p1 = mul(up, hkey_b[d]), mul(up, hkey_a[d])
        A0 = p0 if A0 is None else orc.add(Be, A0, p0)
        A1 = p1 if A1 is None else orc.add(Be, A1, p1)
    return A0, A1


def rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, k, key_a, key_b, alpha, mul=None):
    """c0, c1: [Lv][N] over C; key_a, key_b: the ORDINARY hybrid rotation key
    of step k, [beta][Lv + K][N] coefficient domain (ignored for k == 0).
    Returns (out0, out1), [Lv][N] each."""
    if int(k) == 0:
        return np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    Lv = Bc.L
    ha = hybrid_hoisting_form_coeff(Be, key_a, k)
    hb = hybrid_hoisting_form_coeff(Be, key_b, k)
    A0, A1 = hoisted_sums(Be, Lv, c1, ha, hb, alpha, mul)
    in0 = orc.add(Bc, np.asarray(c0, dtype=np.uint64), moddown_ref(Be.moduli, Lv, A0))
    in1 = moddown_ref(Be.moduli, Lv, A1)
    return orc.rotate_slots(Bc, in0, int(k))[0], orc.rotate_slots(Bc, in1, int(k))[0]


def bsgs_hybrid_ref(Bc, Be, c0, c1, baby, giant, diag_coeff, baby_keys, giant_keys, alpha, mul=None):
    """baby_keys[i], giant_keys[j]: (key_a, key_b) ORDINARY coefficient-domain
    hybrid keys, or None for a step of 0; diag_coeff[j n1 + i]: [Lv][N]
    coefficient-domain plaintexts over C.  Returns (out0, out1)."""
    Lv = Bc.L
    mod = Be.moduli
    cmul = lambda u, v: orc.mul(Bc, u, v)  # noqa: E731
    emul = mul or (lambda u, v: orc.mul(Be, u, v))
    n1 = len(baby)
    rot = [rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, b, *(baby_keys[i] or (None, None)), alpha, mul=mul)
           for i, b in enumerate(baby)]
    s0 = s1 = A0 = A1 = None

    def acc(a, b, B):
        return b if a is None else orc.add(B, a, b)

    for j, g in enumerate(giant):
        v0 = v1 = None
        for i in range(n1):
            p = diag_coeff[j * n1 + i]
            v0 = acc(v0, cmul(rot[i][0], p), Bc)
            v1 = acc(v1, cmul(rot[i][1], p), Bc)
        if int(g) == 0:
            s0, s1 = acc(s0, v0, Bc), acc(s1, v1, Bc)
            continue
        s0 = acc(s0, orc.rotate_slots(Bc, v0, int(g))[0], Bc)
        x = orc.rotate_slots(Bc, v1, int(g))[0]
        ka, kb = giant_keys[j]
        for d in range(n_digits(Lv, alpha)):
            up = modup_ref(mod, Lv, alpha, d, x)
            A0 = acc(A0, emul(up, kb[d]), Be)
            A1 = acc(A1, emul(up, ka[d]), Be)
    if A0 is None:
        return s0, s1
    out0 = orc.add(Bc, s0, moddown_ref(mod, Lv, A0))
    m1 = moddown_ref(mod, Lv, A1)
    return out0, (m1 if s1 is None else orc.add(Bc, s1, m1))
