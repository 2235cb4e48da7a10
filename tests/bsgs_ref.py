"""The CPU yardstick of the baby-step giant-step linear transform
(rnt_ct_linear_bsgs):

    R_i = rotate_ciphertext((c0, c1), baby[i]; baby key i)
    V_j = sum_i P[j][i] * R_i
    out = sum_j rotate_ciphertext(V_j, giant[j]; giant key j)

composed from the oracle's own rotate_ciphertext, mul and add, exactly as a
caller of the reference engine would write it (a step of 0 is the identity,
without a key-switch).  tests/test_bsgs_ref.py checks it against a version
whose products are schoolbook (orc.mul_naive) and against tests/lt_ref.py; the
GPU tests compare the library against it word for word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc


def _rotate(Bo, c0, c1, k, key, threads):
    if int(k) == 0:
        return np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    return orc.rotate_ciphertext(Bo, c0, c1, int(k), key[0], key[1], threads=threads)


def bsgs_ref(Bo, c0, c1, baby, giant, diag_coeff, baby_keys, giant_keys, threads: int = 1, mul=None):
    """c0, c1: [L][N] coefficient-domain residues of one ciphertext;
    diag_coeff: [n2 * n1][L][N] coefficient-domain plaintexts, poly j n1 + i
    for (giant j, baby i); baby_keys[i] / giant_keys[j]: (key_a, key_b), each
    [L][L][N] coefficient domain (ignored, may be None, for a step of 0).
    Returns (out0, out1), [L][N] each."""
    mul = mul or (lambda x, y: orc.mul(Bo, x, y))
    n1 = len(baby)
    rot = [_rotate(Bo, c0, c1, b, baby_keys[i], threads) for i, b in enumerate(baby)]
    out0 = out1 = None
    for j, g in enumerate(giant):
        v0 = v1 = None
        for i in range(n1):
            p = diag_coeff[j * n1 + i]
            p0, p1 = mul(rot[i][0], p), mul(rot[i][1], p)
            v0 = p0 if v0 is None else orc.add(Bo, v0, p0)
            v1 = p1 if v1 is None else orc.add(Bo, v1, p1)
        r0, r1 = _rotate(Bo, v0, v1, g, giant_keys[j], threads)
        out0 = r0 if out0 is None else orc.add(Bo, out0, r0)
        out1 = r1 if out1 is None else orc.add(Bo, out1, r1)
    return out0, out1
