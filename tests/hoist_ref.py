"""The CPU yardstick of the hoisted rotation (rnt_ct_rotate_hoisted) and of the
baby-step giant-step transform built on it (rnt_ct_linear_bsgs_hoisted).

For one ciphertext (c0, c1), a step k, sigma = rotate_slots(., k) and the
ordinary gadget rotation key (key_a[i], key_b[i]) of that step:

    D_i  = alpha_i(c1)         channel j of D_i = channel i of c1 mod q_j
    out0 = sigma(c0) + sum_i sigma(D_i) * key_b[i]
    out1 =             sum_i sigma(D_i) * key_a[i]

literally that, from orc.rotate_slots, orc.mul and orc.add.  It is not
orc.rotate_ciphertext, whose digits are alpha_i(sigma(c1)): the words differ,
the decryption does not.  tests/test_hoist_ref.py checks it against schoolbook
products, against the regrouped form the library computes and against the
decryption; the GPU tests compare the library against it word for word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc


def digits(Bo, c1):
    """alpha_i(c1) for every i: [L][L][N], poly i channel j = c1[i] mod q_j."""
    c1 = np.asarray(c1, dtype=np.uint64)
    q = np.array(Bo.moduli, dtype=np.uint64)
    return np.stack([np.stack([c1[i] % q[j] for j in range(len(q))]) for i in range(len(q))])


def rotate_hoisted_ref(Bo, c0, c1, k, key_a, key_b, mul=None):
    """c0, c1: [L][N] coefficient-domain residues of one ciphertext; key_a,
    key_b: [L][L][N] coefficient domain (ignored for k == 0).  Returns
    (out0, out1), [L][N] each."""
    if int(k) == 0:
        return np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    mul = mul or (lambda x, y: orc.mul(Bo, x, y))
    out0, _ = orc.rotate_slots(Bo, c0, int(k))
    out1 = None
    for i, d in enumerate(digits(Bo, c1)):
        sd, _ = orc.rotate_slots(Bo, d, int(k))
        out0 = orc.add(Bo, out0, mul(sd, key_b[i]))
        p = mul(sd, key_a[i])
        out1 = p if out1 is None else orc.add(Bo, out1, p)
    return out0, out1


def bsgs_hoisted_ref(Bo, c0, c1, baby, giant, diag_coeff, baby_keys, giant_keys, threads: int = 1, mul=None):
    """tests/bsgs_ref.py's bsgs_ref with the baby rotation R_i replaced by the
    hoisted one (ordinary keys on both stages; the giant rotations are
    orc.rotate_ciphertext as there)."""
    mul = mul or (lambda x, y: orc.mul(Bo, x, y))
    n1 = len(baby)
    rot = [rotate_hoisted_ref(Bo, c0, c1, b, *(baby_keys[i] or (None, None)), mul=mul) for i, b in enumerate(baby)]
    out0 = out1 = None
    for j, g in enumerate(giant):
        v0 = v1 = None
        for i in range(n1):
            p = diag_coeff[j * n1 + i]
            p0, p1 = mul(rot[i][0], p), mul(rot[i][1], p)
            v0 = p0 if v0 is None else orc.add(Bo, v0, p0)
            v1 = p1 if v1 is None else orc.add(Bo, v1, p1)
        if int(g) == 0:
            r0, r1 = v0, v1
        else:
            r0, r1 = orc.rotate_ciphertext(Bo, v0, v1, int(g), giant_keys[j][0], giant_keys[j][1], threads=threads)
        out0 = r0 if out0 is None else orc.add(Bo, out0, r0)
        out1 = r1 if out1 is None else orc.add(Bo, out1, r1)
    return out0, out1


def rotation_exponent(k: int, n: int) -> int:
    """The exponent g of sigma_k = automorphism(., g): 5^|k| mod 2N, times
    2N - 1 for k < 0 (rotate_slots' two-automorphism composition)."""
    g = pow(5, abs(int(k)), 2 * n)
    return g * (2 * n - 1) % (2 * n) if k < 0 else g


def hoisting_form_coeff(Bo, key, k):
    """sigma_k^-1(key) in the coefficient domain, [L][L][N]: what
    rnt_key_prepare_hoisted transforms forward."""
    n = key.shape[-1]
    ginv = pow(rotation_exponent(k, n), -1, 2 * n)
    return np.stack([orc.automorphism(Bo, key[i], ginv)[0] for i in range(key.shape[0])])
