"""The CPU yardstick of the linear transform (rnt_ct_linear):

    out = sum_t diag_t * rotate_ciphertext((c0, c1), steps[t]; key_t)

composed from the oracle's own rotate_ciphertext, mul and add, exactly as a
caller of the reference engine would write it (a step of 0 is the identity,
without a key-switch).  tests/test_linear_ref.py checks it against a version
whose products are schoolbook (orc.mul_naive); the GPU tests compare the
library against it word for word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc


def linear_ref(Bo, c0, c1, steps, diag_coeff, keys, threads: int = 1, mul=None):
    """c0, c1: [L][N] coefficient-domain residues of one ciphertext;
    diag_coeff: [n_terms][L][N] coefficient-domain plaintexts; keys[t]:
    (key_a, key_b), each [L][L][N] coefficient domain (ignored, may be None,
    for a step of 0).  Returns (out0, out1), [L][N] each."""
    mul = mul or (lambda x, y: orc.mul(Bo, x, y))
    out0 = out1 = None
    for t, k in enumerate(steps):
        if int(k) == 0:
            r0, r1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
        else:
            ka, kb = keys[t]
            r0, r1 = orc.rotate_ciphertext(Bo, c0, c1, int(k), ka, kb, threads=threads)
        p0, p1 = mul(r0, diag_coeff[t]), mul(r1, diag_coeff[t])
        out0 = p0 if out0 is None else orc.add(Bo, out0, p0)
        out1 = p1 if out1 is None else orc.add(Bo, out1, p1)
    return out0, out1
