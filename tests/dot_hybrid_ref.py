"""The CPU yardstick of the hybrid ciphertext inner product
(rnt_ct_dot_relin_hybrid, rnt_ct_dot_relin_rescale_hybrid): literally the
definition.  For the n_terms ciphertext pairs (x0_i, x1_i), (y0_i, y1_i) over C

    d0 = sum_i x0_i y0_i    d1 = sum_i (x0_i y1_i + x1_i y0_i)    d2 = sum_i x1_i y1_i
    (acc0, acc1) = keyswitch_hybrid_ref(d2)
    out = (d0 + acc0, d1 + acc1)               and, rescaling, rescale_pair(out)

with orc.mul / orc.add over C and the key-switch of tests/hybrid_ref.py.
tests/test_dot_hybrid_ref.py pins this file on the CPU; the GPU tests compare
the library with it word for word.
"""
from __future__ import annotations

import pyoracle as orc
from hybrid_ref import keyswitch_hybrid_ref
from hybrid_rescale_ref import rescale_pair


def dot_tensor_ref(Bc, x0, x1, y0, y1):
    """x0, x1, y0, y1: [n_terms][Lv][N] residues over C.  Returns (d0, d1, d2)."""
    d0 = d1 = d2 = None
    for a0, a1, b0, b1 in zip(x0, x1, y0, y1):
        t0 = orc.mul(Bc, a0, b0)
        t1 = orc.add(Bc, orc.mul(Bc, a0, b1), orc.mul(Bc, a1, b0))
        t2 = orc.mul(Bc, a1, b1)
        d0 = t0 if d0 is None else orc.add(Bc, d0, t0)
        d1 = t1 if d1 is None else orc.add(Bc, d1, t1)
        d2 = t2 if d2 is None else orc.add(Bc, d2, t2)
    return d0, d1, d2


def dot_relin_hybrid_ref(Bc, Be, x0, x1, y0, y1, key_a, key_b, alpha):
    """(d0 + acc0, d1 + acc1) with one key-switch of the summed d2: [Lv][N] each."""
    d0, d1, d2 = dot_tensor_ref(Bc, x0, x1, y0, y1)
    a0, a1 = keyswitch_hybrid_ref(Be, Bc.L, d2, key_a, key_b, alpha)
    return orc.add(Bc, d0, a0), orc.add(Bc, d1, a1)


def dot_relin_rescale_hybrid_ref(Bc, Be, x0, x1, y0, y1, key_a, key_b, alpha):
    """dot_relin_hybrid_ref, then the rescale of either component: [Lv - 1][N]."""
    return rescale_pair(Bc, *dot_relin_hybrid_ref(Bc, Be, x0, x1, y0, y1, key_a, key_b, alpha))
