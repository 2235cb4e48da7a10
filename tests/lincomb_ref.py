"""The CPU yardstick of rnt_ct_lincomb / rnt_ct_lincomb_rescale: literally the
definition in include/rnsntt.h.

x0, x1: [n_in B][Lv][N] residues over an orc.Basis (term i of ciphertext b at
poly i B + b); weights: [n_out][n_in][Lv] residues; bias: [n_out][Lv] residues
or None.  For output j, ciphertext b, limb t:

    r0 = sum_i w[j][i][t] x0_i + bias[j][t] X^0      r1 = sum_i w[j][i][t] x1_i

mod q_t, canonical ([n_out B][Lv][N], output j of ciphertext b at poly j B + b),
and with ``rescale`` orc.rescale of every poly ([n_out B][Lv - 1][N]).  Products
of operands below 2^32 are taken in uint64, where they are exact; wider ones on
Python ints.  tests/test_lincomb_ref.py pins this file against a big-int
computation; the GPU tests compare the library with it word for word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc


def reduce_weights(ints, moduli):
    """Signed Python ints of any shape -> residues with a trailing limb axis."""
    a = np.array(ints, dtype=object)
    return np.stack([np.array(a % int(q), dtype=np.uint64) for q in moduli], axis=-1)


def _weighted_sum(xt, wt, q):
    """xt: [n_in][...] residues mod q; wt: [n_in] residues; sum_i wt[i] xt[i] mod q."""
    if q < (1 << 32):
        acc = np.zeros(xt.shape[1:], dtype=np.uint64)
        for i in range(xt.shape[0]):
            acc = (acc + xt[i] * np.uint64(int(wt[i])) % np.uint64(q)) % np.uint64(q)
        return acc
    acc = np.zeros(xt.shape[1:], dtype=object)
    for i in range(xt.shape[0]):
        acc = acc + xt[i].astype(object) * int(wt[i])
    return np.array(acc % q, dtype=np.uint64)


def lincomb_ref(Bo, x0, x1, n_in, weights, bias=None, rescale=False):
    x = [np.asarray(x0, dtype=np.uint64), np.asarray(x1, dtype=np.uint64)]
    w = np.asarray(weights, dtype=np.uint64)
    n_out, Lv, n = w.shape[0], Bo.L, x[0].shape[2]
    assert w.shape == (n_out, n_in, Lv) and x[0].shape[1] == Lv and x[0].shape[0] % n_in == 0
    B = x[0].shape[0] // n_in
    out = [np.zeros((n_out * B, Lv, n), dtype=np.uint64) for _ in range(2)]
    for comp in range(2):
        for t, q in enumerate(int(m) for m in Bo.moduli):
            xt = x[comp][:, t, :].reshape(n_in, B, n)
            for j in range(n_out):
                r = _weighted_sum(xt, w[j, :, t], q)
                if comp == 0 and bias is not None:
                    r[:, 0] = (r[:, 0].astype(object) + int(bias[j][t])) % q
                out[comp][j * B:(j + 1) * B, t, :] = r
    if rescale:
        out = [np.stack([orc.rescale(Bo, p) for p in o]) for o in out]
    return out[0], out[1]
