"""CPU model of rnt_ct_plain_mac / rnt_ct_plain_mac_rescale on oracle/pyoracle,
for one ciphertext of the batch: forward transform of every term, pointwise
sums against the NTT-domain plaintexts, one inverse per component, then
``rescale_pair``.

x0, x1: [n_terms][Lv][N] residues over an orc.Basis, coefficient domain (the
terms of ONE ciphertext: polys i B + b of the packed batch for i = 0..n_terms-1);
m: [n_terms][Lv][N] NTT-domain residues (the plaintexts that ciphertext meets);
bias: [Lv][N] NTT-domain residues or None.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc
from hybrid_rescale_ref import rescale_pair


def plain_mac_ref(B: orc.Basis, x0, x1, m, bias=None, rescale: bool = False):
    """(r0, r1): [Lv][N] each, or [Lv - 1][N] with ``rescale``."""
    x0, x1, m = (np.asarray(v, dtype=np.uint64) for v in (x0, x1, m))
    assert x0.shape == x1.shape == m.shape and x0.ndim == 3 and x0.shape[0] >= 1
    s0 = s1 = None
    for a0, a1, p in zip(x0, x1, m):
        t0 = orc.mul(B, orc.to_ntt(B, a0), p, ntt=True)
        t1 = orc.mul(B, orc.to_ntt(B, a1), p, ntt=True)
        s0 = t0 if s0 is None else orc.add(B, s0, t0, ntt=True)
        s1 = t1 if s1 is None else orc.add(B, s1, t1, ntt=True)
    if bias is not None:
        s0 = orc.add(B, s0, np.asarray(bias, dtype=np.uint64), ntt=True)
    r0, r1 = orc.to_coeff(B, s0), orc.to_coeff(B, s1)
    return rescale_pair(B, r0, r1) if rescale else (r0, r1)


def pick_terms(x, p, B):
    """The terms of ciphertext p of a packed batch [n_terms B][Lv][N]."""
    return np.asarray(x)[p::B]


def pick_plain(m, p, B, n_terms):
    """The plaintexts ciphertext p meets: ``m`` shared ([n_terms]) or per
    ciphertext ([n_terms B], term i of ciphertext b at i B + b)."""
    m = np.asarray(m)
    return m if m.shape[0] == n_terms else m[p::B]
