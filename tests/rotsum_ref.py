"""The CPU yardstick of the rotate-and-sum on hybrid keys (rnt_ct_rotsum_hybrid)
and of the automorphism in the NTT domain (rnt_automorphism_ntt): literally the
definitions.

Notation as tests/hybrid_ref.py and tests/hybrid_hoist_ref.py: C over
q_0..q_{Lv-1}, E over those followed by p_0..p_{K-1}, beta = ceil(Lv / alpha),
sigma_k = rotate_slots(., k).  With NZ = {t : steps[t] != 0}, z = n_steps - |NZ|,
D_d = ModUp_d(c1) over E and the ORDINARY hybrid rotation key (key_a[t][d],
key_b[t][d]) of step k_t:

    A0   = sum_{t in NZ} sum_d sigma_{k_t}(D_d) key_b[t][d]     (over E); A1 with key_a
    out0 = z c0 + sum_{t in NZ} sigma_{k_t}(c0) + ModDown(A0)
    out1 = z c1 +                                ModDown(A1)

sigma stands OUTSIDE ModUp and INSIDE ModDown.  Built from hybrid_ref.modup_ref /
moddown_ref, orc.mul, orc.add and orc.rotate_slots.  tests/test_rotsum_ref.py
pins this file on the CPU; the GPU tests compare the library with it word for
word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc
from hybrid_ref import moddown_ref, modup_ref, n_digits


def rotsum_hybrid_ref(Bc, Be, c0, c1, steps, keys, alpha, mul=None):
    """c0, c1: [Lv][N] over C; keys[t]: (key_a, key_b), ORDINARY coefficient-domain
    hybrid keys [beta][Lv + K][N] of step steps[t], or None for a step of 0.
    Returns (out0, out1), [Lv][N] each."""
    mul = mul or (lambda u, v: orc.mul(Be, u, v))
    Lv, mod = Bc.L, Be.moduli
    c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    nz = [t for t, k in enumerate(steps) if int(k) != 0]
    z = len(steps) - len(nz)
    zero = np.zeros_like(c0)
    out0, out1 = zero, zero
    for _ in range(z):
        out0, out1 = orc.add(Bc, out0, c0), orc.add(Bc, out1, c1)
    if not nz:
        return out0, out1
    D = [modup_ref(mod, Lv, alpha, d, c1) for d in range(n_digits(Lv, alpha))]
    A0 = A1 = None
    for t in nz:
        k = int(steps[t])
        key_a, key_b = keys[t]
        out0 = orc.add(Bc, out0, orc.rotate_slots(Bc, c0, k)[0])
        for d, Dd in enumerate(D):
            r = orc.rotate_slots(Be, Dd, k)[0]
            p0, p1 = mul(r, key_b[d]), mul(r, key_a[d])
            A0 = p0 if A0 is None else orc.add(Be, A0, p0)
            A1 = p1 if A1 is None else orc.add(Be, A1, p1)
    return orc.add(Bc, out0, moddown_ref(mod, Lv, A0)), orc.add(Bc, out1, moddown_ref(mod, Lv, A1))


def _brv(v, bits):
    """Bit reversal of every entry of an int64 array over `bits` bits."""
    v = np.asarray(v, dtype=np.int64)
    r = np.zeros_like(v)
    for b in range(bits):
        r |= ((v >> b) & 1) << (bits - 1 - b)
    return r


def ntt_automorphism_source(g, log_n):
    """The device-order index function of sigma_g in the NTT domain: the device
    stores device[brv(k)] = a(psi^(2k+1)), so position p of NTT(sigma_g(a)) reads
    position src[p] = brv(((g (2 brv(p) + 1) mod 2N) - 1) / 2) of NTT(a).  g odd.
    Returns src as an int64 array of length N."""
    n = 1 << log_n
    g = int(g) % (2 * n)
    assert g & 1, "sigma_g is an automorphism for odd g only"
    e = g * (2 * _brv(np.arange(n), log_n) + 1) % (2 * n)
    return _brv((e - 1) // 2, log_n)
