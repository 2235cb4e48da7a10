"""The CPU yardstick of hybrid key-switching (rnt_keyswitch_hybrid,
rnt_ct_rotate_hybrid, rnt_ct_mul_relin_hybrid): literally the definition.

Notation: the ciphertext basis C has moduli q_0..q_{Lv-1}; the key basis E
has m = q_0..q_{Lv-1}, p_0..p_{K-1}; P = prod p_k; digit d owns the limbs
I_d = [d alpha, min((d + 1) alpha, Lv)), Q_d their product, beta = ceil(Lv /
alpha) digits.

    ModUp_d(x):  y_i = [x_i (Q_d/q_i)^-1]_{q_i}, i in I_d
                 limb t = x_t for t in I_d, else [sum_i y_i [Q_d/q_i]_{m_t}]_{m_t}
    A0 = sum_d ModUp_d(x) key_b[d],  A1 = sum_d ModUp_d(x) key_a[d]   (over E)
    ModDown(A):  z_k = [A_{p_k} (P/p_k)^-1]_{p_k}
                 out_j = [(A_j - [sum_k z_k [P/p_k]_{q_j}]_{q_j}) [P^-1]_{q_j}]_{q_j}
    key-switch:  acc0 = ModDown(A0), acc1 = ModDown(A1)

The base conversions run on Python ints (numpy object arrays), so 61-bit
products are exact (a product of two operands below 2^32 is taken in uint64,
where it is exact too); the ring products are orc.mul on an orc.Basis of E's
moduli and the automorphisms orc.rotate_slots.  tests/test_hybrid_ref.py pins
this file on the CPU; the GPU tests compare the library with it word for word.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc


def _obj(a):
    return np.array(a, dtype=np.uint64).astype(object)


def _u64(a):
    return np.array(a, dtype=object).astype(np.uint64)


def digit_limbs(Lv: int, alpha: int, d: int) -> range:
    return range(d * alpha, min((d + 1) * alpha, Lv))


def n_digits(Lv: int, alpha: int) -> int:
    return -(-Lv // alpha)


def _mulmod(a, c, m):
    """a (an array of residues below 2^w) times the constant c < m, mod m,
    exact: in uint64 where every product fits (operands below 2^32), else on
    Python ints."""
    if a.dtype != object and int(m) < (1 << 32) and (a.size == 0 or int(a.max()) < (1 << 32)):
        return (a * np.uint64(int(c))) % np.uint64(int(m))
    return _u64((_obj(a) * int(c)) % int(m)) if a.dtype != object else (a * int(c)) % int(m)


def modup_ref(moduli, Lv, alpha, d, x):
    """x: [Lv][N] residues over C; returns ModUp_d(x), [len(moduli)][N] over E."""
    I = list(digit_limbs(Lv, alpha, d))
    Qd = 1
    for i in I:
        Qd *= int(moduli[i])
    x = np.asarray(x, dtype=np.uint64)
    y = {}
    for i in I:
        qi = int(moduli[i])
        y[i] = _mulmod(x[i], pow((Qd // qi) % qi, -1, qi), qi)
    out = np.zeros((len(moduli), x.shape[1]), dtype=np.uint64)
    for t, mt in enumerate(int(m) for m in moduli):
        if t in I:
            out[t] = x[t]
            continue
        acc = np.zeros(x.shape[1], dtype=object)
        for i in I:  # each term is below m_t < 2^63: the sum of Python ints is exact
            acc = acc + _obj(_mulmod(y[i], (Qd // int(moduli[i])) % mt, mt))
        out[t] = _u64(acc % mt)
    return out


def moddown_ref(moduli, Lv, A):
    """A: [Lv + K][N] residues over E (coefficient domain); returns [Lv][N] over C."""
    ps = [int(p) for p in moduli[Lv:]]
    P = 1
    for p in ps:
        P *= p
    A = np.asarray(A, dtype=np.uint64)
    z = [_mulmod(A[Lv + k], pow((P // p) % p, -1, p), p) for k, p in enumerate(ps)]
    out = np.zeros((Lv, A.shape[1]), dtype=np.uint64)
    for j in range(Lv):
        qj = int(moduli[j])
        conv = np.zeros(A.shape[1], dtype=object)
        for k, p in enumerate(ps):
            conv = conv + _obj(_mulmod(z[k], (P // p) % qj, qj))
        diff = _u64((_obj(A[j]) - conv) % qj)
        out[j] = _mulmod(diff, pow(P % qj, -1, qj), qj)
    return out


def keyswitch_hybrid_ref(Be, Lv, x, key_a, key_b, alpha, mul=None):
    """Be: orc.Basis over E's moduli; x: [Lv][N] over C; key_a, key_b:
    [beta][Lv + K][N] coefficient-domain residues over E.  Returns (acc0,
    acc1), [Lv][N] each."""
    mul = mul or (lambda u, v: orc.mul(Be, u, v))
    mod = Be.moduli
    A0 = A1 = None
    for d in range(n_digits(Lv, alpha)):
        up = modup_ref(mod, Lv, alpha, d, x)
        p0, p1 = mul(up, key_b[d]), mul(up, key_a[d])
        A0 = p0 if A0 is None else orc.add(Be, A0, p0)
        A1 = p1 if A1 is None else orc.add(Be, A1, p1)
    return moddown_ref(mod, Lv, A0), moddown_ref(mod, Lv, A1)


def rotate_hybrid_ref(Bc, Be, c0, c1, k, key_a, key_b, alpha):
    """(sigma_k(c0) + acc0, acc1) for x = sigma_k(c1); k == 0 is the identity
    (the key is not read).  Bc: orc.Basis over C's moduli."""
    if int(k) == 0:
        return np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    s0, _ = orc.rotate_slots(Bc, c0, int(k))
    s1, _ = orc.rotate_slots(Bc, c1, int(k))
    a0, a1 = keyswitch_hybrid_ref(Be, Bc.L, s1, key_a, key_b, alpha)
    return orc.add(Bc, s0, a0), a1


def mul_relin_hybrid_ref(Bc, Be, c0, c1, c0p, c1p, key_a, key_b, alpha):
    """The tensor d0 = c0 c0', d1 = c0 c1' + c1 c0', d2 = c1 c1' over C, then
    (d0 + acc0, d1 + acc1) for x = d2."""
    d0 = orc.mul(Bc, c0, c0p)
    d1 = orc.add(Bc, orc.mul(Bc, c0, c1p), orc.mul(Bc, c1, c0p))
    d2 = orc.mul(Bc, c1, c1p)
    a0, a1 = keyswitch_hybrid_ref(Be, Bc.L, d2, key_a, key_b, alpha)
    return orc.add(Bc, d0, a0), orc.add(Bc, d1, a1)


def hybrid_key_plain(moduli, Lv, alpha, target):
    """The plaintexts G_d of a hybrid key for the target s' (``target``: [Lv][N]
    residues of s' over C): limb t of G_d is [P s']_{q_t} for t in I_d and zero
    elsewhere, the special limbs included.  [beta][Lv + K][N]."""
    P = 1
    for p in moduli[Lv:]:
        P *= int(p)
    t = _obj(target)
    n = t.shape[1]
    G = np.zeros((n_digits(Lv, alpha), len(moduli), n), dtype=np.uint64)
    for d in range(G.shape[0]):
        for i in digit_limbs(Lv, alpha, d):
            qi = int(moduli[i])
            G[d, i] = _u64(t[i] * (P % qi) % qi)
    return G


def restrict_key(key, Lv, alpha, Lv_new):
    """The level-Lv_new key from the level-Lv one ([beta][Lv + K][N], either
    domain): the first ceil(Lv_new / alpha) polys on the limbs q_0..q_{Lv_new-1},
    p_0..p_{K-1}."""
    key = np.asarray(key)
    keep = list(range(Lv_new)) + list(range(Lv, key.shape[1]))
    return np.ascontiguousarray(key[: n_digits(Lv_new, alpha)][:, keep, :])


def lift_small(coeffs, moduli):
    """Residues of a small signed polynomial over ``moduli``: [len(moduli)][N]."""
    c = [int(v) for v in coeffs]
    return np.array([[v % int(m) for v in c] for m in moduli], dtype=np.uint64)


def crt_centered(residues, moduli):
    """The centred CRT value of every coefficient of [L][N] residues (Python ints)."""
    Q = 1
    for m in moduli:
        Q *= int(m)
    r = _obj(residues)
    acc = 0
    for i, m in enumerate(int(m) for m in moduli):
        Qi = Q // m
        acc = acc + (r[i] * pow(Qi % m, -1, m) % m) * Qi
    acc = acc % Q
    return [int(v) - Q if int(v) > Q // 2 else int(v) for v in acc]
