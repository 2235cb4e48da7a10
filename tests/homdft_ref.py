"""The CPU model of ModRaise, the monomial product and the staged
coefficient/slot transforms (rnt_mod_raise, rnt_mul_monomial,
CkksEngine.coeff_to_slot_hybrid / slot_to_coeff_hybrid).

    mod_raise_ref         the centred CRT value in Python integers, then % q_j
    mod_raise_garner_ref  the same through the mixed-radix digits the kernel forms
    mul_monomial_ref      the negacyclic shift, written as the definition
    HomDftModel           a CKKS instance (keys for a plan's steps, encryption,
                          decryption) whose transforms are a composition of
                          hybrid_rescale_ref.bsgs_hybrid_rescale_ref, one call per
                          group, on diagonals encoded by oracle/encoder.py

A ciphertext is (c0, c1), [limbs][N] each.
"""
from __future__ import annotations

import numpy as np

import encoder as enc
import pyoracle as orc
from hybrid_ref import _obj, _u64, crt_centered, hybrid_key_plain, n_digits, restrict_key
from hybrid_rescale_ref import bsgs_hybrid_rescale_ref


def mod_raise_ref(x, moduli_in, moduli_out):
    """x: [l0][N] residues over moduli_in; returns [len(moduli_out)][N]: the
    centred CRT value of every coefficient (in (-Q0/2, Q0/2]) mod each q_j."""
    v = np.array(crt_centered(x, moduli_in), dtype=object)
    return _u64(np.stack([v % int(q) for q in moduli_out]))


def mod_raise_garner_ref(x, moduli_in, moduli_out):
    """The kernel's formulation on Python integers: the mixed-radix digits
    d_0 = x_0, d_i = (x_i - (d_0 + q_0 d_1 + ...)) (q_0 .. q_{i-1})^-1 mod q_i,
    the comparison with the digits of floor(Q0 / 2) from the top, and limb j =
    sum_i d_i (q_0 .. q_{i-1} mod q_j) - [x > floor(Q0/2)] (Q0 mod q_j)."""
    q = [int(v) for v in moduli_in]
    x = _obj(x)
    n = x.shape[1]
    d, rad = [], [1]
    for i in range(len(q)):
        s = sum((d[k] * (rad[k] % q[i]) for k in range(i)), np.zeros(n, dtype=object))
        d.append(((x[i] - s) * pow(rad[i] % q[i], -1, q[i])) % q[i] if i else x[0])
        rad.append(rad[i] * q[i])
    Q0 = rad[-1]
    half, hd = Q0 // 2, []
    for qi in q:
        hd.append(half % qi)
        half //= qi
    gt = np.zeros(n, dtype=bool)
    eq = np.ones(n, dtype=bool)
    for i in range(len(q) - 1, -1, -1):
        gt |= eq & np.array([int(v) > hd[i] for v in d[i]])
        eq &= np.array([int(v) == hd[i] for v in d[i]])
    neg = np.array([1 if g else 0 for g in gt], dtype=object)
    out = []
    for qj in (int(v) for v in moduli_out):
        acc = sum(((d[i] * (rad[i] % qj)) % qj for i in range(len(q))), np.zeros(n, dtype=object))
        out.append((acc - neg * (Q0 % qj)) % qj)
    return _u64(np.stack(out))


def mul_monomial_ref(x, moduli, k):
    """x: [..., L, N] residues; x * X^k in Z_q[X]/(X^N + 1), k mod 2N:
    coefficient j lands at (j + k) mod N, negated when floor((j + k) / N) is odd."""
    x = np.asarray(x, dtype=np.uint64)
    n = x.shape[-1]
    k = int(k) % (2 * n)
    q = np.array([int(m) for m in moduli], dtype=np.uint64)[:, None]
    out = np.zeros_like(x)
    j = np.arange(n)
    dst = (j + k) % n
    odd = ((j + k) // n) % 2 == 1
    negated = np.where(x == 0, np.uint64(0), q - x)
    out[..., dst] = np.where(odd, negated, x)
    return out


def decrypt_centered(q, n, sk_coeffs, ct):
    """The centred CRT of c0 + c1 s over the ciphertext's limbs: Python ints [N]."""
    lv = ct[0].shape[0]
    Bl = orc.Basis(q[:lv], n)
    s = orc.from_coeffs(Bl, sk_coeffs)
    return crt_centered(orc.add(Bl, orc.mul(Bl, ct[1], s), ct[0]), q[:lv])


class HomDftModel:
    """A CKKS instance on (q, p) with a ternary secret of Hamming weight
    ``hamming_weight`` and Gaussian errors of width 3.2, holding ONE full-level
    ordinary hybrid rotation key per step it is asked for (``key``)."""

    SIGMA = 3.2

    def __init__(self, q, p, n, alpha, hamming_weight, seed):
        self.q, self.p, self.n, self.alpha, self.h = [int(v) for v in q], [int(v) for v in p], n, alpha, hamming_weight
        self.rng = np.random.default_rng(seed)
        self.mod = self.q + self.p
        self.Bc, self.Be = orc.Basis(self.q, n), orc.Basis(self.mod, n)
        s = np.zeros(n, dtype=np.int64)
        idx = self.rng.choice(n, size=hamming_weight, replace=False)
        s[idx] = self.rng.choice(np.array([-1, 1], dtype=np.int64), size=hamming_weight)
        self.s = s
        self.sk, self.sk_e = orc.from_coeffs(self.Bc, s), orc.from_coeffs(self.Be, s)
        self.keys = {}
        self._lv = {}

    def _gauss(self, Bo):
        return orc.from_coeffs(Bo, np.rint(self.rng.normal(0.0, self.SIGMA, size=self.n)).astype(np.int64))

    def key(self, step):
        """(key_a, key_b), [beta][L + K][N] coefficient domain: the ordinary
        full-level hybrid rotation key of ``step`` (made once)."""
        step = int(step)
        if step not in self.keys:
            L = len(self.q)
            G = hybrid_key_plain(self.mod, L, self.alpha, orc.rotate_slots(self.Bc, self.sk, step)[0])
            a = orc.uniform_poly(self.mod, self.n, self.rng, batch=n_digits(L, self.alpha))
            b = np.zeros_like(a)
            for d in range(a.shape[0]):
                b[d] = orc.add(self.Be, orc.add(self.Be, orc.neg(self.Be, orc.mul(self.Be, a[d], self.sk_e)),
                                                self._gauss(self.Be)), G[d])
            self.keys[step] = (a, b)
        return self.keys[step]

    def level(self, lv):
        if lv not in self._lv:
            self._lv[lv] = (orc.Basis(self.q[:lv], self.n), orc.Basis(self.q[:lv] + self.p, self.n))
        return self._lv[lv]

    def encrypt(self, coeffs, lv):
        """A symmetric encryption of the integer polynomial ``coeffs`` on the
        first ``lv`` limbs: (m + e - a s, a)."""
        Bl = self.level(lv)[0]
        a = orc.uniform_poly(self.q[:lv], self.n, self.rng)
        s = orc.from_coeffs(Bl, self.s)
        c0 = orc.add(Bl, orc.add(Bl, orc.neg(Bl, orc.mul(Bl, a, s)), self._gauss(Bl)), orc.from_coeffs(Bl, coeffs))
        return c0, a

    def decrypt(self, ct):
        return decrypt_centered(self.q, self.n, self.s, ct)

    def decode(self, ct, logp):
        return enc.decode_fft(np.array(self.decrypt(ct), dtype=np.int64), self.n, logp, self.n // 2)

    def mod_raise(self, ct, L):
        lv = ct[0].shape[0]
        return tuple(mod_raise_ref(c, self.q[:lv], self.q[:L]) for c in ct)

    def encode_group(self, group, lv):
        """The plaintexts of one group of a homdft plan at ``lv`` limbs,
        [n2 n1][lv][N] coefficient domain: row (j, i) is diagonal g_j + b_i
        rotated back by g_j, times q_{lv-1} / 2^bits and encoded at bits = the
        bit length of q_{lv-1} -- at the scale q_{lv-1} exactly, the prime the
        group's rescale divides by (CkksEngine.prepare_homdft's rule)."""
        slots = self.n // 2
        bits = self.q[lv - 1].bit_length()
        drift = self.q[lv - 1] / 2.0 ** bits
        Bl = self.level(lv)[0]
        out = []
        for g in group.giant_steps:
            for b in group.baby_steps:
                d = group.diags.get((g + b) % slots)
                row = np.zeros(slots, dtype=np.complex128) if d is None else np.roll(d, g) * drift
                out.append(orc.from_coeffs(Bl, enc.encode_fft(row, self.n, bits)))
        return np.stack(out)

    def transform(self, plan, ct, plaintexts=None):
        """The plan's groups in order, one bsgs_hybrid_rescale_ref each, with
        the full-level keys restricted to the group's level; ``depth`` levels
        down.  ``plaintexts[s]`` ([n2 n1][lv][N], coefficient domain) replaces
        ``encode_group`` for group s: the device encoder may round a tie the
        other way, so a word-for-word comparison hands over the device's."""
        L = len(self.q)
        for gi, group in enumerate(plan.groups):
            lv = ct[0].shape[0]
            Bc, Be = self.level(lv)

            def keys(steps):
                return [None if s == 0 else tuple(restrict_key(k, L, self.alpha, lv) for k in self.key(s))
                        for s in steps]

            ct = bsgs_hybrid_rescale_ref(Bc, Be, ct[0], ct[1], group.baby_steps, group.giant_steps,
                                         self.encode_group(group, lv) if plaintexts is None else plaintexts[gi],
                                         keys(group.baby_steps),
                                         keys(group.giant_steps), self.alpha)
        return ct


def packed_slots(a, n):
    """w_j = a_j + i a_{j+n/2} for a polynomial ``a`` of N = n integer coefficients."""
    a = np.array([float(v) for v in a])
    return a[: n // 2] + 1j * a[n // 2:]


def bit_reversed(v):
    """v[R[s]] for the bit reversal R of the index."""
    n = len(v)
    bits = n.bit_length() - 1
    r = [int(format(i, f"0{bits}b")[::-1], 2) if bits else 0 for i in range(n)]
    return np.asarray(v)[r]


def run_pipeline(model, c2s, s2c, values, logp):
    """raise -> CoeffToSlot -> SlotToCoeff on the model: ``values`` (N/2
    complex slots) are encoded at 2^logp and encrypted on ONE limb, raised onto
    all of the model's limbs and sent through the two plans (``s2c`` None: the
    slot side only).  With ``a`` the centred CRT of the raised ciphertext's
    decryption, returns a dict:

        raised, slot, back   the three ciphertexts
        a                    Python ints [N]
        slot_err             max |decode(slot) - order(a_j + i a_{j+n}) / 2^logp|
                             (bit-reversed for order="bitrev")
        back_err             max |decode(centred((t - a) mod q_0))|, t the
                             decryption of ``back`` (one limb): the round trip
                             against ``a`` itself, as a decode error at 2^logp
    """
    n = model.n
    ct1 = model.encrypt(enc.encode_fft(values, n, logp), 1)
    raised = model.mod_raise(ct1, len(model.q))
    a = model.decrypt(raised)
    slot = model.transform(c2s, raised)
    want = packed_slots(a, n)
    if c2s.order == "bitrev":
        want = bit_reversed(want)
    out = {"first": ct1, "raised": raised, "slot": slot, "a": a,
           "slot_err": float(np.max(np.abs(model.decode(slot, logp) - want / 2.0 ** logp)))}
    if s2c is not None:
        back = model.transform(s2c, slot)
        out["back"] = back
        out["back_err"] = back_error(model, back, a, logp)
    return out


def back_error(model, back, a, logp):
    q0 = model.q[0]
    t = model.decrypt(back)
    diff = [((int(u) - int(v) + q0 // 2) % q0) - q0 // 2 for u, v in zip(t, a)]
    return float(np.max(np.abs(enc.decode_fft(np.array(diff, dtype=np.int64), model.n, logp, model.n // 2))))
