"""The CPU execution of a ``poly_eval_plan`` (rns_ntt/poly_eval.py): the same
list of operations ``CkksEngine.evaluate_polynomial_hybrid`` runs on the device,
on oracle/pyoracle, tests/hybrid_ref.py and tests/lincomb_ref.py.

    drop     the first limbs of both components
    mul      hybrid_ref.mul_relin_hybrid_ref with restrict_key of the ONE
             full-level key at the operands' level, then orc.rescale
    add      orc.add
    lincomb  lincomb_ref of the packed sources (weights and bias reduced mod
             every q_t of the level), with the plan's ``rescale``

A ciphertext is (c0, c1), [limbs][N] each; level l lives on q_0..q_{L-l-1}.
``Model`` is the CKKS instance around it (keys, encryption, decryption) that
tools/poly_eval_tolerance.py measures and the tests bound.
"""
from __future__ import annotations

import numpy as np

import encoder as enc
import pyoracle as orc
from hybrid_ref import hybrid_key_plain, mul_relin_hybrid_ref, n_digits, restrict_key
from lincomb_ref import lincomb_ref, reduce_weights


class PlanRunner:
    """Executes plans for one ring: q (ciphertext moduli), p (special moduli),
    the full-level relinearisation key (key_a, key_b: [beta][L + K][N],
    coefficient domain)."""

    def __init__(self, q, p, n, alpha, key_a, key_b):
        self.q, self.p, self.n, self.alpha = [int(v) for v in q], [int(v) for v in p], n, alpha
        self.key = (np.asarray(key_a), np.asarray(key_b))
        self._lv = {}

    def level(self, lv):
        """(Bc, Be, key_a, key_b) for ciphertexts of lv limbs."""
        if lv not in self._lv:
            L = len(self.q)
            Bc, Be = orc.Basis(self.q[:lv], self.n), orc.Basis(self.q[:lv] + self.p, self.n)
            ka, kb = (restrict_key(k, L, self.alpha, lv) for k in self.key)
            self._lv[lv] = (Bc, Be, ka, kb)
        return self._lv[lv]

    def run(self, plan, ct):
        """ct = (c0, c1) at level 0, [L][N] each; returns the plan's result."""
        L = len(self.q)
        v = {"x": (np.asarray(ct[0], dtype=np.uint64), np.asarray(ct[1], dtype=np.uint64))}
        for op in plan.ops:
            if op[0] == "drop":
                _, dst, src, level = op
                v[dst] = tuple(np.ascontiguousarray(c[:L - level]) for c in v[src])
            elif op[0] == "mul":
                _, dst, a, b = op
                Bc, Be, ka, kb = self.level(L - plan.levels[a])
                o0, o1 = mul_relin_hybrid_ref(Bc, Be, *v[a], *v[b], ka, kb, self.alpha)
                v[dst] = (orc.rescale(Bc, o0), orc.rescale(Bc, o1))
            elif op[0] == "add":
                _, dst, a, b = op
                Bc = self.level(L - plan.levels[a])[0]
                v[dst] = (orc.add(Bc, v[a][0], v[b][0]), orc.add(Bc, v[a][1], v[b][1]))
            else:
                _, dsts, srcs, weights, bias, rescale, _, _ = op
                lv = L - plan.levels[srcs[0]]
                Bc = self.level(lv)[0]
                x0 = np.stack([v[s][0] for s in srcs])
                x1 = np.stack([v[s][1] for s in srcs])
                w = reduce_weights(weights, self.q[:lv])
                bb = None if bias is None else reduce_weights(bias, self.q[:lv])
                o0, o1 = lincomb_ref(Bc, x0, x1, len(srcs), w, bb, rescale=rescale)
                for j, d in enumerate(dsts):
                    v[d] = (o0[j], o1[j])
        return v[plan.result]


class Model:
    """A CKKS instance on (q, p): ternary secret of weight N / 2, Gaussian
    errors of width 3.2, one full-level hybrid relinearisation key."""

    SIGMA = 3.2

    def __init__(self, q, p, n, alpha, logp, seed):
        self.q, self.p, self.n, self.alpha, self.logp = list(q), list(p), n, alpha, logp
        self.rng = rng = np.random.default_rng(seed)
        mod = self.q + self.p
        L = len(self.q)
        self.Bc, self.Be = orc.Basis(self.q, n), orc.Basis(mod, n)
        s = self._ternary()
        self.sk, sk_e = orc.from_coeffs(self.Bc, s), orc.from_coeffs(self.Be, s)
        self.pk_a = orc.uniform_poly(self.q, n, rng)
        self.pk_b = orc.add(self.Bc, orc.neg(self.Bc, orc.mul(self.Bc, self.pk_a, self.sk)), self._gauss(self.Bc))
        G = hybrid_key_plain(mod, L, alpha, orc.mul(self.Bc, self.sk, self.sk))
        self.key_a = orc.uniform_poly(mod, n, rng, batch=n_digits(L, alpha))
        self.key_b = np.zeros_like(self.key_a)
        for d in range(self.key_a.shape[0]):
            self.key_b[d] = orc.add(self.Be, orc.add(self.Be, orc.neg(self.Be, orc.mul(self.Be, self.key_a[d], sk_e)),
                                                     self._gauss(self.Be)), G[d])
        self.runner = PlanRunner(self.q, self.p, n, alpha, self.key_a, self.key_b)

    def _ternary(self):
        c = np.zeros(self.n, dtype=np.int64)
        idx = self.rng.choice(self.n, size=self.n // 2, replace=False)
        c[idx] = self.rng.choice(np.array([-1, 1], dtype=np.int64), size=self.n // 2)
        return c

    def _gauss(self, Bo):
        return orc.from_coeffs(Bo, np.rint(self.rng.normal(0.0, self.SIGMA, size=self.n)).astype(np.int64))

    def encrypt(self, values):
        Bc = self.Bc
        m = orc.from_coeffs(Bc, enc.encode_fft(values, self.n, self.logp))
        u = orc.from_coeffs(Bc, self._ternary())
        c0 = orc.add(Bc, orc.add(Bc, orc.mul(Bc, self.pk_b, u), self._gauss(Bc)), m)
        return c0, orc.add(Bc, orc.mul(Bc, self.pk_a, u), self._gauss(Bc))

    def decode(self, ct):
        """Decrypt and decode at the nominal scale 2^logp (the engine's integer
        bookkeeping: the drift of q != 2^logp is part of the error)."""
        lv = ct[0].shape[0]
        Bl = self.runner.level(lv)[0]
        dec = orc.add(Bl, orc.mul(Bl, ct[1], self.sk[:lv]), ct[0])
        return enc.decode_fft(orc.to_coeffs(Bl, dec), self.n, self.logp, self.n // 2)


def plain_value(coeffs, basis, x):
    """numpy's evaluation of the polynomial on the plain inputs."""
    if basis == "chebyshev":
        return np.polynomial.chebyshev.chebval(x, coeffs)
    return np.polyval(list(coeffs)[::-1], x)
