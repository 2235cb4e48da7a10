"""The plan of the homomorphic modular reduction of bootstrapping (EvalMod):
a pure host function, numpy only (DESIGN.md §4 "Fused multiply-add and
EvalMod").

After ModRaise and CoeffToSlot the real slots hold ``u = (I + eps) / K`` with an
integer ``|I| < K`` (the multiple of the first modulus the raise added) and the
small message part ``eps``.  EvalMod removes ``I``: it evaluates

    sin(2 pi K u) / (2 pi) = sin(2 pi eps) / (2 pi) ~ eps.

A sine of ``K`` periods on ``[-1, 1]`` needs a high degree, so the circuit
evaluates a cosine of ``K / 2^r`` periods and doubles the angle ``r`` times:

    g(u) = a cos(2 pi (K u - 1/4) / 2^r),   a = (2 pi)^(-1 / 2^r),
    y_0 = g(u),   y_{j+1} = 2 y_j^2 - a^(2^(j+1)).

By cos 2t = 2 cos^2 t - 1, ``y_j = a^(2^j) cos(2^j theta)`` with ``theta`` the
angle of g, so ``y_r = cos(2 pi (K u - 1/4)) / (2 pi) = sin(2 pi K u) / (2 pi)``:
the amplitude ``a`` makes the factor ``1 / (2 pi)`` come out of the squarings
and no multiplication by a constant is spent on it.

``g`` is interpolated at the Chebyshev points of ``[-1, 1]``
(``numpy.polynomial.chebyshev.chebinterpolate``) and evaluated by the fused
schedule of ``poly_eval_plan_fused`` (every Chebyshev recurrence step one
``mul_ciphertexts_hybrid_rescale_affine``); each double angle is one more such
call with w = 2, no addend and the bias ``-rint(a^(2^(j+1)) 2^logp)``.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from numpy.polynomial import chebyshev as _cheb

from .poly_eval import PolyEvalPlan, poly_eval_plan_fused

__all__ = ["EvalModPlan", "evalmod_plan"]


@dataclass
class EvalModPlan:
    K: int
    degree: int
    double_angles: int
    logp: int
    poly: PolyEvalPlan                              # the fused Chebyshev plan of g
    coeffs: list = field(default_factory=list)      # g's Chebyshev coefficients
    constants: list = field(default_factory=list)   # rint(a^(2^(j+1)) 2^logp), j < r
    fconstants: list = field(default_factory=list)  # the real numbers they stand for

    @property
    def depth(self) -> int:
        return self.poly.depth + self.double_angles

    def evaluate_float(self, u):
        """The circuit on plain numbers: the polynomial, then the double
        angles -- what the device computes up to the rounding of the integer
        weights and the scheme's noise."""
        y = self.poly.evaluate_float(u)
        for c in self.fconstants:
            y = 2.0 * y * y - c
        return y


def evalmod_plan(K: int, degree: int, double_angles: int, logp: int) -> EvalModPlan:
    K, degree, r, logp = int(K), int(degree), int(double_angles), int(logp)
    if K < 1:
        raise ValueError("evalmod_plan: K must be at least 1")
    if degree < 1:
        raise ValueError("evalmod_plan: the degree must be at least 1")
    if r < 0:
        raise ValueError("evalmod_plan: double_angles must not be negative")
    if not 1 <= logp < 62:
        raise ValueError("evalmod_plan: logp must be in [1, 62): the constants are biases of the fused call")
    a = (2.0 * np.pi) ** (-1.0 / 2 ** r)

    def g(u):
        return a * np.cos(2.0 * np.pi * (K * u - 0.25) / 2 ** r)

    coeffs = [float(c) for c in _cheb.chebinterpolate(g, degree)]
    poly = poly_eval_plan_fused(coeffs, "chebyshev", logp)
    fconst = [float(a ** (2 ** (j + 1))) for j in range(r)]
    const = [int(np.rint(c * 2.0 ** logp)) for c in fconst]
    return EvalModPlan(K, degree, r, logp, poly, coeffs, const, fconst)
