"""The plan of the homomorphic CoeffToSlot / SlotToCoeff transforms (pure
host, numpy only; DESIGN.md §4 "ModRaise and the coefficient/slot transforms").

Notation: ``n = N / 2`` slots, ``zeta = exp(i pi / N)``, ``U[k][j] =
zeta^(5^k j)`` for ``k, j < n``.  The encoder's slot vector of a polynomial
``a`` is ``z = U w`` with ``w_j = a_j + i a_{j+n}``, and ``U^-1 = U^H / n``.

``U = S_m ... S_1 R`` with ``m = log2 n``, ``R`` the bit-reversal permutation
and ``S_t`` the radix-2 butterfly stage of span ``len = 2^t``: ``(u, v) ->
(u + tau v, u - tau v)`` on positions ``(i + j, i + j + len/2)``, ``tau =
zeta^((5^j mod 4 len) (2N / (4 len)))``.  ``S_t`` has the cyclic diagonals
``{0, +len/2, -len/2}`` only, and ``S_t^-1 = S_t^H / 2``.

A matrix is kept as a dict from step ``k`` in ``[0, n)`` to its diagonal
``d_k[s] = M[s][(s + k) mod n]``; products are diagonal convolutions

    (A B)_k[s] = sum_{a + b = k} A_a[s] B_b[(s + a) mod n],

so nothing here is ever an n x n matrix (except ``order="natural"``, which is
for small rings).

A plan says nothing about the basis its diagonals are encoded on: the engine
encodes them over the level's ``Q_l`` (``CkksEngine.prepare_homdft``, one
``linear_transform_bsgs_hybrid_rescale`` per group) or over ``Q_l u P``
(``prepare_homdft_dh``, one double-hoisted call per group) with the same key
sets.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

__all__ = ["HomDftGroup", "HomDftPlan", "homdft_plan", "diag_product", "diag_adjoint", "stage_diagonals",
           "bit_reverse_permutation"]


def bit_reverse_permutation(n: int) -> np.ndarray:
    """``r[i]`` = the ``log2 n``-bit reversal of i."""
    bits = n.bit_length() - 1
    r = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


def stage_diagonals(degree: int, t: int) -> dict:
    """The diagonals of ``S_t`` (span ``len = 2^t``) for ring degree N."""
    n = degree // 2
    ln = 1 << t
    h = ln // 2
    j = np.arange(n) % ln  # position inside the butterfly block
    jj = j % h
    # 5^jj mod 4 len, by repeated multiplication over the h distinct values
    pw = np.ones(h, dtype=np.int64)
    for x in range(1, h):
        pw[x] = pw[x - 1] * 5 % (4 * ln)
    tau = np.exp(2j * np.pi * pw[jj] / (4 * ln))  # zeta^(e 2N / (4 len)) = exp(2 pi i e / (4 len))
    upper = j < h
    d0 = np.where(upper, 1.0 + 0j, -tau)
    dp = np.where(upper, tau, 0j)   # row s (upper) reads s + len/2
    dm = np.where(upper, 0j, 1.0 + 0j)  # row s (lower) reads s - len/2
    out = {0: d0}
    if h % n == (-h) % n:  # the top stage: +n/2 and -n/2 are one diagonal
        out[h % n] = dp + dm
    else:
        out[h % n] = dp
        out[(-h) % n] = dm
    return out


def diag_product(A: dict, B: dict, n: int) -> dict:
    """The diagonals of the matrix product A B; all-zero diagonals are dropped."""
    out = {}
    for a, da in A.items():
        for b, db in B.items():
            k = (a + b) % n
            term = da * np.roll(db, -a)
            out[k] = out[k] + term if k in out else term
    return {k: v for k, v in out.items() if np.any(v != 0)}


def diag_adjoint(A: dict, n: int) -> dict:
    """The diagonals of A^H: ``d^H_k[s] = conj(d_{-k}[(s + k) mod n])``."""
    return {(-k) % n: np.conj(np.roll(v, k)) for k, v in A.items()}


def _scale(A: dict, c) -> dict:
    return {k: v * c for k, v in A.items()}


@dataclass
class HomDftGroup:
    """One linear_transform_bsgs call: the matrix of ``stages`` (the S_t it
    multiplies, in application order) as ``diags``; ``stride`` is the smallest
    half-span, which every diagonal index is a multiple of; the BSGS grid
    ``giant_steps x baby_steps`` names every nonzero diagonal once."""

    stages: list
    diags: dict
    stride: int
    baby_steps: list
    giant_steps: list

    def n_keyswitches(self) -> int:
        return sum(1 for b in self.baby_steps if b) + sum(1 for g in self.giant_steps if g)


@dataclass
class HomDftPlan:
    degree: int
    direction: str
    depth: int
    order: str
    constant: complex
    groups: list = field(default_factory=list)

    @property
    def slots(self) -> int:
        return self.degree // 2

    def rotation_steps(self) -> list:
        """Per group ``(baby, giant)``: the nonzero steps, which need keys."""
        return [([b for b in g.baby_steps if b], [s for s in g.giant_steps if s]) for g in self.groups]

    def n_keyswitches(self) -> int:
        return sum(g.n_keyswitches() for g in self.groups)

    def apply(self, v):
        """The plan applied to a slot vector (or [..., n] stack) in float64:
        the groups in order, each as ``sum_k d_k * roll(v, -k)``."""
        v = np.asarray(v, dtype=np.complex128)
        for g in self.groups:
            v = sum(d * np.roll(v, -k, axis=-1) for k, d in g.diags.items())
        return v


def _grid(stride: int, lo: int, hi: int, n: int):
    """A BSGS grid over the diagonals ``stride * e``, ``lo <= e <= hi`` (mod n):
    babies ``stride * [0, n1)``, giants ``stride * n1 * j``; when the range
    wraps the ``n / stride`` multiples of the stride, the grid is all of them."""
    per = n // stride  # the multiples of the stride mod n
    count = min(hi - lo + 1, per)
    n1 = 1
    while n1 * n1 < count:
        n1 *= 2
    n1 = min(n1, per)
    baby = [stride * i for i in range(n1)]
    if hi - lo + 1 >= per or (hi // n1 - lo // n1 + 1) * n1 > per:
        giant = [stride * n1 * j for j in range(per // n1)]
    else:
        giant = [(stride * n1 * j) % n for j in range(lo // n1, hi // n1 + 1)]
    return baby, giant


def homdft_plan(degree: int, direction: str, depth: int, order: str = "bitrev", constant=1.0) -> HomDftPlan:
    """The staged transform for ring degree ``degree``.

    ``direction="slot_to_coeff"`` is ``w -> z = U w``: a ciphertext whose slots
    hold ``a_j + i a_{j+n}`` becomes one that encodes the polynomial ``a``;
    ``"coeff_to_slot"`` is the inverse ``z -> w = U^-1 z``.  With
    ``order="bitrev"`` R is left out: CoeffToSlot is ``S_1^-1 ... S_m^-1`` with
    its output in bit-reversed slot order, SlotToCoeff ``S_m ... S_1`` on input
    in that order.  ``order="natural"`` (``depth = 1`` only) folds R into one
    dense matrix.  The m stages are split into ``depth`` contiguous groups of
    sizes differing by at most one, ``groups[0]`` the first applied;
    ``constant`` (real or complex) enters as ``constant^(1/depth)`` in each."""
    n = degree // 2
    if degree < 4 or degree & (degree - 1):
        raise ValueError("homdft_plan: the degree must be a power of two, at least 4")
    m = n.bit_length() - 1
    if direction not in ("slot_to_coeff", "coeff_to_slot"):
        raise ValueError("homdft_plan: direction is 'slot_to_coeff' or 'coeff_to_slot'")
    if order not in ("bitrev", "natural"):
        raise ValueError("homdft_plan: order is 'bitrev' or 'natural'")
    depth = int(depth)
    if not 1 <= depth <= m:
        raise ValueError(f"homdft_plan: depth must be in [1, {m}]")
    if order == "natural" and depth != 1:
        raise ValueError("homdft_plan: order='natural' folds the bit reversal into ONE dense matrix (depth = 1)")
    c = complex(constant) ** (1.0 / depth)
    plan = HomDftPlan(degree, direction, depth, order, complex(constant))
    if order == "natural":
        k = np.arange(n)
        e = np.ones(n, dtype=np.int64)
        for x in range(1, n):
            e[x] = e[x - 1] * 5 % (2 * degree)
        U = np.exp(1j * np.pi * ((e[:, None] * k[None, :]) % (2 * degree)) / degree)
        M = (U if direction == "slot_to_coeff" else U.conj().T / n) * c
        s = np.arange(n)
        diags = {d: M[s, (s + d) % n] for d in range(n)}
        baby, giant = _grid(1, 0, n - 1, n)
        plan.groups.append(HomDftGroup(list(range(1, m + 1)), diags, 1, baby, giant))
        return plan
    sizes = [m // depth + (1 if g < m % depth else 0) for g in range(depth)]
    # the stages in application order: S_1 first for SlotToCoeff, S_m^-1 first for CoeffToSlot
    order_t = list(range(1, m + 1)) if direction == "slot_to_coeff" else list(range(m, 0, -1))
    at = 0
    for g in sizes:
        ts = order_t[at:at + g]
        at += g
        acc = None
        for t in ts:
            S = stage_diagonals(degree, t)
            if direction == "coeff_to_slot":
                S = _scale(diag_adjoint(S, n), 0.5)
            acc = S if acc is None else diag_product(S, acc, n)  # a later stage multiplies from the left
        acc = _scale(acc, c)
        stride = 1 << (min(ts) - 1)
        span = sum(1 << (t - 1) for t in ts) // stride  # the diagonals are stride * e, |e| <= span
        baby, giant = _grid(stride, -span, span, n)
        plan.groups.append(HomDftGroup(ts, acc, stride, baby, giant))
    return plan
