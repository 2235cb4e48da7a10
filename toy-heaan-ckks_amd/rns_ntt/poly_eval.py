"""The schedule of a ciphertext polynomial evaluation (Paterson-Stockmeyer), as
a list of operations: a pure host function, no device access.

``poly_eval_plan(coeffs, basis, logp)`` turns the coefficients ``c_0..c_d`` of
``p = sum_k c_k Phi_k`` (``Phi_k = x^k`` in the monomial basis, ``T_k`` in the
Chebyshev one) into the exact operations ``CkksEngine.evaluate_polynomial_hybrid``
runs on the device; a CPU model that executes the same list reproduces its
words.  Every value has a name and a level (the ciphertext primes consumed);
an operand is never used above the level the plan states.

    ("drop", dst, src, level)       mod_drop_last of src down to ``level``
    ("mul", dst, a, b)              mul_ciphertexts_hybrid_rescale: level + 1
    ("add", dst, a, b)              add_ciphertexts
    ("lincomb", dsts, srcs, weights, bias, rescale, fweights, fbias)
                                    ct_lincomb of the packed srcs: dsts[j] =
                                    sum_i weights[j][i] srcs[i] + bias[j]; with
                                    ``rescale`` level + 1.  fweights / fbias:
                                    the real numbers the integers stand for.
    ("fma", dst, a, b, w, z, u, bias, fbias)   (poly_eval_plan_fused alone)
                                    mul_ciphertexts_hybrid_rescale_affine:
                                    dst = w a b + u z + bias at level + 1, z
                                    (or None) at that level already; fbias the
                                    real number the integer bias stands for.

The schedule.  m = max(2, 2^ceil(log2(d + 1) / 2)) babies Phi_1..Phi_{m-1}, the
giants g_k = m 2^k <= d.  Phi_n = Phi_a Phi_b with a the largest power of two
below n (n / 2 for a power of two) and b = n - a; in the Chebyshev basis
T_n = 2 T_a T_b - T_{a-b} (T_{2a} = 2 T_a^2 - 1) through an un-rescaled
ct_lincomb.  eval(P) of degree e >= m: (Q, R) = divmod(P, Phi_g), g the largest
giant <= e, eval(P) = eval(Q) Phi_g + eval(R); every P of degree < m is a leaf,
and all leaves come from ONE rescaling ct_lincomb of the babies (chunks of 16
outputs): weight k >= 1 is rint(c_k 2^logp), the bias rint(c_0 2^(2 logp)).
The depth is at most ceil(log2(d + 1)) + 1 levels.

``poly_eval_plan_fused(coeffs, basis, logp)`` (the same arguments; a function of
its own, so that ``poly_eval_plan`` is what it was, signature included)
keeps the schedule, its levels and its leaves and folds every
affine step that follows a product into the product's own call: a Chebyshev
power is ONE fma (w = 2, z = T_{a-b} at the output level, u = -1; for T_{2a}
w = 2 and the bias -2^logp), so no un-rescaled ct_lincomb is left, and a node
eval(Q) Phi_g + eval(R) is one fma with z = eval(R) dropped to the product's
level.  Where eval(R) sits deeper than the product the node keeps mul, drop,
add.  The default plan is today's, op for op.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
from numpy.polynomial import chebyshev as _cheb

MAX_TERMS = 16  # rnt_ct_lincomb's n_in / n_out limit


@dataclass
class PolyEvalPlan:
    basis: str
    logp: int
    degree: int
    m: int
    giants: list
    ops: list = field(default_factory=list)
    levels: dict = field(default_factory=dict)  # name -> level
    result: str = ""

    @property
    def depth(self) -> int:
        return self.levels[self.result]

    @property
    def n_leaves(self) -> int:
        return sum(len(op[1]) for op in self.ops if op[0] == "lincomb" and op[5])

    def evaluate_float(self, x):
        """The plan on plain numbers: what the circuit computes up to the
        rounding of the weights and the scheme's noise."""
        v = {"x": np.asarray(x, dtype=np.float64)}
        for op in self.ops:
            if op[0] == "drop":
                v[op[1]] = v[op[2]]
            elif op[0] == "mul":
                v[op[1]] = v[op[2]] * v[op[3]]
            elif op[0] == "add":
                v[op[1]] = v[op[2]] + v[op[3]]
            elif op[0] == "fma":
                _, dst, a, b, w, z, u, _, fbias = op
                v[dst] = w * (v[a] * v[b]) + (u * v[z] if z is not None else 0.0) + fbias
            else:
                _, dsts, srcs, _, _, _, fw, fb = op
                for j, d in enumerate(dsts):
                    acc = np.zeros_like(v["x"]) + (fb[j] if fb is not None else 0.0)
                    for i, s in enumerate(srcs):
                        acc = acc + fw[j][i] * v[s]
                    v[d] = acc
        return v[self.result]


def _trim(c):
    c = [float(v) for v in c]
    while len(c) > 1 and c[-1] == 0.0:
        c.pop()
    return c


def poly_eval_plan(coeffs, basis: str, logp: int) -> PolyEvalPlan:
    return _build_plan(coeffs, basis, logp, fused=False)


def poly_eval_plan_fused(coeffs, basis: str, logp: int) -> PolyEvalPlan:
    """The same schedule with every affine step that follows a product folded
    into the product's call (the module docstring's ``fma`` op)."""
    return _build_plan(coeffs, basis, logp, fused=True)


def _build_plan(coeffs, basis: str, logp: int, fused: bool) -> PolyEvalPlan:
    if basis not in ("monomial", "chebyshev"):
        raise ValueError(f"poly_eval_plan: unknown basis {basis!r} (monomial or chebyshev)")
    cheb = basis == "chebyshev"
    logp = int(logp)
    if logp < 1:
        raise ValueError("poly_eval_plan: logp must be at least 1")
    P = _trim(coeffs)
    d = len(P) - 1
    if d < 1:
        raise ValueError("poly_eval_plan: the polynomial must have degree at least 1")
    m = max(2, 1 << -(-(int(d).bit_length()) // 2))  # bit_length(d) = ceil(log2(d + 1))
    if m - 1 > MAX_TERMS:
        raise ValueError(f"poly_eval_plan: degree {d} needs {m - 1} baby powers, above ct_lincomb's {MAX_TERMS}")
    giants = []
    g = m
    while g <= d:
        giants.append(g)
        g *= 2
    plan = PolyEvalPlan(basis, logp, d, m, giants)
    ops, lev = plan.ops, plan.levels
    lev["x"] = 0
    tmp = [0]

    def fresh(prefix):
        tmp[0] += 1
        return f"{prefix}{tmp[0]}"

    def at(name, level):
        """``name`` at ``level``: itself, or its mod-drop (emitted once)."""
        if lev[name] == level:
            return name
        assert lev[name] < level, (name, lev[name], level)
        dn = f"{name}@{level}"
        if dn not in lev:
            ops.append(("drop", dn, name, level))
            lev[dn] = level
        return dn

    power = {1: "x"}

    def make_power(n):
        a = n // 2 if n & (n - 1) == 0 else 1 << (n.bit_length() - 1)
        b = n - a
        lv = max(lev[power[a]], lev[power[b]])
        A, Bn = at(power[a], lv), at(power[b], lv)
        name = f"phi{n}"
        if not cheb:
            ops.append(("mul", name, A, Bn))
        elif fused:
            if a != b:  # T_n = 2 T_a T_b - T_{a-b}
                ops.append(("fma", name, A, Bn, 2, at(power[a - b], lv + 1), -1, 0, 0.0))
            else:  # T_2a = 2 T_a^2 - 1, the constant at the scale 2^logp
                ops.append(("fma", name, A, Bn, 2, None, 0, -(1 << logp), -1.0))
        else:
            t = fresh("t")
            ops.append(("mul", t, A, Bn))
            lev[t] = lv + 1
            if a != b:  # T_n = 2 T_a T_b - T_{a-b}
                C = at(power[a - b], lv + 1)
                ops.append(("lincomb", [name], [t, C], [[2, -1]], None, False, [[2.0, -1.0]], None))
            else:  # T_2a = 2 T_a^2 - 1, the constant at the scale 2^logp
                ops.append(("lincomb", [name], [t], [[2]], [-(1 << logp)], False, [[2.0]], [-1.0]))
        lev[name] = lv + 1
        power[n] = name

    for n in list(range(2, m)) + giants:
        make_power(n)

    # the tree of splits; its leaves are the polynomials of degree < m
    leaves = []
    unit = {}

    def split(poly):
        e = len(poly) - 1
        if e < m:
            leaves.append(poly)
            return ("leaf", len(leaves) - 1)
        g = max(x for x in giants if x <= e)
        if cheb:
            if g not in unit:
                unit[g] = [0.0] * g + [1.0]
            Q, R = _cheb.chebdiv(poly, unit[g])
            Q, R = _trim(Q), _trim(R)
        else:
            Q, R = _trim(poly[g:]), _trim(poly[:g])
        r_zero = len(R) == 1 and R[0] == 0.0
        return ("node", g, split(Q), None if r_zero else split(R))

    tree = split(P)

    # all leaves from one rescaling lincomb of the babies (chunks of MAX_TERMS)
    lb = max(lev[power[k]] for k in range(1, m))
    srcs = [at(power[k], lb) for k in range(1, m)]
    leaf_names = [f"leaf{i}" for i in range(len(leaves))]
    for c0 in range(0, len(leaves), MAX_TERMS):
        chunk = leaves[c0:c0 + MAX_TERMS]
        W, bias, fw, fb = [], [], [], []
        for poly in chunk:
            ck = [poly[k] if k < len(poly) else 0.0 for k in range(m)]
            W.append([int(np.rint(ck[k] * 2.0 ** logp)) for k in range(1, m)])
            bias.append(int(np.rint(ck[0] * 2.0 ** (2 * logp))))
            fw.append(ck[1:])
            fb.append(ck[0])
        names = leaf_names[c0:c0 + MAX_TERMS]
        ops.append(("lincomb", names, srcs, W, bias, True, fw, fb))
        for nm in names:
            lev[nm] = lb + 1

    def emit(node):
        if node[0] == "leaf":
            return leaf_names[node[1]]
        _, g, qn, rn = node
        q = emit(qn)
        lv = max(lev[q], lev[power[g]])
        if fused and rn is not None:
            r = emit(rn)
            if lev[r] <= lv + 1:  # eval(R) reaches the product's level: one call
                t = fresh("t")
                ops.append(("fma", t, at(q, lv), at(power[g], lv), 1, at(r, lv + 1), 1, 0, 0.0))
                lev[t] = lv + 1
                return t
            t = fresh("t")
            ops.append(("mul", t, at(q, lv), at(power[g], lv)))
            lev[t] = lv + 1
            s = fresh("t")
            ops.append(("add", s, at(t, lev[r]), r))
            lev[s] = lev[r]
            return s
        t = fresh("t")
        ops.append(("mul", t, at(q, lv), at(power[g], lv)))
        lev[t] = lv + 1
        if rn is None:
            return t
        r = emit(rn)
        lv2 = max(lev[t], lev[r])
        s = fresh("t")
        ops.append(("add", s, at(t, lv2), at(r, lv2)))
        lev[s] = lv2
        return s

    plan.result = emit(tree)
    assert plan.depth <= int(d).bit_length() + 1, (d, plan.depth)
    return plan
