"""The CPU execution of the fused plans (rns_ntt.poly_eval_plan_fused,
rns_ntt/evalmod.py): tests/poly_eval_ref.py's runner and model,
extended by subclassing with the one new op and the double angles.

    fma      hybrid_rescale_ref.mul_relin_rescale_hybrid_ref -- the multiply's
             own yardstick -- and then, with Python integers on every word,
             w r + u z (+ bias on coefficient 0 of component 0) mod q_t:
             affine_ref, the definition of
             rnt_ct_mul_relin_rescale_affine_hybrid's words.

PlanRunner.run keeps its table of values to itself, so FusedRunner.run walks
the op list itself; the four old ops are restated in ``_old_op`` and
tests/test_evalmod_ref.py pins the restatement against PlanRunner.run on the
unfused plans.
"""
from __future__ import annotations

import numpy as np

import pyoracle as orc
from hybrid_ref import mul_relin_hybrid_ref
from hybrid_rescale_ref import mul_relin_rescale_hybrid_ref
from lincomb_ref import lincomb_ref, reduce_weights
from poly_eval_ref import Model, PlanRunner


def affine_ref(moduli, r0, r1, w, z, u, bias):
    """(w r0 + u z0 + bias X^0, w r1 + u z1) limb by limb over ``moduli``:
    r0, r1 [L][N] canonical residues, z = (z0, z1) or None, w / u / bias signed
    Python integers.  Exact (object arithmetic), canonical."""
    out = []
    for comp, r in enumerate((r0, r1)):
        r = np.asarray(r, dtype=np.uint64)
        o = np.zeros_like(r)
        for t, q in enumerate(int(m) for m in moduli):
            acc = r[t].astype(object) * int(w)
            if z is not None:
                acc = acc + np.asarray(z[comp][t], dtype=np.uint64).astype(object) * int(u)
            if comp == 0:
                acc[0] = acc[0] + int(bias)
            o[t] = (acc % q).astype(np.uint64)
        out.append(o)
    return out[0], out[1]


class FusedRunner(PlanRunner):
    """PlanRunner that also executes ``fma`` ops, and EvalMod plans."""

    def fma(self, a, b, w, z, u, bias):
        """One fused call on ciphertexts (c0, c1) of a's limb count."""
        lv = a[0].shape[0]
        Bc, Be, ka, kb = self.level(lv)
        r0, r1 = mul_relin_rescale_hybrid_ref(Bc, Be, *a, *b, ka, kb, self.alpha)
        return affine_ref(self.q[:lv - 1], r0, r1, w, z, u, bias)

    def _old_op(self, plan, op, v):
        L = len(self.q)
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

    def run(self, plan, ct):
        L = len(self.q)
        v = {"x": (np.asarray(ct[0], dtype=np.uint64), np.asarray(ct[1], dtype=np.uint64))}
        for op in plan.ops:
            if op[0] == "fma":
                _, dst, a, b, w, z, u, bias, _ = op
                assert v[a][0].shape[0] == v[b][0].shape[0] == L - plan.levels[a]
                assert z is None or v[z][0].shape[0] == L - plan.levels[dst]
                v[dst] = self.fma(v[a], v[b], w, None if z is None else v[z], u, bias)
            else:
                self._old_op(plan, op, v)
        return v[plan.result]

    def run_evalmod(self, plan, ct):
        """The polynomial, then y <- 2 y^2 - c_j for every double angle."""
        y = self.run(plan.poly, ct)
        for c in plan.constants:
            y = self.fma(y, y, 2, None, 0, -c)
        return y


class FusedModel(Model):
    """poly_eval_ref.Model whose runner executes fused and EvalMod plans."""

    def __init__(self, q, p, n, alpha, logp, seed):
        super().__init__(q, p, n, alpha, logp, seed)
        self.runner = FusedRunner(self.q, self.p, n, alpha, self.key_a, self.key_b)
