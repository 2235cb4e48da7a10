#!/usr/bin/env python3
"""The decode errors of the fused polynomial evaluator and of EvalMod measured
on the CPU: the tolerances of tests/test_gpu_evalmod.py and
tests/test_evalmod_ref.py.  Writes profiles/evalmod_tolerance.txt.

Two rings, the tests' own, both N = 2^10, alpha = 2, scale 2^30, ternary secret
of weight N / 2, errors of width 3.2, 2 special primes of 31 bits:

  evaluator  7 ciphertext primes of 30 bits (tests/test_gpu_poly_eval.py's
             ring); degrees 7 and 15 in both bases, inputs and coefficients
             uniform in (-1, 1), against numpy.polyval / chebval;
  EvalMod    9 ciphertext primes of 30 bits; evalmod_plan(4, 15, 2, 30), inputs
             u = (I + eps) / 4 with integer |I| <= 3 and |eps| <= 2^-8, against
             sin(2 pi eps) / (2 pi).

For each seed every case runs twice on tests/evalmod_ref.py (the CPU model of
tests/poly_eval_ref.py with the fused op): the fused plan, and beside it the
unfused composition of the calls that existed before -- poly_eval_plan's
default schedule, and per double angle a multiply followed by an un-rescaled
lincomb.  The two compute the same words wherever their schedules agree, so the
figures differ only through the order of the additions.  Results are decoded at
the NOMINAL scale 2^30: the drift of q != 2^30, which the engine's integer logp
ignores, is part of every figure and most of it.  No device is touched.

    python tools/evalmod_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "toy-heaan-ckks_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

import pyoracle as orc  # noqa: E402
from evalmod_ref import FusedModel  # noqa: E402
from poly_eval_ref import plain_value  # noqa: E402
from rns_ntt.evalmod import evalmod_plan  # noqa: E402  (pure host modules: the library is not loaded)
from rns_ntt.poly_eval import poly_eval_plan, poly_eval_plan_fused  # noqa: E402

N, K, ALPHA, LOGP = 1024, 2, 2, 30
L_EVAL, L_MOD = 7, 9
CASES = [(7, "monomial"), (7, "chebyshev"), (15, "monomial"), (15, "chebyshev")]
EVALMOD = (4, 15, 2)
EPS = 2.0 ** -8
OUT = os.path.join(REPO, "profiles", "evalmod_tolerance.txt")


def ring_moduli(L):
    return orc.generate_primes(LOGP, L, N), orc.generate_primes(31, K, N)


def evalmod_inputs(rng, Kmod, count):
    I = rng.integers(-(Kmod - 1), Kmod, count)
    eps = rng.uniform(-EPS, EPS, count)
    return (I + eps) / Kmod, eps


def unfused_evalmod(runner, plan, ct):
    """EvalMod from the calls that existed before the fused one: the default
    schedule of the polynomial, then per double angle a multiply and an
    un-rescaled lincomb 2 t - c."""
    from hybrid_rescale_ref import mul_relin_rescale_hybrid_ref
    from lincomb_ref import lincomb_ref, reduce_weights

    y = runner.run(poly_eval_plan(plan.coeffs, "chebyshev", plan.logp), ct)
    for c in plan.constants:
        lv = y[0].shape[0]
        Bc, Be, ka, kb = runner.level(lv)
        t0, t1 = mul_relin_rescale_hybrid_ref(Bc, Be, *y, *y, ka, kb, runner.alpha)
        Bl = runner.level(lv - 1)[0]
        q = runner.q[:lv - 1]
        o0, o1 = lincomb_ref(Bl, t0[None], t1[None], 1, reduce_weights([[2]], q), reduce_weights([-c], q),
                             rescale=False)
        y = (o0[0], o1[0])
    return y


def run_eval(seed, degree, basis):
    model = FusedModel(*ring_moduli(L_EVAL), N, ALPHA, LOGP, seed)
    x = model.rng.uniform(-1, 1, N // 2)
    coeffs = model.rng.uniform(-1, 1, degree + 1)
    ct = model.encrypt(x)
    want = plain_value(coeffs, basis, x)
    out = []
    for fused in (True, False):
        plan = (poly_eval_plan_fused if fused else poly_eval_plan)(coeffs, basis, LOGP)
        got = model.decode(model.runner.run(plan, ct))
        out.append(float(np.max(np.abs(got - want))))
    return out


def run_evalmod(seed):
    model = FusedModel(*ring_moduli(L_MOD), N, ALPHA, LOGP, seed)
    u, eps = evalmod_inputs(model.rng, EVALMOD[0], N // 2)
    plan = evalmod_plan(*EVALMOD, LOGP)
    ct = model.encrypt(u)
    want = np.sin(2 * np.pi * eps) / (2 * np.pi)
    fused = model.decode(model.runner.run_evalmod(plan, ct))
    plain = model.decode(unfused_evalmod(model.runner, plan, ct))
    return [float(np.max(np.abs(fused - want))), float(np.max(np.abs(plain - want)))]


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    names = [f"degree {d:2d} {b:9s}" for d, b in CASES] + ["evalmod (K, degree, r) = (%d, %d, %d)" % EVALMOD]
    worst = {nm: [0.0, 0.0] for nm in names}
    for seed in range(n_seeds):
        for nm, c in zip(names, CASES + [None]):
            e = run_evalmod(seed) if c is None else run_eval(seed, *c)
            worst[nm] = [max(a, b) for a, b in zip(worst[nm], e)]
            say(f"seed {seed}: {nm}: decode error fused {e[0]:.3e}  unfused {e[1]:.3e}")
    for nm in names:
        say(f"{nm}: largest error over {n_seeds} seeds fused {worst[nm][0]:.3e} (tolerance 4 x = "
            f"{4 * worst[nm][0]:.3e})  unfused {worst[nm][1]:.3e}")
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
