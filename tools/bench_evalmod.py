#!/usr/bin/env python3
"""EvalMod and the fused polynomial evaluator at N = 2^16 with 16 x 30-bit
ciphertext primes (+ K = 2 special primes of 31 bits, alpha = 2), in one process
on one GPU, against the unfused composition of the calls that existed before
the fused multiply-add:

  evalmod    CkksEngine.eval_mod_hybrid on evalmod_plan(16, 31, 3, 30) (depth 9)
             against evaluate_polynomial_hybrid of the same
             Chebyshev coefficients followed, per double angle, by
             mul_ciphertexts_hybrid_rescale and an un-rescaled ct_lincomb;
  evaluator  evaluate_polynomial_hybrid_fused against evaluate_polynomial_hybrid on
             those coefficients (the polynomial part alone).

The inputs are uniform residues (the time of exact arithmetic does not depend on
the values); tests/test_gpu_evalmod.py holds the words.  B = 1 and 8.

Timing as tools/bench_ct_dot_hybrid.py: HIP events on the basis' stream around
enough back-to-back calls to last `--window` seconds, after `--warmup` calls,
`--repeats` windows, the forms taken in turn.  One JSON line per (bench, B) with
the windows, the ratio of the medians and the per-kernel split of one profiled
run of either form (rnt_profile_read): moddown_rescale_affine next to
moddown_rescale + lincomb.  On stdout and, with --out, appended to that file.

    python tools/bench_evalmod.py --out profiles/evalmod_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("toy-heaan-ckks_amd", "oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(REPO, p))

import numpy as np  # noqa: E402

import rns_ntt as rn  # noqa: E402
import bench_keyswitch_hybrid as bkh  # noqa: E402
from bench_keyswitch_hybrid import Timer  # noqa: E402
from rns_ntt.engine import CkksEngine  # noqa: E402

bkh.KERNELS = tuple(dict.fromkeys(bkh.KERNELS + ("lincomb", "moddown_rescale", "moddown_rescale_affine", "rescale",
                                                 "mf_mul", "whole_mul")))
LOG_N, L, K, ALPHA, LOGP = 16, 16, 2, 2, 30
PLAN = (16, 31, 3)


def clock_mhz():
    try:
        import torch

        return int(torch.cuda.clock_rate())
    except Exception:  # not every torch build exposes it
        return None


def emit(r, out):
    r.update({"log_n": LOG_N, "L": L, "K": K, "alpha": ALPHA, "bits": 30, "plan": list(PLAN), "sclk_mhz": clock_mhz()})
    line = json.dumps(r)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def report(tm, name, B, fused, plain, out):
    (t_f, t_p), iters = tm.alternate([fused, plain])
    split_f, split_p = tm.split(fused), tm.split(plain)
    mf, mp = float(np.median(t_f)), float(np.median(t_p))
    emit({"bench": name, "batch": B, "iters": {"fused": iters[0], "unfused": iters[1]}, "fused_ms": t_f,
          "unfused_ms": t_p, "unfused_over_fused_time": round(mp / mf, 4),
          "fused_spread": round((max(t_f) - min(t_f)) / mf, 4), "unfused_spread": round((max(t_p) - min(t_p)) / mp, 4),
          "fused_kernels": split_f, "unfused_kernels": split_p,
          "fused_kernel_ms_sum": round(sum(v["ms"] for v in split_f.values()), 4),
          "unfused_kernel_ms_sum": round(sum(v["ms"] for v in split_p.values()), 4),
          "fused_launches": sum(v["launches"] for v in split_f.values()),
          "unfused_launches": sum(v["launches"] for v in split_p.values())}, out)


def run(basis, key, B, a, out):
    rng = rn.DeviceRng(5100 + B)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B), LOGP,
                       basis.total_bits())
    plan = rn.evalmod_plan(*PLAN, LOGP)
    assert plan.depth == 9

    def poly_fused():
        return CkksEngine.evaluate_polynomial_hybrid_fused(ct, plan.coeffs, key, basis="chebyshev")

    def poly_plain():
        return CkksEngine.evaluate_polynomial_hybrid(ct, plan.coeffs, key, basis="chebyshev")

    def evalmod_fused():
        return CkksEngine.eval_mod_hybrid(ct, plan, key)

    def evalmod_plain():
        y = poly_plain()
        for c in plan.constants:
            t = rn.mul_ciphertexts_hybrid_rescale(y, y, key)
            y = rn.ct_lincomb(t, 1, [[2]], [-c], rescale=False)
        return y

    tm = Timer(basis, a.warmup, a.repeats, a.window)
    report(tm, "evalmod", B, evalmod_fused, evalmod_plain, out)
    report(tm, "evaluator", B, poly_fused, poly_plain, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="append", type=int, help="ciphertexts (repeatable; default 1 and 8)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    n = 1 << LOG_N
    ext = rn.RnsBasis(rn.generate_primes(30, L, n) + rn.generate_primes(31, K, n), n)
    basis = ext.drop_last(K)
    rng = rn.DeviceRng(5000)
    beta = -(-L // ALPHA)
    key = rn.RnsHybridKey(rn.RnsPoly.sample_uniform(ext, rng, beta), rn.RnsPoly.sample_uniform(ext, rng, beta), ALPHA,
                          n_special=K)
    for B in a.batch or [1, 8]:
        run(basis, key, B, a, a.out)
        rn.pool_trim()
    return 0


if __name__ == "__main__":
    sys.exit(main())
