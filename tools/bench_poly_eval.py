#!/usr/bin/env python3
"""The scalar path and the polynomial evaluator at N = 2^16 with 16 x 30-bit
ciphertext primes (+ K = 4 special primes of 31 bits, alpha = 4), in one process
on one GPU:

1. rnt_ct_lincomb_rescale at (n_in, n_out) = (7, 8): time, the bytes it must
   move -- 2 (n_in (Lv + 1) + n_out (Lv - 1)) B N word: every input plane once,
   the last limb's a second time for r_last, every output plane once, two
   components -- and the achieved bytes/s beside rnt_add's on buffers of the
   inputs' size in the same run (3 planes moved per plane added).
2. The same combination composed from calls that exist without it: the inputs
   held in the NTT domain already (their forward transforms are NOT timed), one
   pointwise rnt_mul by a constant polynomial per term, rnt_add, rnt_ntt_inv and
   rnt_ct_rescale per output.  Both results are compared word for word.
3. A degree-31 Chebyshev evaluation (CkksEngine.evaluate_polynomial_hybrid) end
   to end with the per-kernel split of one profiled run (rnt_profile_read).

Timing as tools/bench_keyswitch_hybrid.py: HIP events on the basis' stream
around enough back-to-back calls to last `--window` seconds, after `--warmup`
calls, `--repeats` windows, the forms of a comparison taken in turn.  One JSON
line per measurement on stdout and, with --out, appended to that file.

    python tools/bench_poly_eval.py --out profiles/poly_eval_bench.jsonl
"""
from __future__ import annotations

import argparse
import ctypes
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

bkh.KERNELS = tuple(dict.fromkeys(bkh.KERNELS + ("lincomb", "moddown_rescale", "rescale", "mf_mul", "whole_mul")))
LOG_N, L, K, ALPHA = 16, 16, 4, 4
N_IN, N_OUT = 7, 8
DEGREE = 31


def clock_mhz():
    try:
        import torch

        return int(torch.cuda.clock_rate())
    except Exception:  # not every torch build exposes it
        return None


def emit(r, out):
    r.update({"log_n": LOG_N, "L": L, "K": K, "alpha": ALPHA, "bits": 30, "sclk_mhz": clock_mhz()})
    line = json.dumps(r)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def run_lincomb(basis, B, a, out):
    n, word = 1 << LOG_N, 4
    rng = rn.DeviceRng(3100 + B)
    lib = rn.load()
    mods = basis.moduli()
    low = basis.drop_last(1)
    host = np.random.default_rng(B)
    ints = [[int(v) for v in row] for row in host.integers(-(1 << 40), 1 << 40, size=(N_OUT, N_IN))]
    x = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, N_IN * B), rn.RnsPoly.sample_uniform(basis, rng, N_IN * B))
    w = np.array([[[v % q for q in mods] for v in row] for row in ints], dtype=np.uint64)
    wp = w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    fo = rn.Ciphertext(rn.RnsPoly(low, N_OUT * B), rn.RnsPoly(low, N_OUT * B))
    tmp = rn.RnsPoly(basis, N_IN * B)

    def call_lincomb():
        rn.check(lib.rnt_ct_lincomb_rescale(fo.c0.handle, fo.c1.handle, x.c0.handle, x.c1.handle, N_IN, N_OUT, wp, None))

    def call_add():
        rn.check(lib.rnt_add(tmp.handle, x.c0.handle, x.c1.handle))

    # the composition: per-term buffers, inputs already in the NTT domain
    terms = []
    for comp in (x.c0, x.c1):
        row = []
        for i in range(N_IN):
            t = rn.RnsPoly(basis, B)
            t.copy_polys(comp, 0, i * B, B)
            t.to_ntt_domain()
            row.append(t)
        terms.append(row)
    consts = []
    for j in range(N_OUT):
        row = []
        for i in range(N_IN):
            c = np.zeros((B, n), dtype=np.int64)
            c[:, 0] = ints[j][i]  # |weight| < 2^40: from_coeffs reduces it into every limb
            p = rn.RnsPoly.from_coeffs(c, basis)
            p.to_ntt_domain()
            row.append(p)
        consts.append(row)
    acc = [[rn.RnsPoly(basis, B) for _ in range(N_OUT)] for _ in range(2)]
    prod = rn.RnsPoly(basis, B)
    co = [[rn.RnsPoly(low, B) for _ in range(N_OUT)] for _ in range(2)]

    def call_composed():
        for j in range(N_OUT):
            for comp in range(2):
                rn.check(lib.rnt_mul(acc[comp][j].handle, terms[comp][0].handle, consts[j][0].handle))
                for i in range(1, N_IN):
                    rn.check(lib.rnt_mul(prod.handle, terms[comp][i].handle, consts[j][i].handle))
                    rn.check(lib.rnt_add(acc[comp][j].handle, acc[comp][j].handle, prod.handle))
                rn.check(lib.rnt_ntt_inv(acc[comp][j].handle))
            rn.check(lib.rnt_ct_rescale(co[0][j].handle, co[1][j].handle, acc[0][j].handle, acc[1][j].handle))

    tm = Timer(basis, a.warmup, a.repeats, a.window)
    (t_l, t_a, t_c), iters = tm.alternate([call_lincomb, call_add, call_composed])
    split_l, split_c = tm.split(call_lincomb), tm.split(call_composed)
    equal = True
    for j in range(N_OUT):
        for comp, f in enumerate((fo.c0, fo.c1)):
            equal = equal and bool(np.array_equal(f.channels_of(j * B, 1)[0], co[comp][j].channels_of(0, 1)[0]))
    lc_bytes = 2 * (N_IN * (L + 1) + N_OUT * (L - 1)) * B * n * word
    add_bytes = 3 * N_IN * B * L * n * word
    lc_rate = lc_bytes / (float(np.median(t_l)) * 1e-3)
    add_rate = add_bytes / (float(np.median(t_a)) * 1e-3)
    emit({"bench": "lincomb_rescale", "batch": B, "n_in": N_IN, "n_out": N_OUT,
          "iters": {"lincomb": iters[0], "add": iters[1], "composed": iters[2]},
          "lincomb_ms": t_l, "add_ms": t_a, "composed_ms": t_c, "lincomb_bytes": lc_bytes, "add_bytes": add_bytes,
          "lincomb_GBs": round(lc_rate / 1e9, 1), "add_GBs": round(add_rate / 1e9, 1),
          "lincomb_over_add_rate": round(lc_rate / add_rate, 3),
          "composed_over_lincomb_time": round(float(np.median(t_c) / np.median(t_l)), 2),
          "composed_excludes": "the forward transforms of the inputs",
          "lincomb_equals_composed_poly0": equal, "lincomb_kernels": split_l, "composed_kernels": split_c}, out)
    return equal


def run_eval(ext, basis, B, a, out):
    from rns_ntt.engine import CkksEngine

    rng = rn.DeviceRng(3200 + B)
    beta = -(-L // ALPHA)
    key = rn.RnsHybridKey(rn.RnsPoly.sample_uniform(ext, rng, beta), rn.RnsPoly.sample_uniform(ext, rng, beta), ALPHA,
                          n_special=K)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B), 30,
                       basis.total_bits())
    coeffs = np.random.default_rng(31).uniform(-1, 1, DEGREE + 1)
    plan = rn.poly_eval_plan(coeffs, "chebyshev", 30)
    res = []

    def call_eval():
        res[:] = [CkksEngine.evaluate_polynomial_hybrid(ct, coeffs, key, basis="chebyshev")]

    tm = Timer(basis, a.warmup, a.repeats, a.window)
    (t_e,), iters = tm.alternate([call_eval])
    split = tm.split(call_eval)
    counts = {k: sum(op[0] == k for op in plan.ops) for k in ("mul", "lincomb", "add", "drop")}
    emit({"bench": "poly_eval_chebyshev", "degree": DEGREE, "batch": B, "depth": plan.depth, "plan_ops": counts,
          "leaves": plan.n_leaves, "iters": iters[0], "eval_ms": t_e, "out_limbs": res[0].c0.basis.channel_count(),
          "kernels": split, "kernel_ms_sum": round(sum(v["ms"] for v in split.values()), 4)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="append", type=int, help="ciphertexts (repeatable; default 1 and 64)")
    ap.add_argument("--no-lincomb", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    n = 1 << LOG_N
    ext = rn.RnsBasis(rn.generate_primes(30, L, n) + rn.generate_primes(31, K, n), n)
    basis = ext.drop_last(K)
    ok = True
    for B in a.batch or [1, 64]:
        if not a.no_lincomb:
            ok = run_lincomb(basis, B, a, a.out) and ok
            rn.pool_trim()
        if not a.no_eval:
            run_eval(ext, basis, B, a, a.out)
            rn.pool_trim()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
