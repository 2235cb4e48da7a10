#!/usr/bin/env python3
"""The hybrid ciphertext inner product at N = 2^16 with 16 x 30-bit ciphertext
primes (+ K = 4 special primes of 31 bits, alpha = 4), in one process on one
GPU: rnt_ct_dot_relin_rescale_hybrid on n_terms packed ciphertext pairs against
the loop it replaces -- one rnt_ct_mul_relin_rescale_hybrid per term and an
rnt_add of both components from the second term on -- on the same inputs (the
loop reads per-term copies made before the timing), for n_terms in {2, 4, 8,
16} and B in {1, 64} ciphertexts.  The two results are different words by
definition (one ModDown of a sum against a sum of ModDowns) and are not
compared here: tests/test_gpu_dot_hybrid.py holds the words.

Timing as tools/bench_keyswitch_hybrid.py: HIP events on the basis' stream
around enough back-to-back calls to last `--window` seconds, after `--warmup`
calls, `--repeats` windows, the two forms taken in turn.  One JSON line per
(n_terms, B) with the per-kernel split of one profiled run of either form
(rnt_profile_read) and the ratio of the medians, on stdout and, with --out,
appended to that file.

    python tools/bench_ct_dot_hybrid.py --out profiles/ct_dot_hybrid_bench.jsonl
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

bkh.KERNELS = tuple(dict.fromkeys(bkh.KERNELS + ("dot_tensor", "moddown_rescale", "rescale")))
LOG_N, L, K, ALPHA = 16, 16, 4, 4


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


def run(ext, basis, key, n_terms, B, a, out):
    n, word = 1 << LOG_N, 4
    rng = rn.DeviceRng(4100 + 100 * n_terms + B)
    lib = rn.load()
    low = basis.drop_last(1)
    x = rn.Ciphertext(*[rn.RnsPoly.sample_uniform(basis, rng, n_terms * B) for _ in range(2)])
    y = rn.Ciphertext(*[rn.RnsPoly.sample_uniform(basis, rng, n_terms * B) for _ in range(2)])
    fo = [rn.RnsPoly(low, B) for _ in range(2)]

    def call_dot():
        rn.check(lib.rnt_ct_dot_relin_rescale_hybrid(fo[0].handle, fo[1].handle, x.c0.handle, x.c1.handle, y.c0.handle,
                                                     y.c1.handle, n_terms, key.a.handle, key.b.handle, ALPHA))

    def term(p, i):
        t = rn.RnsPoly(basis, B)
        t.copy_polys(p, 0, i * B, B)
        return t

    terms = [[term(p, i) for p in (x.c0, x.c1, y.c0, y.c1)] for i in range(n_terms)]
    acc = [rn.RnsPoly(low, B) for _ in range(2)]
    tmp = [rn.RnsPoly(low, B) for _ in range(2)]

    def call_loop():
        for i, t in enumerate(terms):
            o = acc if i == 0 else tmp
            rn.check(lib.rnt_ct_mul_relin_rescale_hybrid(o[0].handle, o[1].handle, t[0].handle, t[1].handle,
                                                         t[2].handle, t[3].handle, key.a.handle, key.b.handle, ALPHA))
            if i:
                rn.check(lib.rnt_add(acc[0].handle, acc[0].handle, tmp[0].handle))
                rn.check(lib.rnt_add(acc[1].handle, acc[1].handle, tmp[1].handle))

    tm = Timer(basis, a.warmup, a.repeats, a.window)
    (t_d, t_l), iters = tm.alternate([call_dot, call_loop])
    split_d, split_l = tm.split(call_dot), tm.split(call_loop)
    beta = -(-L // ALPHA)
    # planes of B N words a call must move (DESIGN.md "Hybrid inner product"): per term the gather (8 Lv), four
    # transforms in place (8 Lv) and the tensor's reads (4 Lv); per group of kDotT = 4 terms the sums (3 Lv
    # written, 3 Lv read again from the second group on); once d2's inverse and unscale (4 Lv) and the fused
    # tail (ModUp Lv + beta LE, digit transforms 2 beta LE, key products beta LE + 2 Lv + 2 LE, two inverses
    # 4 LE, two ModDown-rescales 2 LE + 2 (Lv - 1))
    groups = -(-n_terms // 4)
    LE = L + K
    tail = 3 * L + 4 * beta * LE + 8 * LE + 2 * (L - 1)
    dot_planes = n_terms * 20 * L + (6 * groups - 3) * L + 4 * L + tail
    dot_bytes = dot_planes * B * n * word
    md, ml = float(np.median(t_d)), float(np.median(t_l))
    emit({"bench": "ct_dot_hybrid_rescale", "n_terms": n_terms, "batch": B, "iters": {"dot": iters[0], "loop": iters[1]},
          "dot_ms": t_d, "loop_ms": t_l, "loop_over_dot_time": round(ml / md, 3),
          "dot_ms_per_term": round(md / n_terms, 4), "loop_ms_per_term": round(ml / n_terms, 4),
          "dot_model_bytes": dot_bytes, "dot_model_GBs": round(dot_bytes / (md * 1e-3) / 1e9, 1),
          "dot_kernels": split_d, "loop_kernels": split_l,
          "dot_kernel_ms_sum": round(sum(v["ms"] for v in split_d.values()), 4),
          "loop_kernel_ms_sum": round(sum(v["ms"] for v in split_l.values()), 4)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="append", type=int, help="ciphertexts (repeatable; default 1 and 64)")
    ap.add_argument("--terms", action="append", type=int, help="n_terms (repeatable; default 2, 4, 8, 16)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    n = 1 << LOG_N
    ext = rn.RnsBasis(rn.generate_primes(30, L, n) + rn.generate_primes(31, K, n), n)
    basis = ext.drop_last(K)
    rng = rn.DeviceRng(4000)
    beta = -(-L // ALPHA)
    key = rn.RnsHybridKey(rn.RnsPoly.sample_uniform(ext, rng, beta), rn.RnsPoly.sample_uniform(ext, rng, beta), ALPHA)
    for B in a.batch or [1, 64]:
        for n_terms in a.terms or [2, 4, 8, 16]:
            run(ext, basis, key, n_terms, B, a, a.out)
            rn.pool_trim()
    return 0


if __name__ == "__main__":
    sys.exit(main())
