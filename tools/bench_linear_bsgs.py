#!/usr/bin/env python3
"""rnt_ct_linear_bsgs against rnt_ct_linear on the same diagonals, in one
process on one GPU.  The matrix is a band of n1 n2 diagonals 0 .. n1 n2 - 1:
baby steps 0 .. n1 - 1, giant steps 0, n1, .. (n2 - 1) n1 for the one call,
steps 0 .. n1 n2 - 1 for the other (random keys and plaintexts: the two calls
are timed, their words differ by definition).

Timing: HIP events on the basis' stream around `--iters` back-to-back calls,
after `--warmup` calls, `--repeats` times; then one profiled call of each for
the per-kernel split (rnt_profile_read).  One JSON line per shape on stdout
and, with --out, appended to that file.

    python tools/bench_linear_bsgs.py --out profiles/linear_bsgs_bench.jsonl
    python tools/bench_linear_bsgs.py --shape 16,16,31,4,4,64
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "toy-heaan-ckks_amd"))

import numpy as np  # noqa: E402

import rns_ntt as rn  # noqa: E402

KERNELS = ("automorphism", "ks_decompose", "ks_rows", "ks_whole", "bsgs_mac", "col_inv", "col_fwd", "row_fwd",
           "row_inv", "mf_ntt_fwd", "mf_ntt_inv", "whole_fwd", "whole_inv", "elementwise", "copy")
# log_n, L, bits, n1, n2, batch, iters
SHAPES = [(16, 16, 31, 8, 8, 1, 10), (16, 16, 31, 4, 4, 64, 3), (17, 32, 31, 4, 4, 1, 10)]


def key_set(basis, rng, steps):
    L = basis.channel_count()
    keys = [None if k == 0 else
            rn.RnsGadgetKey(rn.RnsPoly.sample_uniform(basis, rng, L), rn.RnsPoly.sample_uniform(basis, rng, L), k)
            for k in steps]
    return rn.RnsGadgetKeySet(keys, basis)


def run_shape(log_n, L, bits, n1, n2, B, iters, warmup, repeats):
    import torch

    n = 1 << log_n
    basis = rn.RnsBasis(rn.generate_primes(bits, L, n), n)
    rng = rn.DeviceRng(2025)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    baby, giant = list(range(n1)), [j * n1 for j in range(n2)]
    flat = list(range(n1 * n2))
    diag = rn.RnsPoly.sample_uniform(basis, rng, n1 * n2)
    diag.to_ntt_domain()
    bset, gset = key_set(basis, rng, baby), key_set(basis, rng, giant)
    fset = key_set(basis, rng, flat)
    out = rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))

    def call_bsgs():
        rn.linear_transform_bsgs(ct, diag, bset, gset, out=out)

    def call_flat():
        rn.linear_transform(ct, diag, fset, out=out)

    stream = torch.cuda.ExternalStream(basis.stream())

    def timed(fn):
        for _ in range(warmup):
            fn()
        basis.sync()
        res = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(iters):
                fn()
            b.record(stream)
            b.synchronize()
            res.append(a.elapsed_time(b) / iters)
        return res

    def split(fn):
        basis.profile_enable(True)
        fn()
        res = {}
        for k in KERNELS:
            cnt, ms = basis.profile_read(k)
            if cnt:
                res[k] = {"launches": cnt, "ms": round(ms, 4)}
        basis.profile_enable(False)
        return res

    t_flat = timed(call_flat)
    t_bsgs = timed(call_bsgs)
    s_flat, s_bsgs = split(call_flat), split(call_bsgs)
    return {"log_n": log_n, "L": L, "bits": bits, "n_baby": n1, "n_giant": n2, "diagonals": n1 * n2, "batch": B,
            "iters": iters, "linear_ms": [round(x, 4) for x in t_flat], "bsgs_ms": [round(x, 4) for x in t_bsgs],
            "speedup_median": round(float(np.median(t_flat) / np.median(t_bsgs)), 3),
            "linear_kernels": s_flat, "bsgs_kernels": s_bsgs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="log_n,L,bits,n_baby,n_giant,batch[,iters] (repeatable)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    shapes = SHAPES
    if a.shape:
        shapes = []
        for s in a.shape:
            v = [int(x) for x in s.split(",")]
            shapes.append(tuple(v) if len(v) == 7 else tuple(v) + (10,))
    for sh in shapes:
        r = run_shape(*sh, a.warmup, a.repeats)
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        rn.pool_trim()
    return 0


if __name__ == "__main__":
    sys.exit(main())
