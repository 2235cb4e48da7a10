#!/usr/bin/env python3
"""rnt_ct_linear against the composition of the public ops it replaces
(rnt_ct_rotate, two rnt_mul, two rnt_add per term), in one process on one
GPU: the composition's kernels are the library's own, unchanged.

Timing: HIP events on the basis' stream around `--iters` back-to-back calls,
after `--warmup` calls, `--repeats` times; then one profiled call of each for
the per-kernel split (rnt_profile_read), then parity of the two outputs on
one ciphertext.  One JSON line per shape on stdout.

    python tools/bench_linear.py                 # the three shapes of DESIGN.md
    python tools/bench_linear.py --shape 16,16,31,8,64
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

KERNELS = ("automorphism", "ks_decompose", "ks_rows", "ks_whole", "col_inv", "col_fwd", "row_fwd", "row_inv",
           "row_mul", "mf_ntt_fwd", "mf_ntt_inv", "mf_mul", "plane_fused", "whole_fwd", "whole_inv", "whole_mul",
           "elementwise", "copy")
SHAPES = [(16, 16, 31, 8, 1), (16, 16, 31, 8, 64), (17, 32, 31, 8, 1)]


def run_shape(log_n, L, bits, terms, B, warmup, iters, repeats):
    import torch

    n = 1 << log_n
    basis = rn.RnsBasis(rn.generate_primes(bits, L, n), n)
    lib = rn.load()
    rng = rn.DeviceRng(2024)
    steps = list(range(1, terms + 1))
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    keys = [rn.RnsGadgetKey(rn.RnsPoly.sample_uniform(basis, rng, L), rn.RnsPoly.sample_uniform(basis, rng, L), k)
            for k in steps]
    keyset = rn.RnsGadgetKeySet(keys, basis)
    dcoef = rn.RnsPoly.sample_uniform(basis, rng, terms)  # the plaintexts, coefficient domain
    diag = dcoef.clone()
    diag.to_ntt_domain()
    # the composition multiplies whole batches: plaintext t repeated B times
    dB = []
    for t in range(terms):
        m = rn.RnsPoly(basis, B)
        for p in range(B):
            m.copy_polys(dcoef, p, t, 1)
        dB.append(m)
    fused = rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))
    acc = [rn.RnsPoly(basis, B), rn.RnsPoly(basis, B)]
    tmp = [rn.RnsPoly(basis, B), rn.RnsPoly(basis, B)]

    def call_fused():
        rn.linear_transform(ct, diag, keyset, out=fused)

    def call_composed():
        for t, key in enumerate(keys):
            rn.check(lib.rnt_ct_rotate(tmp[0].handle, tmp[1].handle, ct.c0.handle, ct.c1.handle, steps[t],
                                       key.a.handle, key.b.handle))
            for o in range(2):
                if t == 0:
                    rn.check(lib.rnt_mul(acc[o].handle, tmp[o].handle, dB[t].handle))
                else:
                    rn.check(lib.rnt_mul(tmp[o].handle, tmp[o].handle, dB[t].handle))
                    rn.check(lib.rnt_add(acc[o].handle, acc[o].handle, tmp[o].handle))

    stream = torch.cuda.ExternalStream(basis.stream())

    def timed(fn):
        for _ in range(warmup):
            fn()
        basis.sync()
        out = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(iters):
                fn()
            b.record(stream)
            b.synchronize()
            out.append(a.elapsed_time(b) / iters)
        return out

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

    t_comp = timed(call_composed)
    t_fused = timed(call_fused)
    s_comp, s_fused = split(call_composed), split(call_fused)
    p = B - 1
    parity = bool(np.array_equal(fused.c0.channels_of(p), acc[0].channels_of(p)) and
                  np.array_equal(fused.c1.channels_of(p), acc[1].channels_of(p)))
    return {"log_n": log_n, "L": L, "bits": bits, "terms": terms, "batch": B, "iters": iters,
            "composed_ms": [round(x, 4) for x in t_comp], "fused_ms": [round(x, 4) for x in t_fused],
            "speedup_median": round(float(np.median(t_comp) / np.median(t_fused)), 3),
            "composed_kernels": s_comp, "fused_kernels": s_fused, "parity": parity}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="log_n,L,bits,terms,batch (repeatable)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shape] if a.shape else SHAPES
    ok = True
    for sh in shapes:
        r = run_shape(*sh, a.warmup, a.iters, a.repeats)
        ok = ok and r["parity"]
        print(json.dumps(r), flush=True)
        rn.pool_trim()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
