#!/usr/bin/env python3
"""rnt_ct_rotate against rnt_ct_rotate_hybrid, and rnt_ct_mul_relin against
rnt_ct_mul_relin_hybrid, on the same ciphertexts in one process on one GPU.
The two forms give different words by definition, so each is checked against
its own expected result after the timing, on ciphertext 0: the hybrid calls
against tests/hybrid_ref.py, the gadget calls against the oracle.

Timing: the two forms alternate; each window is HIP events on the basis'
stream around enough back-to-back calls to last `--window` seconds (sized from
a first timed call), after `--warmup` calls, `--repeats` windows each; then
one profiled call of each for the per-kernel split (rnt_profile_read).  One
JSON line per measurement on stdout and, with --out, appended to that file.

    python tools/bench_keyswitch_hybrid.py --out profiles/keyswitch_hybrid_bench.jsonl
    python tools/bench_keyswitch_hybrid.py --rotate 14,8,2,2,256 --no-mul
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("toy-heaan-ckks_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import numpy as np  # noqa: E402

import rns_ntt as rn  # noqa: E402

KERNELS = ("modup", "moddown", "hoist_mac", "automorphism", "ks_decompose", "ks_rows", "ks_whole", "col_inv",
           "col_fwd", "row_fwd", "row_inv", "mf_ntt_fwd", "mf_ntt_inv", "whole_fwd", "whole_inv", "tensor_rows",
           "tensor_whole", "mf_tensor", "elementwise", "copy")
# log_n, L, alpha (= K), batch
ROTATE = [(14, 8, 2, 256), (16, 16, 4, 1), (16, 16, 4, 64), (17, 32, 8, 1)]
MUL = [(16, 16, 4, 64)]
BITS = 31
STEP = 1


class Timer:
    def __init__(self, basis, warmup, repeats, window):
        import torch

        self.torch, self.basis, self.warmup, self.repeats, self.window = torch, basis, warmup, repeats, window
        self.stream = torch.cuda.ExternalStream(basis.stream())

    def _window(self, fn, iters):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        for _ in range(iters):
            fn()
        b.record(self.stream)
        b.synchronize()
        return a.elapsed_time(b) / iters

    def alternate(self, fns):
        """ms per call of every fn, `repeats` windows each, taken in turn."""
        iters = []
        for fn in fns:
            for _ in range(self.warmup):
                fn()
            self.basis.sync()
            iters.append(max(1, int(np.ceil(self.window * 1e3 / max(self._window(fn, 1), 1e-3)))))
        res = [[] for _ in fns]
        for _ in range(self.repeats):
            for i, fn in enumerate(fns):
                res[i].append(round(self._window(fn, iters[i]), 4))
        return res, iters

    def split(self, fn):
        self.basis.profile_enable(True)
        fn()
        res = {}
        for k in KERNELS:
            cnt, ms = self.basis.profile_read(k)
            if cnt:
                res[k] = {"launches": cnt, "ms": round(ms, 4)}
        self.basis.profile_enable(False)
        return res


def setup(log_n, L, alpha, B):
    n, K = 1 << log_n, alpha
    primes = rn.generate_primes(BITS, L + K, n)
    ext = rn.RnsBasis(primes, n)
    basis = ext.drop_last(K)
    rng = rn.DeviceRng(2028)
    beta = -(-L // alpha)
    gk = rn.RnsGadgetKey(rn.RnsPoly.sample_uniform(basis, rng, L), rn.RnsPoly.sample_uniform(basis, rng, L), STEP)
    ha, hb = rn.RnsPoly.sample_uniform(ext, rng, beta), rn.RnsPoly.sample_uniform(ext, rng, beta)
    host = (ha.channels(), hb.channels())
    hk = rn.RnsHybridKey(ha, hb, alpha, STEP)
    cts = [rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
           for _ in range(2)]
    return primes, basis, gk, hk, host, cts


def gadget_host(gk):
    a, b = gk.a.clone(), gk.b.clone()
    a.to_coeff_domain()
    b.to_coeff_domain()
    return a.channels(), b.channels()


def same(p, w):
    return bool(np.array_equal(p.channels_of(0)[0], w))


def run(kind, log_n, L, alpha, B, a):
    import pyoracle as orc
    from hybrid_ref import mul_relin_hybrid_ref, rotate_hybrid_ref

    primes, basis, gk, hk, host, (ct, ctp) = setup(log_n, L, alpha, B)
    lib = rn.load()
    gout = rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))
    hout = rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))
    if kind == "rotate":
        def call_gadget():
            rn.check(lib.rnt_ct_rotate(gout.c0.handle, gout.c1.handle, ct.c0.handle, ct.c1.handle, STEP,
                                       gk.a.handle, gk.b.handle))

        def call_hybrid():
            rn.check(lib.rnt_ct_rotate_hybrid(hout.c0.handle, hout.c1.handle, ct.c0.handle, ct.c1.handle, STEP,
                                              hk.a.handle, hk.b.handle, alpha))
    else:
        def call_gadget():
            rn.check(lib.rnt_ct_mul_relin(gout.c0.handle, gout.c1.handle, ct.c0.handle, ct.c1.handle, ctp.c0.handle,
                                          ctp.c1.handle, gk.a.handle, gk.b.handle))

        def call_hybrid():
            rn.check(lib.rnt_ct_mul_relin_hybrid(hout.c0.handle, hout.c1.handle, ct.c0.handle, ct.c1.handle,
                                                 ctp.c0.handle, ctp.c1.handle, hk.a.handle, hk.b.handle, alpha))

    tm = Timer(basis, a.warmup, a.repeats, a.window)
    (t_g, t_h), iters = tm.alternate([call_gadget, call_hybrid])
    s_g, s_h = tm.split(call_gadget), tm.split(call_hybrid)
    # each form against its own expected words, ciphertext 0
    Bc, Be = orc.Basis(primes[:L], 1 << log_n), orc.Basis(primes, 1 << log_n)
    x = [p.channels_of(0)[0] for p in (ct.c0, ct.c1, ctp.c0, ctp.c1)]
    ga, gb = gadget_host(gk)
    T = orc.host_threads()
    if kind == "rotate":
        w = rotate_hybrid_ref(Bc, Be, x[0], x[1], STEP, host[0], host[1], alpha)
        r = orc.rotate_ciphertext(Bc, x[0], x[1], STEP, ga, gb, threads=T)
    else:
        w = mul_relin_hybrid_ref(Bc, Be, *x, host[0], host[1], alpha)
        r = orc.mul_ciphertexts_gadget(Bc, *x, ga, gb, threads=T)
    return {"bench": kind, "log_n": log_n, "L": L, "K": alpha, "alpha": alpha, "bits": BITS, "batch": B,
            "iters": {"gadget": iters[0], "hybrid": iters[1]}, "gadget_ms": t_g, "hybrid_ms": t_h,
            "speedup_median": round(float(np.median(t_g) / np.median(t_h)), 3),
            "hybrid_matches_hybrid_ref": same(hout.c0, w[0]) and same(hout.c1, w[1]),
            "gadget_matches_oracle": same(gout.c0, r[0]) and same(gout.c1, r[1]),
            "gadget_kernels": s_g, "hybrid_kernels": s_h}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rotate", action="append", help="log_n,L,alpha,batch (repeatable)")
    ap.add_argument("--mul", action="append", help="log_n,L,alpha,batch (repeatable)")
    ap.add_argument("--no-rotate", action="store_true")
    ap.add_argument("--no-mul", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    parse = lambda items: [tuple(int(x) for x in s.split(",")) for s in items]  # noqa: E731
    rotate = parse(a.rotate) if a.rotate else ([] if a.no_rotate else ROTATE)
    mul = parse(a.mul) if a.mul else ([] if a.no_mul else MUL)
    bad = False
    for kind, shapes in (("rotate", rotate), ("mul", mul)):
        for sh in shapes:
            r = run(kind, *sh, a)
            bad = bad or not (r["hybrid_matches_hybrid_ref"] and r["gadget_matches_oracle"])
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            rn.pool_trim()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
