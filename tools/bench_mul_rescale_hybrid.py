#!/usr/bin/env python3
"""rnt_ct_mul_relin_rescale_hybrid against rnt_ct_mul_relin_hybrid followed by
rnt_ct_rescale, and rnt_ct_linear_bsgs_hybrid_rescale against
rnt_ct_linear_bsgs_hybrid followed by rnt_ct_rescale, on the same ciphertexts
in one process on one GPU.  The fused call is DEFINED as the composition, so
after the timing the two outputs are compared with each other on every poly and
ciphertext 0 of each with tests/hybrid_rescale_ref.py.

Timing as tools/bench_keyswitch_hybrid.py: the two forms alternate; each window
is HIP events on the basis' stream around enough back-to-back calls to last
`--window` seconds, after `--warmup` calls, `--repeats` windows each; then one
profiled call of each for the per-kernel split (rnt_profile_read).  One JSON
line per measurement on stdout and, with --out, appended to that file.

    python tools/bench_mul_rescale_hybrid.py --out profiles/mul_rescale_hybrid_bench.jsonl
    python tools/bench_mul_rescale_hybrid.py --mul 14,8,2,256 --no-bsgs
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
from bench_rotate_hybrid_hoisted import hybrid_keys, reupload  # noqa: E402

# (after the import above, which extends the list too)
bkh.KERNELS = tuple(dict.fromkeys(bkh.KERNELS + ("moddown_rescale", "rescale", "moddown_auto", "bsgs_mac")))
# log_n, L, alpha (= K), batch
MUL = [(14, 8, 2, 256), (16, 16, 4, 1), (16, 16, 4, 64)]
# log_n, L, alpha (= K), n_baby, n_giant, batch: 16 diagonals
BSGS = [(16, 16, 4, 4, 4, 64)]
BITS = 31


def equal(a, b):
    return bool(np.array_equal(a.channels(), b.channels()))


def same(p, w):
    return bool(np.array_equal(p.channels_of(0)[0], w))


def report(r, t_c, t_f, iters, s_c, s_f):
    r.update({"iters": {"composition": iters[0], "fused": iters[1]}, "composition_ms": t_c, "fused_ms": t_f,
              "speedup_median": round(float(np.median(t_c) / np.median(t_f)), 3),
              "composition_kernels": s_c, "fused_kernels": s_f})
    return r


def run_mul(log_n, L, alpha, B, a):
    import pyoracle as orc
    from hybrid_rescale_ref import mul_relin_rescale_hybrid_ref

    primes, basis, _, hk, host, (ct, ctp) = bkh.setup(log_n, L, alpha, B)
    lib = rn.load()
    low = basis.drop_last(1)
    mid = rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))
    cout = rn.Ciphertext(rn.RnsPoly(low, B), rn.RnsPoly(low, B))
    fout = rn.Ciphertext(rn.RnsPoly(low, B), rn.RnsPoly(low, B))
    ins = (ct.c0.handle, ct.c1.handle, ctp.c0.handle, ctp.c1.handle, hk.a.handle, hk.b.handle, alpha)

    def call_composition():
        rn.check(lib.rnt_ct_mul_relin_hybrid(mid.c0.handle, mid.c1.handle, *ins))
        rn.check(lib.rnt_ct_rescale(cout.c0.handle, cout.c1.handle, mid.c0.handle, mid.c1.handle))

    def call_fused():
        rn.check(lib.rnt_ct_mul_relin_rescale_hybrid(fout.c0.handle, fout.c1.handle, *ins))

    tm = Timer(basis, a.warmup, a.repeats, a.window)
    (t_c, t_f), iters = tm.alternate([call_composition, call_fused])
    s_c, s_f = tm.split(call_composition), tm.split(call_fused)
    Bc, Be = orc.Basis(primes[:L], 1 << log_n), orc.Basis(primes, 1 << log_n)
    x = [p.channels_of(0)[0] for p in (ct.c0, ct.c1, ctp.c0, ctp.c1)]
    w = mul_relin_rescale_hybrid_ref(Bc, Be, *x, host[0], host[1], alpha)
    r = {"bench": "mul_rescale_hybrid", "log_n": log_n, "L": L, "K": alpha, "alpha": alpha, "bits": BITS, "batch": B,
         "fused_equals_composition": equal(fout.c0, cout.c0) and equal(fout.c1, cout.c1),
         "fused_matches_ref": same(fout.c0, w[0]) and same(fout.c1, w[1]),
         "composition_matches_ref": same(cout.c0, w[0]) and same(cout.c1, w[1])}
    return report(r, t_c, t_f, iters, s_c, s_f)


def run_bsgs(log_n, L, alpha, n1, n2, B, a):
    import pyoracle as orc
    from hybrid_rescale_ref import bsgs_hybrid_rescale_ref

    n, K = 1 << log_n, alpha
    primes = rn.generate_primes(BITS, L + K, n)
    ext = rn.RnsBasis(primes, n)
    basis = ext.drop_last(K)
    low = basis.drop_last(1)
    rng = rn.DeviceRng(2031)
    beta = -(-L // alpha)
    baby, giant = list(range(n1)), [n1 * j for j in range(n2)]
    bhost, _ = hybrid_keys(ext, rng, beta, alpha, baby, False)
    ghost, gplain = hybrid_keys(ext, rng, beta, alpha, giant, False)
    bset = rn.RnsHybridKeySet(reupload(bhost, ext, alpha, baby, True), alpha)
    gset = rn.RnsHybridKeySet(gplain, alpha)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    diag = rn.RnsPoly.sample_uniform(basis, rng, n1 * n2)
    dhost = diag.channels()
    diag.to_ntt_domain()
    lib = rn.load()
    mid = rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))
    cout = rn.Ciphertext(rn.RnsPoly(low, B), rn.RnsPoly(low, B))
    fout = rn.Ciphertext(rn.RnsPoly(low, B), rn.RnsPoly(low, B))
    bs, gs = (ctypes.c_int32 * n1)(*baby), (ctypes.c_int32 * n2)(*giant)
    args = (ct.c0.handle, ct.c1.handle, bs, n1, gs, n2, diag.handle, bset.a.handle, bset.b.handle, gset.a.handle,
            gset.b.handle, alpha)

    def call_composition():
        rn.check(lib.rnt_ct_linear_bsgs_hybrid(mid.c0.handle, mid.c1.handle, *args))
        rn.check(lib.rnt_ct_rescale(cout.c0.handle, cout.c1.handle, mid.c0.handle, mid.c1.handle))

    def call_fused():
        rn.check(lib.rnt_ct_linear_bsgs_hybrid_rescale(fout.c0.handle, fout.c1.handle, *args))

    tm = Timer(basis, a.warmup, a.repeats, a.window)
    (t_c, t_f), iters = tm.alternate([call_composition, call_fused])
    s_c, s_f = tm.split(call_composition), tm.split(call_fused)
    Bc, Be = orc.Basis(primes[:L], n), orc.Basis(primes, n)
    x0, x1 = ct.c0.channels_of(0)[0], ct.c1.channels_of(0)[0]
    w = bsgs_hybrid_rescale_ref(Bc, Be, x0, x1, baby, giant, dhost, bhost, ghost, alpha)
    r = {"bench": "linear_bsgs_hybrid_rescale", "log_n": log_n, "L": L, "K": K, "alpha": alpha, "bits": BITS,
         "batch": B, "n_baby": n1, "n_giant": n2,
         "fused_equals_composition": equal(fout.c0, cout.c0) and equal(fout.c1, cout.c1),
         "fused_matches_ref": same(fout.c0, w[0]) and same(fout.c1, w[1]),
         "composition_matches_ref": same(cout.c0, w[0]) and same(cout.c1, w[1])}
    return report(r, t_c, t_f, iters, s_c, s_f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mul", action="append", help="log_n,L,alpha,batch (repeatable)")
    ap.add_argument("--bsgs", action="append", help="log_n,L,alpha,n_baby,n_giant,batch (repeatable)")
    ap.add_argument("--no-mul", action="store_true")
    ap.add_argument("--no-bsgs", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    parse = lambda items: [tuple(int(x) for x in s.split(",")) for s in items]  # noqa: E731
    mul = parse(a.mul) if a.mul else ([] if a.no_mul else MUL)
    bsgs = parse(a.bsgs) if a.bsgs else ([] if a.no_bsgs else BSGS)
    bad = False
    for fn, shapes in ((run_mul, mul), (run_bsgs, bsgs)):
        for sh in shapes:
            r = fn(*sh, a)
            bad = bad or not (r["fused_equals_composition"] and r["fused_matches_ref"] and r["composition_matches_ref"])
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            rn.pool_trim()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
