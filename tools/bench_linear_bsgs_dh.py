#!/usr/bin/env python3
"""rnt_ct_linear_bsgs_hybrid_dh against rnt_ct_linear_bsgs_hybrid on the same
ciphertexts, keys and diagonals, in one process on one GPU; then CoeffToSlot /
SlotToCoeff through either call.  The two give different words by definition,
so after the timing ciphertext 0 of the double-hoisted call is checked against
its own reference (tests/dh_bsgs_ref.py).

Timing is tools/bench_rotate_hybrid_hoisted.py's: the forms alternate; each
window is HIP events on the basis' stream around enough back-to-back calls to
last `--window` seconds, after `--warmup` calls, `--repeats` windows each; then
one profiled call of each for the per-kernel split (rnt_profile_read).  The
shapes are that tool's BSGS rows (alpha = K); the transforms run
tools/bench_homdft.py's ring (N = 2^16, 16 x 30-bit + 2 x 31-bit, alpha = 2)
with random keys of the right shape on random ciphertexts, the real diagonals
encoded over Q (today's call) and over Q_l u P (the double-hoisted one).  One
JSON line per measurement on stdout and, with --out, appended to that file.

    python tools/bench_linear_bsgs_dh.py --out profiles/linear_bsgs_dh_bench.jsonl
    python tools/bench_linear_bsgs_dh.py --bsgs 14,8,2,4,4,2 --no-homdft --no-check
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
from bench_homdft import random_keyset  # noqa: E402
from bench_keyswitch_hybrid import Timer  # noqa: E402
from bench_rotate_hybrid_hoisted import BSGS, hybrid_keys, reupload  # noqa: E402
from rns_ntt.engine import CkksEngine  # noqa: E402

bkh.KERNELS = bkh.KERNELS + ("moddown_auto", "moddown_rescale", "bsgs_mac", "dh_bsgs_mac", "dh_bsgs_fold")
BITS = 31
H_LOG_N, H_L, H_K, H_ALPHA = 16, 16, 2, 2  # tools/bench_homdft.py's ring


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def run_bsgs(log_n, L, alpha, n1, n2, B, a):
    n, K = 1 << log_n, alpha
    primes = rn.generate_primes(BITS, L + K, n)
    ext = rn.RnsBasis(primes, n)
    basis = ext.drop_last(K)
    rng = rn.DeviceRng(2031)
    beta = -(-L // alpha)
    baby, giant = list(range(n1)), [n1 * j for j in range(n2)]
    bhost, _ = hybrid_keys(ext, rng, beta, alpha, baby, False)
    ghost, gplain = hybrid_keys(ext, rng, beta, alpha, giant, False)
    bset = rn.RnsHybridKeySet(reupload(bhost, ext, alpha, baby, True), alpha)
    gset = rn.RnsHybridKeySet(gplain, alpha)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    dE = rn.RnsPoly.sample_uniform(ext, rng, n1 * n2)  # uniform words over E; today's call reads the q-limbs
    dhost = dE.channels()
    dC = rn.RnsPoly.from_channels(np.ascontiguousarray(dhost[:, :L, :]), basis)
    dE.to_ntt_domain()
    dC.to_ntt_domain()
    new = lambda: rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))  # noqa: E731
    hout, dout = new(), new()

    def call_hybrid():
        rn.linear_transform_bsgs_hybrid(ct, dC, bset, gset, out=hout)

    def call_dh():
        rn.linear_bsgs_hybrid_dh(ct, dE, bset, gset, out=dout)

    fns, names = [call_hybrid, call_dh], ["bsgs_hybrid", "bsgs_hybrid_dh"]
    tm = Timer(basis, a.warmup, a.repeats, a.window)
    res, iters = tm.alternate(fns)
    splits = {nm: tm.split(fn) for nm, fn in zip(names, fns)}
    out = {"bench": "linear_bsgs_hybrid_dh", "log_n": log_n, "L": L, "K": K, "alpha": alpha, "bits": BITS, "batch": B,
           "n_baby": n1, "n_giant": n2, "iters": dict(zip(names, iters))}
    for nm, t in zip(names, res):
        out[nm + "_ms"] = t
    out["speedup_median"] = round(float(np.median(res[0]) / np.median(res[1])), 3)
    if not a.no_check:
        import pyoracle as orc
        from concurrent.futures import ThreadPoolExecutor
        from dh_bsgs_ref import dh_bsgs_ref

        Bc, Be = orc.Basis(primes[:L], n), orc.Basis(primes, n)
        x0, x1 = ct.c0.channels_of(0)[0], ct.c1.channels_of(0)[0]
        with ThreadPoolExecutor(8) as pool:
            w = dh_bsgs_ref(Bc, Be, x0, x1, baby, giant, dhost, bhost, ghost, alpha, pmap=pool.map)
        out["bsgs_hybrid_dh_matches_ref"] = bool(np.array_equal(dout.c0.channels_of(0)[0], w[0]) and
                                                 np.array_equal(dout.c1.channels_of(0)[0], w[1]))
    out["kernels"] = splits
    return out


def run_homdft(a, out_path):
    n = 1 << H_LOG_N
    q, p = rn.generate_primes(30, H_L, n), rn.generate_primes(31, H_K, n)
    eng = CkksEngine(q, n, special_moduli=p)
    ext, top = eng.ext_basis, eng.basis
    rng = rn.DeviceRng(2032)
    beta = -(-H_L // H_ALPHA)
    tm = Timer(top, a.warmup, a.repeats, a.window)
    for depth in [int(d) for d in a.depths.split(",")]:
        for direction in ("coeff_to_slot", "slot_to_coeff"):
            plan = rn.homdft_plan(n, direction, depth)
            old, new = eng.prepare_homdft(plan, top), eng.prepare_homdft_dh(plan, top)
            keysets = [(random_keyset(ext, rng, g.baby_steps, beta, True),
                        random_keyset(ext, rng, g.giant_steps, beta, False)) for g in plan.groups]
            c2s = direction == "coeff_to_slot"
            run_old = eng.coeff_to_slot_hybrid if c2s else eng.slot_to_coeff_hybrid
            run_new = eng.coeff_to_slot_hybrid_dh if c2s else eng.slot_to_coeff_hybrid_dh
            line = {"bench": "homdft_dh", "case": direction, "log_n": H_LOG_N, "L": H_L, "K": H_K, "alpha": H_ALPHA,
                    "depth": depth,
                    "groups": [{"diagonals": len(g.diags), "n_baby": len(g.baby_steps), "n_giant": len(g.giant_steps)}
                               for g in plan.groups], "keyswitches": plan.n_keyswitches()}
            for B in [int(b) for b in a.batches.split(",")]:
                ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(top, rng, B), rn.RnsPoly.sample_uniform(top, rng, B), 30,
                                   top.total_bits())
                fns = [lambda: run_old(ct, old, keysets), lambda: run_new(ct, new, keysets)]
                res, iters = tm.alternate(fns)
                line[f"hybrid_ms_batch{B}"], line[f"dh_ms_batch{B}"] = res
                line[f"iters_batch{B}"] = iters
                line[f"speedup_median_batch{B}"] = round(float(np.median(res[0]) / np.median(res[1])), 3)
                if B == 1:
                    line["kernels"] = {"hybrid": tm.split(fns[0]), "dh": tm.split(fns[1])}
                del ct
            emit(line, out_path)
            del old, new, keysets
            rn.pool_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bsgs", action="append", help="log_n,L,alpha,n_baby,n_giant,batch (repeatable)")
    ap.add_argument("--no-bsgs", action="store_true")
    ap.add_argument("--no-homdft", action="store_true")
    ap.add_argument("--no-check", action="store_true", help="skip the CPU reference of ciphertext 0")
    ap.add_argument("--depths", default="2,3,4")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.bsgs] if a.bsgs else ([] if a.no_bsgs else BSGS)
    bad = False
    for sh in shapes:
        r = run_bsgs(*sh, a)
        bad = bad or not all(v for k, v in r.items() if k.endswith("_ref"))
        emit(r, a.out)
        rn.pool_trim()
    if not a.no_homdft:
        run_homdft(a, a.out)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
