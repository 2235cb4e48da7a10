#!/usr/bin/env python3
"""CoeffToSlot / SlotToCoeff, rnt_mod_raise and rnt_mul_monomial timed in one
process on one GPU.

Ring: N = 2^16, 16 ciphertext primes of 30 bits and 2 special primes of 31
bits, alpha = 2.  Per depth (2, 3, 4) and direction the plan of
rns_ntt.homdft_plan is prepared on the top basis (the real diagonals) and run
with random hybrid keys of the right shape and form (timing does not read their
values) on random ciphertexts, for one ciphertext and for a batch of 8;
key-switches per transform are the plan's nonzero steps.  rnt_mod_raise from 1
and from 2 limbs onto the 16, and rnt_mul_monomial on 16 limbs, are timed next
to rnt_copy of the same 16 planes in the same run: the streaming yardstick (a
raise reads l0 planes and writes 16, a copy reads and writes 16).

Timing: HIP events on the basis' stream around `--iters` back-to-back calls
after `--warmup` calls, `--repeats` times; the median is reported.  One JSON
line per case on stdout and, with --out, appended to that file.

    python tools/bench_homdft.py --out profiles/homdft_bench.jsonl
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
from rns_ntt.engine import CkksEngine  # noqa: E402

LOG_N, L, K, ALPHA = 16, 16, 2, 2


def timer(basis, warmup, repeats):
    import torch

    stream = torch.cuda.ExternalStream(basis.stream())

    def timed(fn, iters):
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
        return float(np.median(res))

    return timed


def random_keyset(ext, rng, steps, beta, hoisted):
    keys = []
    for s in steps:
        if s == 0:
            keys.append(None)
            continue
        k = rn.RnsHybridKey(rn.RnsPoly.sample_uniform(ext, rng, beta), rn.RnsPoly.sample_uniform(ext, rng, beta),
                            ALPHA, rotation=s, n_special=K)
        k.hoisted = hoisted  # (random words serve as either form)
        keys.append(k)
    return rn.RnsHybridKeySet(keys, ALPHA)


def emit(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="2,3,4")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    n = 1 << LOG_N
    q, p = rn.generate_primes(30, L, n), rn.generate_primes(31, K, n)
    eng = CkksEngine(q, n, special_moduli=p)
    ext, top = eng.ext_basis, eng.basis
    rng = rn.DeviceRng(2026)
    timed = timer(top, a.warmup, a.repeats)
    beta = -(-L // ALPHA)
    # the streaming calls, next to rnt_copy of the same 16 planes
    for B in (1, 8):
        full = rn.RnsPoly.sample_uniform(top, rng, B)
        dst = rn.RnsPoly(top, B)
        copy_ms = timed(lambda: rn.check(rn.load().rnt_copy(dst.handle, full.handle)), 20)
        plane_bytes = B * n * 4
        line = {"case": "streaming", "log_n": LOG_N, "L": L, "batch": B, "copy_ms": round(copy_ms, 5),
                "copy_GBs": round(2 * L * plane_bytes / copy_ms / 1e6, 1)}
        for l0 in (1, 2):
            low = rn.RnsPoly.sample_uniform(top.drop_last(L - l0), rng, B)
            ms = timed(lambda: rn.check(rn.load().rnt_mod_raise(dst.handle, low.handle)), 20)
            line[f"mod_raise_from_{l0}_ms"] = round(ms, 5)
            line[f"mod_raise_from_{l0}_GBs"] = round((l0 + L) * plane_bytes / ms / 1e6, 1)
        for k in (n // 2, 1):
            ms = timed(lambda: rn.check(rn.load().rnt_mul_monomial(dst.handle, full.handle, k)), 20)
            line[f"mul_monomial_k{k}_ms"] = round(ms, 5)
            line[f"mul_monomial_k{k}_GBs"] = round(2 * L * plane_bytes / ms / 1e6, 1)
        emit(line, a.out)
    for depth in [int(d) for d in a.depths.split(",")]:
        for direction in ("coeff_to_slot", "slot_to_coeff"):
            plan = rn.homdft_plan(n, direction, depth)
            prepared = eng.prepare_homdft(plan, top)
            keysets = [(random_keyset(ext, rng, g.baby_steps, beta, True),
                        random_keyset(ext, rng, g.giant_steps, beta, False)) for g in plan.groups]
            run = eng.coeff_to_slot_hybrid if direction == "coeff_to_slot" else eng.slot_to_coeff_hybrid
            line = {"case": direction, "log_n": LOG_N, "L": L, "K": K, "alpha": ALPHA, "depth": depth,
                    "groups": [{"stages": len(g.stages), "diagonals": len(g.diags), "n_baby": len(g.baby_steps),
                                "n_giant": len(g.giant_steps)} for g in plan.groups],
                    "keyswitches": plan.n_keyswitches(), "iters": a.iters}
            for B in [int(b) for b in a.batches.split(",")]:
                ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(top, rng, B), rn.RnsPoly.sample_uniform(top, rng, B), 30,
                                   top.total_bits())
                line[f"ms_batch{B}"] = round(timed(lambda: run(ct, prepared, keysets), a.iters), 3)
                del ct
            emit(line, a.out)
            del prepared, keysets
            rn.pool_trim()
    return 0


if __name__ == "__main__":
    sys.exit(main())
