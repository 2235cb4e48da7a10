#!/usr/bin/env python3
"""Inner sums over slots: rnt_ct_rotsum_hybrid stage by stage (rotsum_plan at
radix 2, 4, 8 and 16) against the chain of rnt_ct_rotate_hybrid and rnt_add the
library offered before, on the same ciphertexts in one process on one GPU.

Ring: N = 2^16, 16 x 30-bit limbs + 2 special primes, alpha = 2 (beta = 8; a key
is 2 beta (16 + 2) planes = 72 MiB of 32-bit words).  Sweep: n in {8, 64, 1024}
slots summed, B in {1, 8, 64} ciphertexts.  The chain is the logarithmic one --
acc += rotate(acc, 2^i) for i < log2 n, the fewest rotations the old calls need
-- and reads the keys of the radix-2 plan.  Keys are uniform polys (timing does
not depend on their values), one per distinct step, shared by every form.

Timing is tools/bench_keyswitch_hybrid.py's Timer: the forms alternate; each
window is HIP events on the basis' stream around enough back-to-back calls to
last `--window` seconds, after `--warmup` calls, `--repeats` windows each; then
one profiled call of each for the launch counts (rnt_profile_read).  One JSON
line per point on stdout and, with --out, appended to that file.

    python tools/bench_rotsum.py --out profiles/rotsum_bench.jsonl
    python tools/bench_rotsum.py --n 8,64 --batch 1 --radix 2,4
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("toy-heaan-ckks_amd", "tools"):
    sys.path.insert(0, os.path.join(REPO, p))

import numpy as np  # noqa: E402

import rns_ntt as rn  # noqa: E402
import bench_keyswitch_hybrid as bkh  # noqa: E402
from bench_keyswitch_hybrid import Timer  # noqa: E402

bkh.KERNELS = tuple(rn._lib.PROFILE_NAMES)
LOG_N, L, K, ALPHA = 16, 16, 2, 2


class Ring:
    def __init__(self):
        n = 1 << LOG_N
        self.primes = rn.generate_primes(30, L, n) + rn.generate_primes(31, K, n)
        self.ext = rn.RnsBasis(self.primes, n)
        self.basis = self.ext.drop_last(K)
        self.rng = rn.DeviceRng(2031)
        self.beta = -(-L // ALPHA)
        self.keys = {}
        self.sets = {}
        self.key_bytes = 2 * self.beta * (L + K) * n * 4

    def key(self, step):
        if step not in self.keys:
            a = rn.RnsPoly.sample_uniform(self.ext, self.rng, self.beta)
            b = rn.RnsPoly.sample_uniform(self.ext, self.rng, self.beta)
            self.keys[step] = rn.RnsHybridKey(a, b, ALPHA, step)
        return self.keys[step]

    def keyset(self, steps):
        steps = tuple(steps)
        if steps not in self.sets:
            self.sets[steps] = rn.RnsHybridKeySet([None if s == 0 else self.key(s) for s in steps], ALPHA)
        return self.sets[steps]


def run_point(ring, n, B, radices, a):
    basis, lib = ring.basis, rn.load()
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, ring.rng, B), rn.RnsPoly.sample_uniform(basis, ring.rng, B))
    new = lambda: rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))  # noqa: E731
    acc, rot = new(), new()
    chain_steps = [1 << i for i in range(n.bit_length() - 1)]
    chain_keys = [ring.key(s) for s in chain_steps]

    def call_chain():
        src = ct
        for s, key in zip(chain_steps, chain_keys):
            rn.check(lib.rnt_ct_rotate_hybrid(rot.c0.handle, rot.c1.handle, src.c0.handle, src.c1.handle, s,
                                              key.a.handle, key.b.handle, ALPHA))
            rn.check(lib.rnt_add(acc.c0.handle, src.c0.handle, rot.c0.handle))
            rn.check(lib.rnt_add(acc.c1.handle, src.c1.handle, rot.c1.handle))
            src = acc

    plans, fns, names = {}, [call_chain], ["chain"]
    for r in radices:
        if r > n:
            continue
        plan = rn.rotsum_plan(n, 1, r)
        sets = [ring.keyset(st) for st in plan.stages]
        out = new()

        def call(sets=sets, out=out):
            src = ct
            for ks in sets:
                rn.rotsum_ciphertext_hybrid(src, ks, out=out)
                src = out

        plans[r] = plan
        fns.append(call)
        names.append(f"radix{r}")
    tm = Timer(basis, a.warmup, a.repeats, a.window)
    res, iters = tm.alternate(fns)
    splits = [tm.split(fn) for fn in fns]
    basis.sync()
    res_out = {"bench": "rotsum", "log_n": LOG_N, "L": L, "K": K, "alpha": ALPHA, "n": n, "batch": B,
               "key_mib": ring.key_bytes / 2 ** 20, "iters": dict(zip(names, iters))}
    chain_med = float(np.median(res[0]))
    for nm, t, sp in zip(names, res, splits):
        r = None if nm == "chain" else int(nm[5:])
        n_keys = len(chain_steps) if r is None else len(plans[r].all_steps)
        res_out[nm] = {"ms": t, "median_ms": round(float(np.median(t)), 4),
                       "vs_chain": round(chain_med / float(np.median(t)), 3),
                       "launches": int(sum(v["launches"] for v in sp.values())),
                       "keys": n_keys, "key_mib_resident": n_keys * ring.key_bytes / 2 ** 20,
                       "stages": None if r is None else plans[r].radices, "kernels": sp}
    return res_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="8,64,1024")
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--radix", default="2,4,8,16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",")]  # noqa: E731
    ring = Ring()
    for B in ints(a.batch):
        for n in ints(a.n):
            line = json.dumps(run_point(ring, n, B, ints(a.radix), a))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        rn.pool_trim()
    return 0


if __name__ == "__main__":
    sys.exit(main())
