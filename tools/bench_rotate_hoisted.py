#!/usr/bin/env python3
"""rnt_ct_rotate_hoisted against a loop of rnt_ct_rotate on the same steps, and
rnt_ct_linear_bsgs_hoisted against rnt_ct_linear_bsgs on the same band, in one
process on one GPU.  The two forms of a rotation give different words by
definition, so each side is checked against its own expected result after the
timing: ciphertext 0 of the first step against tests/hoist_ref.py
(rotate_hoisted_ref) and against the oracle's rotate_ciphertext; the hoisted
BSGS call against the library's own composition (hoisted baby rotations,
coefficient-domain products, adds, giant rotations).

Timing: HIP events on the basis' stream around `--iters` back-to-back calls,
after `--warmup` calls, `--repeats` times; then one profiled call of each for
the per-kernel split (rnt_profile_read).  One JSON line per measurement on
stdout and, with --out, appended to that file.

    python tools/bench_rotate_hoisted.py --out profiles/rotate_hoisted_bench.jsonl
    python tools/bench_rotate_hoisted.py --rotate 16,16,31,64,8 --no-bsgs
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

KERNELS = ("hoist_digits", "hoist_mac", "automorphism", "ks_decompose", "ks_rows", "ks_whole", "bsgs_mac", "col_inv",
           "col_fwd", "row_fwd", "row_inv", "mf_ntt_fwd", "mf_ntt_inv", "whole_fwd", "whole_inv", "elementwise", "copy")
# log_n, L, bits, batch, n_steps, iters
ROTATE = [(16, 16, 31, 1, 8, 10), (16, 16, 31, 1, 1, 10), (16, 16, 31, 64, 8, 3), (16, 16, 31, 64, 1, 3),
          (17, 32, 31, 1, 8, 10), (17, 32, 31, 1, 1, 10)]
# log_n, L, bits, n1, n2, batch, iters: the rows of profiles/linear_bsgs_bench.jsonl
BSGS = [(16, 16, 31, 8, 8, 1, 10), (16, 16, 31, 4, 4, 64, 3), (17, 32, 31, 4, 4, 1, 10)]


def key_pair(basis, rng, k, keep_host=False):
    """The same random key channels in both forms: (ordinary, hoisting form,
    host copy of (a, b) or None)."""
    L = basis.channel_count()
    a, b = rn.RnsPoly.sample_uniform(basis, rng, L), rn.RnsPoly.sample_uniform(basis, rng, L)
    host = (a.channels(), b.channels()) if keep_host else None
    plain = rn.RnsGadgetKey(a.clone(), b.clone(), k)
    return plain, rn.RnsGadgetKey(a, b, k).prepare_hoisted(), host


class Timer:
    def __init__(self, basis, warmup, repeats):
        import torch

        self.torch, self.basis, self.warmup, self.repeats = torch, basis, warmup, repeats
        self.stream = torch.cuda.ExternalStream(basis.stream())

    def timed(self, fn, iters):
        torch = self.torch
        for _ in range(self.warmup):
            fn()
        self.basis.sync()
        res = []
        for _ in range(self.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(self.stream)
            for _ in range(iters):
                fn()
            b.record(self.stream)
            b.synchronize()
            res.append(round(a.elapsed_time(b) / iters, 4))
        return res

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


def run_rotate(log_n, L, bits, B, n_steps, iters, warmup, repeats):
    import pyoracle as orc
    from hoist_ref import rotate_hoisted_ref

    n = 1 << log_n
    mod = rn.generate_primes(bits, L, n)
    basis = rn.RnsBasis(mod, n)
    rng = rn.DeviceRng(2026)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    steps = list(range(1, n_steps + 1))
    plain, hoisted, host = [], [], None
    for t, k in enumerate(steps):
        p, h, hk = key_pair(basis, rng, k, keep_host=t == 0)
        plain.append(p)
        hoisted.append(h)
        host = host or hk
    hset = rn.RnsGadgetKeySet(hoisted, basis)
    hoisted.clear()
    lib = rn.load()
    hout = rn.Ciphertext(rn.RnsPoly(basis, n_steps * B), rn.RnsPoly(basis, n_steps * B))
    pout = [rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B)) for _ in steps]

    def call_hoisted():
        rn.rotate_ciphertext_hoisted(ct, hset, out=hout)

    def call_loop():
        for t, k in enumerate(steps):
            rn.check(lib.rnt_ct_rotate(pout[t].c0.handle, pout[t].c1.handle, ct.c0.handle, ct.c1.handle, k,
                                       plain[t].a.handle, plain[t].b.handle))

    tm = Timer(basis, warmup, repeats)
    t_loop = tm.timed(call_loop, iters)
    t_hoist = tm.timed(call_hoisted, iters)
    s_loop, s_hoist = tm.split(call_loop), tm.split(call_hoisted)
    # each side against its own expected result: ciphertext 0, the first step
    Bo = orc.Basis(mod, n)
    c0, c1 = ct.c0.channels_of(0)[0], ct.c1.channels_of(0)[0]
    w0, w1 = rotate_hoisted_ref(Bo, c0, c1, steps[0], host[0], host[1])
    ok_h = bool(np.array_equal(hout.c0.channels_of(0)[0], w0) and np.array_equal(hout.c1.channels_of(0)[0], w1))
    r0, r1 = orc.rotate_ciphertext(Bo, c0, c1, steps[0], host[0], host[1], threads=orc.host_threads())
    ok_p = bool(np.array_equal(pout[0].c0.channels_of(0)[0], r0) and np.array_equal(pout[0].c1.channels_of(0)[0], r1))
    return {"bench": "rotate", "log_n": log_n, "L": L, "bits": bits, "batch": B, "n_steps": n_steps, "iters": iters,
            "rotate_loop_ms": t_loop, "hoisted_ms": t_hoist,
            "speedup_median": round(float(np.median(t_loop) / np.median(t_hoist)), 3),
            "hoisted_matches_hoist_ref": ok_h, "rotate_matches_oracle": ok_p,
            "rotate_loop_kernels": s_loop, "hoisted_kernels": s_hoist}


def run_bsgs(log_n, L, bits, n1, n2, B, iters, warmup, repeats):
    n = 1 << log_n
    basis = rn.RnsBasis(rn.generate_primes(bits, L, n), n)
    rng = rn.DeviceRng(2027)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    baby, giant = list(range(n1)), [j * n1 for j in range(n2)]
    diag = rn.RnsPoly.sample_uniform(basis, rng, n1 * n2)
    bplain, bhoist = [], []
    for k in baby:
        p, h, _ = key_pair(basis, rng, k) if k else (None, None, None)
        bplain.append(p)
        bhoist.append(h)
    gkeys = [key_pair(basis, rng, k)[0] if k else None for k in giant]
    bset, hset, gset = (rn.RnsGadgetKeySet(x, basis) for x in (bplain, bhoist, gkeys))
    dn = diag.clone()
    dn.to_ntt_domain()
    out = rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))

    def call_plain():
        rn.linear_transform_bsgs(ct, dn, bset, gset, out=out)

    def call_hoisted():
        rn.linear_transform_bsgs_hoisted(ct, dn, hset, gset, out=out)

    tm = Timer(basis, warmup, repeats)
    t_plain = tm.timed(call_plain, iters)
    t_hoist = tm.timed(call_hoisted, iters)
    s_plain, s_hoist = tm.split(call_plain), tm.split(call_hoisted)
    # the hoisted call (in `out`) against the library's own composition
    rot = rn.rotate_ciphertext_hoisted(ct, hset)
    acc = None
    for j, g in enumerate(giant):
        v = None
        for i in range(n1):
            m = rn.RnsPoly(basis, B)
            for b in range(B):
                m.copy_polys(diag, b, j * n1 + i, 1)
            r0, r1 = rn.RnsPoly(basis, B), rn.RnsPoly(basis, B)
            r0.copy_polys(rot.c0, 0, i * B, B)
            r1.copy_polys(rot.c1, 0, i * B, B)
            p0, p1 = r0 * m, r1 * m
            v = (p0, p1) if v is None else (v[0] + p0, v[1] + p1)
        vc = rn.Ciphertext(v[0], v[1])
        r = vc if g == 0 else rn.rotate_ciphertext(vc, gkeys[j])
        acc = (r.c0, r.c1) if acc is None else (acc[0] + r.c0, acc[1] + r.c1)
    ok = bool(np.array_equal(out.c0.channels_of(0)[0], acc[0].channels_of(0)[0]) and
              np.array_equal(out.c1.channels_of(B - 1)[0], acc[1].channels_of(B - 1)[0]))
    return {"bench": "bsgs", "log_n": log_n, "L": L, "bits": bits, "n_baby": n1, "n_giant": n2,
            "diagonals": n1 * n2, "batch": B, "iters": iters, "bsgs_ms": t_plain, "bsgs_hoisted_ms": t_hoist,
            "speedup_median": round(float(np.median(t_plain) / np.median(t_hoist)), 3),
            "hoisted_matches_composition": ok, "bsgs_kernels": s_plain, "bsgs_hoisted_kernels": s_hoist}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rotate", action="append", help="log_n,L,bits,batch,n_steps[,iters] (repeatable)")
    ap.add_argument("--bsgs", action="append", help="log_n,L,bits,n_baby,n_giant,batch[,iters] (repeatable)")
    ap.add_argument("--no-rotate", action="store_true")
    ap.add_argument("--no-bsgs", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()

    def parse(items, full):
        out = []
        for s in items:
            v = [int(x) for x in s.split(",")]
            out.append(tuple(v) if len(v) == full else tuple(v) + (10,))
        return out

    rotate = parse(a.rotate, 6) if a.rotate else ([] if a.no_rotate else ROTATE)
    bsgs = parse(a.bsgs, 7) if a.bsgs else ([] if a.no_bsgs else BSGS)
    bad = False
    for fn, shapes in ((run_rotate, rotate), (run_bsgs, bsgs)):
        for sh in shapes:
            r = fn(*sh, a.warmup, a.repeats)
            bad = bad or not all(v for k, v in r.items() if k.startswith(("hoisted_matches", "rotate_matches")))
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            rn.pool_trim()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
