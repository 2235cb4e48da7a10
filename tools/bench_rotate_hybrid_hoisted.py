#!/usr/bin/env python3
"""rnt_ct_rotate_hybrid_hoisted against a loop of rnt_ct_rotate_hybrid, and
rnt_ct_linear_bsgs_hybrid against the same sum composed from
rnt_ct_rotate_hybrid, rnt_mul and rnt_add (with rnt_ct_linear_bsgs_hoisted on
gadget keys beside it for context), on the same ciphertexts in one process on
one GPU.  The forms give different words by definition, so after the timing
ciphertext 0 of each new call is checked against its own reference
(tests/hybrid_hoist_ref.py) and the loop against tests/hybrid_ref.py.

Timing is tools/bench_keyswitch_hybrid.py's: the forms alternate; each window is
HIP events on the basis' stream around enough back-to-back calls to last
`--window` seconds, after `--warmup` calls, `--repeats` windows each; then one
profiled call of each for the per-kernel split (rnt_profile_read).  The form
"hoisted_unfused" is the hoisted call on a context created with
RNT_MODDOWN_AUTO=0 (k_moddown, the automorphism launch and a strided copy in
place of k_moddown_auto), timed in windows of its own right after the other
two, and with --tail fused (the default of this tool) "hoisted" and
"bsgs_hybrid" run on one created with RNT_MODDOWN_AUTO=2 (k_moddown_auto at
every size): the A/B of the per-step tail, from which the library's default
takes the faster one per chunk size; --tail default measures that choice.  One JSON line per
measurement on stdout and, with --out, appended to that file.

    python tools/bench_rotate_hybrid_hoisted.py --out profiles/rotate_hybrid_hoisted_bench.jsonl
    python tools/bench_rotate_hybrid_hoisted.py --rotate 14,8,2,4,8 --no-bsgs
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
from bench_keyswitch_hybrid import Timer  # noqa: E402
import bench_keyswitch_hybrid as bkh  # noqa: E402

bkh.KERNELS = bkh.KERNELS + ("moddown_auto", "bsgs_mac", "hoist_digits")
# log_n, L, alpha (= K), batch, steps
ROTATE = [(16, 16, 4, 1, 1), (16, 16, 4, 1, 8), (16, 16, 4, 64, 1), (16, 16, 4, 64, 8), (17, 32, 8, 1, 1),
          (17, 32, 8, 1, 8)]
# log_n, L, alpha (= K), n_baby, n_giant, batch: the shapes of profiles/linear_bsgs_bench.jsonl
BSGS = [(16, 16, 4, 8, 8, 1), (16, 16, 4, 4, 4, 64), (17, 32, 8, 4, 4, 1)]
BITS = 31
# --tail: the per-step tail of the form under test ("hoisted", "bsgs_hybrid")
TAILS = {"fused": "2", "default": "1"}


def hybrid_keys(ext, rng, beta, alpha, steps, hoisted):
    """Uniform key channels per nonzero step: (host channels, RnsHybridKey)."""
    host, keys = [], []
    for k in steps:
        if k == 0:
            host.append(None)
            keys.append(None)
            continue
        a, b = rn.RnsPoly.sample_uniform(ext, rng, beta), rn.RnsPoly.sample_uniform(ext, rng, beta)
        host.append((a.channels(), b.channels()))
        key = rn.RnsHybridKey(a, b, alpha, k)
        keys.append(key.prepare_hoisted() if hoisted else key)
    return host, keys


def reupload(keys_host, ext, alpha, steps, hoisted):
    out = []
    for k, kk in zip(steps, keys_host):
        key = None if kk is None else rn.RnsHybridKey.from_channels(kk[0], kk[1], ext, alpha, rotation=k)
        out.append(key.prepare_hoisted() if key is not None and hoisted else key)
    return out


def run_rotate(log_n, L, alpha, B, n_steps, a):
    import pyoracle as orc
    from hybrid_hoist_ref import rotate_hybrid_hoisted_ref
    from hybrid_ref import rotate_hybrid_ref

    n, K = 1 << log_n, alpha
    primes = rn.generate_primes(BITS, L + K, n)
    os.environ["RNT_MODDOWN_AUTO"] = TAILS[a.tail]  # read at rnt_ctx_create
    ext = rn.RnsBasis(primes, n)
    basis = ext.drop_last(K)
    rng = rn.DeviceRng(2029)
    beta = -(-L // alpha)
    steps = [1, 2, 3, 5, 7, 11, 13, 17][:n_steps]
    host, plain = hybrid_keys(ext, rng, beta, alpha, steps, False)
    kset = rn.RnsHybridKeySet(reupload(host, ext, alpha, steps, True), alpha)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    os.environ["RNT_MODDOWN_AUTO"] = "0"  # read at rnt_ctx_create
    ext_u = rn.RnsBasis(primes, n)
    del os.environ["RNT_MODDOWN_AUTO"]
    basis_u = ext_u.drop_last(K)  # (its own stream and its own Timer: a context must outlive its stream's users)
    kset_u = rn.RnsHybridKeySet(reupload(host, ext_u, alpha, steps, True), alpha)
    x0, x1 = ct.c0.channels_of(0)[0], ct.c1.channels_of(0)[0]
    ct_u = rn.Ciphertext(rn.RnsPoly.from_channels(ct.c0.channels(), basis_u),
                         rn.RnsPoly.from_channels(ct.c1.channels(), basis_u))
    lib = rn.load()
    louts = [rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B)) for _ in steps]
    hout = rn.Ciphertext(rn.RnsPoly(basis, n_steps * B), rn.RnsPoly(basis, n_steps * B))
    uout = rn.Ciphertext(rn.RnsPoly(basis_u, n_steps * B), rn.RnsPoly(basis_u, n_steps * B))

    def call_loop():
        for o, k, key in zip(louts, steps, plain):
            rn.check(lib.rnt_ct_rotate_hybrid(o.c0.handle, o.c1.handle, ct.c0.handle, ct.c1.handle, k, key.a.handle,
                                              key.b.handle, alpha))

    def call_hoisted():
        rn.rotate_ciphertext_hybrid_hoisted(ct, kset, out=hout)

    def call_unfused():
        rn.rotate_ciphertext_hybrid_hoisted(ct_u, kset_u, out=uout)

    tm, tm_u = Timer(basis, a.warmup, a.repeats, a.window), Timer(basis_u, a.warmup, a.repeats, a.window)
    (t_l, t_h), iters = tm.alternate([call_loop, call_hoisted])
    (t_u,), iters_u = tm_u.alternate([call_unfused])
    iters = iters + iters_u
    s_l, s_h, s_u = tm.split(call_loop), tm.split(call_hoisted), tm_u.split(call_unfused)
    basis.sync()
    basis_u.sync()
    Bc, Be = orc.Basis(primes[:L], n), orc.Basis(primes, n)
    t = n_steps - 1
    w = rotate_hybrid_hoisted_ref(Bc, Be, x0, x1, steps[t], host[t][0], host[t][1], alpha)
    r = rotate_hybrid_ref(Bc, Be, x0, x1, steps[t], host[t][0], host[t][1], alpha)
    same = lambda p, i, v: bool(np.array_equal(p.channels_of(i)[0], v))  # noqa: E731
    return {"bench": "rotate_hybrid_hoisted", "tail": a.tail, "log_n": log_n, "L": L, "K": K, "alpha": alpha, "bits": BITS, "batch": B,
            "steps": n_steps, "iters": dict(zip(("loop", "hoisted", "hoisted_unfused"), iters)),
            "loop_ms": t_l, "hoisted_ms": t_h, "hoisted_unfused_ms": t_u,
            "speedup_median": round(float(np.median(t_l) / np.median(t_h)), 3),
            "fused_tail_speedup_median": round(float(np.median(t_u) / np.median(t_h)), 3),
            "hoisted_matches_ref": same(hout.c0, t * B, w[0]) and same(hout.c1, t * B, w[1]),
            "unfused_matches_ref": same(uout.c0, t * B, w[0]) and same(uout.c1, t * B, w[1]),
            "loop_matches_hybrid_ref": same(louts[t].c0, 0, r[0]) and same(louts[t].c1, 0, r[1]),
            "loop_kernels": s_l, "hoisted_kernels": s_h, "hoisted_unfused_kernels": s_u}


def run_bsgs(log_n, L, alpha, n1, n2, B, a):
    import pyoracle as orc
    from hybrid_hoist_ref import bsgs_hybrid_ref

    n, K = 1 << log_n, alpha
    primes = rn.generate_primes(BITS, L + K, n)
    os.environ["RNT_MODDOWN_AUTO"] = TAILS[a.tail]  # read at rnt_ctx_create
    ext = rn.RnsBasis(primes, n)
    basis = ext.drop_last(K)
    rng = rn.DeviceRng(2030)
    beta = -(-L // alpha)
    baby, giant = list(range(n1)), [n1 * j for j in range(n2)]
    bhost, bplain = hybrid_keys(ext, rng, beta, alpha, baby, False)
    ghost, gplain = hybrid_keys(ext, rng, beta, alpha, giant, False)
    bset = rn.RnsHybridKeySet(reupload(bhost, ext, alpha, baby, True), alpha)
    gset = rn.RnsHybridKeySet(gplain, alpha)
    ct = rn.Ciphertext(rn.RnsPoly.sample_uniform(basis, rng, B), rn.RnsPoly.sample_uniform(basis, rng, B))
    diag = rn.RnsPoly.sample_uniform(basis, rng, n1 * n2)
    dhost = diag.channels()
    dntt = diag.clone()
    dntt.to_ntt_domain()
    # the composition: every diagonal broadcast over the batch for rnt_mul
    dB = []
    for t in range(n1 * n2):
        d = rn.RnsPoly(basis, B)
        for p in range(B):
            d.copy_polys(diag, p, t, 1)
        dB.append(d)
    lib = rn.load()
    new = lambda: rn.Ciphertext(rn.RnsPoly(basis, B), rn.RnsPoly(basis, B))  # noqa: E731
    R = [ct if b == 0 else new() for b in baby]
    V, T, G, acc = new(), new(), new(), new()
    hout = new()

    def rot(o, c, k, key):
        rn.check(lib.rnt_ct_rotate_hybrid(o.c0.handle, o.c1.handle, c.c0.handle, c.c1.handle, k, key.a.handle,
                                          key.b.handle, alpha))

    def call_composed():
        for r, b, key in zip(R, baby, bplain):
            if b:
                rot(r, ct, b, key)
        for j, g in enumerate(giant):
            for i in range(n1):
                dst = V if i == 0 else T
                for o, x in ((dst.c0, R[i].c0), (dst.c1, R[i].c1)):
                    rn.check(lib.rnt_mul(o.handle, x.handle, dB[j * n1 + i].handle))
                if i:
                    V.c0 += T.c0
                    V.c1 += T.c1
            src = V
            if g:
                rot(G, V, g, gplain[j])
                src = G
            if j == 0:
                rn.check(lib.rnt_copy(acc.c0.handle, src.c0.handle))
                rn.check(lib.rnt_copy(acc.c1.handle, src.c1.handle))
            else:
                acc.c0 += src.c0
                acc.c1 += src.c1

    def call_hybrid():
        rn.linear_transform_bsgs_hybrid(ct, dntt, bset, gset, out=hout)

    fns, names = [call_composed, call_hybrid], ["composed", "bsgs_hybrid"]
    # context: the gadget call on the same ring (its own keys, 2^58-scale pipelines)
    gk = lambda steps, hoisted: rn.RnsGadgetKeySet([  # noqa: E731
        None if k == 0 else (lambda key: key.prepare_hoisted() if hoisted else key)(
            rn.RnsGadgetKey(rn.RnsPoly.sample_uniform(basis, rng, L), rn.RnsPoly.sample_uniform(basis, rng, L), k))
        for k in steps], basis)
    gb, gg = gk(baby, True), gk(giant, False)
    gout = new()
    fns.append(lambda: rn.linear_transform_bsgs_hoisted(ct, dntt, gb, gg, out=gout))
    names.append("gadget_bsgs_hoisted")
    tm = Timer(basis, a.warmup, a.repeats, a.window)
    res, iters = tm.alternate(fns)
    splits = {nm: tm.split(fn) for nm, fn in zip(names, fns)}
    Bc, Be = orc.Basis(primes[:L], n), orc.Basis(primes, n)
    x0, x1 = ct.c0.channels_of(0)[0], ct.c1.channels_of(0)[0]
    w = bsgs_hybrid_ref(Bc, Be, x0, x1, baby, giant, dhost, bhost, ghost, alpha)
    ok = bool(np.array_equal(hout.c0.channels_of(0)[0], w[0]) and np.array_equal(hout.c1.channels_of(0)[0], w[1]))
    out = {"bench": "linear_bsgs_hybrid", "tail": a.tail, "log_n": log_n, "L": L, "K": K, "alpha": alpha, "bits": BITS, "batch": B,
           "n_baby": n1, "n_giant": n2, "iters": dict(zip(names, iters))}
    for nm, t in zip(names, res):
        out[nm + "_ms"] = t
    out["speedup_median"] = round(float(np.median(res[0]) / np.median(res[1])), 3)
    out["bsgs_hybrid_matches_ref"] = ok
    out["kernels"] = splits
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rotate", action="append", help="log_n,L,alpha,batch,steps (repeatable)")
    ap.add_argument("--bsgs", action="append", help="log_n,L,alpha,n_baby,n_giant,batch (repeatable)")
    ap.add_argument("--no-rotate", action="store_true")
    ap.add_argument("--no-bsgs", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--tail", choices=sorted(TAILS), default="fused",
                    help="fused: k_moddown_auto at every size (the A/B); default: the library's choice by chunk size")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    parse = lambda items: [tuple(int(x) for x in s.split(",")) for s in items]  # noqa: E731
    rotate = parse(a.rotate) if a.rotate else ([] if a.no_rotate else ROTATE)
    bsgs = parse(a.bsgs) if a.bsgs else ([] if a.no_bsgs else BSGS)
    bad = False
    for fn, shapes in ((run_rotate, rotate), (run_bsgs, bsgs)):
        for sh in shapes:
            r = fn(*sh, a)
            bad = bad or not all(v for k, v in r.items() if k.endswith("_ref"))
            line = json.dumps(r)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            rn.pool_trim()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
