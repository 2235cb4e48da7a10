#!/usr/bin/env python3
"""A hybrid key's level view (RnsHybridKey.at_level / RnsHybridKeySet.at_level:
no copy, the full key's planes through a limb map) against the restricted key
on a fresh root (RnsHybridKey.restrict: a copy per level, its own tables), on
the same ciphertext words in one process on one GPU, at several levels of one
ring.  Calls: mul_ciphertexts_hybrid_rescale, and rotate_hoisted_hybrid with
eight steps.  The two forms are DEFINED to give the same words, which is
checked on every poly after the timing.

Timing as tools/bench_mul_rescale_hybrid.py: the two forms alternate; each
window is HIP events on the stream around enough back-to-back calls to last
`--window` seconds, after `--warmup` calls, `--repeats` windows each; then one
profiled call of each for the per-kernel split (rnt_profile_read).  One JSON
line per measurement on stdout and, with --out, appended to that file; every
line carries the key bytes resident on the device either way (the view: the
full key, once; the restricted form: this level's copy, and the sum of the
copies of every level L..1 a circuit would keep).

    python tools/bench_hybrid_levels.py --out profiles/hybrid_level_view_bench.jsonl
    python tools/bench_hybrid_levels.py --levels 16,3 --batch 1 --no-hoisted
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

bkh.KERNELS = tuple(dict.fromkeys(bkh.KERNELS + ("moddown_rescale", "rescale", "moddown_auto")))
LOG_N, L, ALPHA, BITS = 16, 16, 4, 31  # K = alpha
LEVELS = [16, 12, 8, 3]
BATCHES = [1, 64]
STEPS = [1, 2, 3, 4, 5, 6, 7, 8]


def equal(a, b):
    return bool(np.array_equal(a.channels_batch(), b.channels_batch()))


def key_planes(level, n_keys):
    """Planes of N words of n_keys hybrid keys (both halves) at a level."""
    return 2 * n_keys * -(-level // ALPHA) * (level + ALPHA)


class Ring:
    def __init__(self):
        n, K = 1 << LOG_N, ALPHA
        self.n, self.K = n, K
        self.primes = rn.generate_primes(BITS, L + K, n)
        self.ext = rn.RnsBasis(self.primes, n)
        self.rng = rn.DeviceRng(2033)
        beta = -(-L // ALPHA)
        u = lambda: rn.RnsPoly.sample_uniform(self.ext, self.rng, beta)  # noqa: E731
        self.rlk = rn.RnsHybridKey(u(), u(), ALPHA, None, n_special=K)
        self.rot = [rn.RnsHybridKey(u(), u(), ALPHA, s, n_special=K).prepare_hoisted() for s in STEPS]
        self.kset = rn.RnsHybridKeySet(self.rot, ALPHA)

    def sides(self, lv):
        """(ciphertext basis, relin key, hoisted set) of the view and of the
        restricted form at level lv."""
        view = (self.ext.drop_last(self.K + L - lv), self.rlk.at_level(lv), self.kset.at_level(lv))
        root = rn.RnsBasis(self.primes[:lv] + self.primes[L:], self.n)
        restricted = (root.drop_last(self.K), self.rlk.restrict(root),
                      rn.RnsHybridKeySet([k.restrict(root) for k in self.rot], ALPHA))
        return view, restricted


def run(ring, kind, lv, B, a):
    (vb, vkey, vset), (rb, rkey, rset) = ring.sides(lv)
    x = [rn.RnsPoly.sample_uniform(vb, ring.rng, B) for _ in range(4)]
    y = [rn.RnsPoly.from_channels(p.channels_batch(), rb) for p in x]  # the same words on the fresh root
    vct, vctp = rn.Ciphertext(x[0], x[1]), rn.Ciphertext(x[2], x[3])
    rct, rctp = rn.Ciphertext(y[0], y[1]), rn.Ciphertext(y[2], y[3])
    out = {}
    if kind == "mul_rescale":
        def call_view():
            out["v"] = rn.mul_ciphertexts_hybrid_rescale(vct, vctp, vkey)

        def call_restricted():
            out["r"] = rn.mul_ciphertexts_hybrid_rescale(rct, rctp, rkey)
        n_keys = 1
    else:
        vo = rn.Ciphertext(rn.RnsPoly(vb, len(STEPS) * B), rn.RnsPoly(vb, len(STEPS) * B))
        ro = rn.Ciphertext(rn.RnsPoly(rb, len(STEPS) * B), rn.RnsPoly(rb, len(STEPS) * B))

        def call_view():
            out["v"] = rn.rotate_ciphertext_hybrid_hoisted(vct, vset, out=vo)

        def call_restricted():
            out["r"] = rn.rotate_ciphertext_hybrid_hoisted(rct, rset, out=ro)
        n_keys = len(STEPS)
    if lv == 1 and kind == "mul_rescale":
        return None
    # the two forms run on two roots, so on two streams: each window is timed on its own
    tv, tr = Timer(vb, a.warmup, a.repeats, a.window), Timer(rb, a.warmup, a.repeats, a.window)
    for t, fn in ((tv, call_view), (tr, call_restricted)):
        for _ in range(a.warmup):
            fn()
        t.basis.sync()
    it_v = max(1, int(np.ceil(a.window * 1e3 / max(tv._window(call_view, 1), 1e-3))))
    it_r = max(1, int(np.ceil(a.window * 1e3 / max(tr._window(call_restricted, 1), 1e-3))))
    t_v, t_r = [], []
    for _ in range(a.repeats):
        t_v.append(round(tv._window(call_view, it_v), 4))
        t_r.append(round(tr._window(call_restricted, it_r), 4))
    s_v, s_r = tv.split(call_view), tr.split(call_restricted)
    wb, plane = 4, (1 << LOG_N)
    return {"bench": "hybrid_level_view", "call": kind, "log_n": LOG_N, "L": L, "K": ALPHA, "alpha": ALPHA,
            "bits": BITS, "level": lv, "gap": L - lv, "batch": B, "steps": len(STEPS) if kind == "hoisted" else 0,
            "iters": {"view": it_v, "restricted": it_r}, "view_ms": t_v, "restricted_ms": t_r,
            "view_over_restricted_median": round(float(np.median(t_v) / np.median(t_r)), 4),
            "view_equals_restricted": equal(out["v"].c0, out["r"].c0) and equal(out["v"].c1, out["r"].c1),
            "key_bytes": {"view_resident": key_planes(L, n_keys) * plane * wb,
                          "restricted_this_level": key_planes(lv, n_keys) * plane * wb,
                          "restricted_levels_L_to_1": sum(key_planes(v, n_keys) for v in range(1, L + 1)) * plane * wb},
            "view_kernels": s_v, "restricted_kernels": s_r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", help="comma-separated levels (default 16,12,8,3)")
    ap.add_argument("--batch", help="comma-separated batch sizes (default 1,64)")
    ap.add_argument("--no-mul", action="store_true")
    ap.add_argument("--no-hoisted", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    levels = [int(v) for v in a.levels.split(",")] if a.levels else LEVELS
    batches = [int(v) for v in a.batch.split(",")] if a.batch else BATCHES
    kinds = ([] if a.no_mul else ["mul_rescale"]) + ([] if a.no_hoisted else ["hoisted"])
    ring = Ring()
    bad = False
    for kind in kinds:
        for lv in levels:
            for B in batches:
                r = run(ring, kind, lv, B, a)
                if r is None:
                    continue
                bad = bad or not r["view_equals_restricted"]
                line = json.dumps(r)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                rn.pool_trim()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
