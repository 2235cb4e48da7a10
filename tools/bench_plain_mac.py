#!/usr/bin/env python3
"""The ciphertext x plaintext multiply-accumulate at N = 2^16 with 16 x 30-bit
primes, in one process on one GPU: rnt_ct_plain_mac_rescale on n_terms packed
ciphertexts against the composition it replaces -- per term one rnt_mul of
either component with the plaintext in the coefficient domain and, from the
second term on, one rnt_add of either, then rnt_ct_rescale -- on the same
inputs (the composition reads per-term copies and coefficient-domain plaintexts
made before the timing, so it pays no transform of the plaintext that the
library's rnt_mul does not pay), for n_terms in {1, 4, 16}, B in {1, 8, 64}
ciphertexts and plaintexts shared by the batch or one per ciphertext.  The words
of both are compared once per shape before the timing.

Timing as tools/bench_keyswitch_hybrid.py: HIP events on the basis' stream
around enough back-to-back calls to last `--window` seconds, after `--warmup`
calls, `--repeats` windows, the two forms taken in turn.  One JSON line per
shape with the per-kernel split of one profiled run of either form
(rnt_profile_read) and the ratio of the medians, on stdout and, with --out,
appended to that file.

    python tools/bench_plain_mac.py --out profiles/plain_mac_bench.jsonl
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
from bench_ct_dot_hybrid import clock_mhz  # noqa: E402
from bench_keyswitch_hybrid import Timer  # noqa: E402

bkh.KERNELS = tuple(dict.fromkeys(bkh.KERNELS + ("plain_mac", "rescale", "mf_mul", "plane_fused", "row_mul",
                                                 "whole_mul")))
LOG_N, L, KPLAIN_T = 16, 16, 16


def emit(r, out):
    r.update({"log_n": LOG_N, "L": L, "bits": 30, "sclk_mhz": clock_mhz()})
    line = json.dumps(r)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def run(basis, n_terms, B, shared, a, out):
    n, word = 1 << LOG_N, 4
    rng = rn.DeviceRng(5100 + 100 * n_terms + B + (7 if shared else 0))
    lib = rn.load()
    low = basis.drop_last(1)
    x = rn.Ciphertext(*[rn.RnsPoly.sample_uniform(basis, rng, n_terms * B) for _ in range(2)])
    m = rn.RnsPoly.sample_uniform(basis, rng, n_terms if shared else n_terms * B)
    m.to_ntt_domain()
    fo = [rn.RnsPoly(low, B) for _ in range(2)]

    def call_mac():
        rn.check(lib.rnt_ct_plain_mac_rescale(fo[0].handle, fo[1].handle, x.c0.handle, x.c1.handle, m.handle, None,
                                              n_terms))

    def term(p, i, count=B):
        t = rn.RnsPoly(basis, B)
        for b in range(B if count == 1 else 1):
            t.copy_polys(p, b, i * count, count)
        return t

    mc = m.clone()
    mc.to_coeff_domain()
    terms = [[term(x.c0, i), term(x.c1, i), term(mc, i, 1 if shared else B)] for i in range(n_terms)]
    acc = [rn.RnsPoly(basis, B) for _ in range(2)]
    tmp = [rn.RnsPoly(basis, B) for _ in range(2)]
    co = [rn.RnsPoly(low, B) for _ in range(2)]

    def call_comp():
        for i, t in enumerate(terms):
            o = acc if i == 0 else tmp
            rn.check(lib.rnt_mul(o[0].handle, t[0].handle, t[2].handle))
            rn.check(lib.rnt_mul(o[1].handle, t[1].handle, t[2].handle))
            if i:
                rn.check(lib.rnt_add(acc[0].handle, acc[0].handle, tmp[0].handle))
                rn.check(lib.rnt_add(acc[1].handle, acc[1].handle, tmp[1].handle))
        rn.check(lib.rnt_ct_rescale(co[0].handle, co[1].handle, acc[0].handle, acc[1].handle))

    call_mac()
    call_comp()
    for f, c in zip(fo, co):
        assert np.array_equal(f.channels_of(B - 1), c.channels_of(B - 1)), "the two forms differ"
    tm = Timer(basis, a.warmup, a.repeats, a.window)
    (t_m, t_c), iters = tm.alternate([call_mac, call_comp])
    split_m, split_c = tm.split(call_mac), tm.split(call_comp)
    # planes of B N words a call must move (DESIGN.md "Plaintext multiply-accumulate"): per term the gather (4 Lv),
    # two transforms in place (4 Lv) and the kernel's reads (2 Lv + the plaintext's Lv, or Lv / B shared); per group
    # of kPlainT terms the sums (2 Lv written, 2 Lv read again from the second group on); once the inverse of both
    # sums in place (4 Lv) and the rescale (2 Lv read, 2 (Lv - 1) written)
    groups = -(-n_terms // KPLAIN_T)
    planes = n_terms * (10 * L + (L / B if shared else L)) + (4 * groups - 2) * L + 4 * L + 2 * L + 2 * (L - 1)
    nbytes = planes * B * n * word
    mm, mc_ = float(np.median(t_m)), float(np.median(t_c))
    emit({"bench": "ct_plain_mac_rescale", "n_terms": n_terms, "batch": B, "plaintexts": "shared" if shared else "each",
          "iters": {"mac": iters[0], "composition": iters[1]}, "mac_ms": t_m, "composition_ms": t_c,
          "composition_over_mac_time": round(mc_ / mm, 3), "mac_ms_per_term": round(mm / n_terms, 4),
          "composition_ms_per_term": round(mc_ / n_terms, 4), "mac_model_bytes": int(nbytes),
          "mac_model_GBs": round(nbytes / (mm * 1e-3) / 1e9, 1), "mac_kernels": split_m,
          "composition_kernels": split_c,
          "mac_kernel_ms_sum": round(sum(v["ms"] for v in split_m.values()), 4),
          "composition_kernel_ms_sum": round(sum(v["ms"] for v in split_c.values()), 4)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", action="append", type=int, help="ciphertexts (repeatable; default 1, 8 and 64)")
    ap.add_argument("--terms", action="append", type=int, help="n_terms (repeatable; default 1, 4, 16)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timing window")
    ap.add_argument("--out", help="append the JSON lines to this file as well")
    a = ap.parse_args()
    n = 1 << LOG_N
    basis = rn.RnsBasis(rn.generate_primes(30, L, n), n)
    for B in a.batch or [1, 8, 64]:
        for n_terms in a.terms or [1, 4, 16]:
            for shared in (True, False):
                if B == 1 and not shared:
                    continue  # one ciphertext: the two forms are one
                run(basis, n_terms, B, shared, a, a.out)
                rn.pool_trim()
    return 0


if __name__ == "__main__":
    sys.exit(main())
