#!/usr/bin/env python3
"""The decode error of the baby-step giant-step linear transform's end-to-end
pipeline, measured on the CPU: the tolerance of
tests/test_gpu_bsgs.py::test_engine_linear_transform_bsgs_end_to_end.

encode -> encrypt -> 16-diagonal band (baby [0,1,2,3] x giant [0,4,8,12]) ->
rescale -> decrypt -> decode at N = 64, 4 x 31-bit primes, ciphertext scale
2^58, diagonal scale 2^30, x and the entries uniform in (-1, 1), with
oracle/pyoracle, oracle/encoder.py, numpy draws and tests/bsgs_ref.py.  No
device is touched.  Prints one line per seed and the largest error.

    python tools/bsgs_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "toy-heaan-ckks_amd"):
    sys.path.insert(0, os.path.join(REPO, p))

import encoder as enc  # noqa: E402
import pyoracle as orc  # noqa: E402
from bsgs_ref import bsgs_ref  # noqa: E402
from rns_ntt import bsgs_diagonal_rows  # noqa: E402

N, SLOTS, L = 64, 32, 4
LOGP_X, LOGP_D = 58, 30
BABY, GIANT = [0, 1, 2, 3], [0, 4, 8, 12]
SIGMA, HW = 3.2, N // 2


def ternary(rng):
    c = np.zeros(N, dtype=np.int64)
    idx = rng.choice(N, size=HW, replace=False)
    c[idx] = rng.choice(np.array([-1, 1], dtype=np.int64), size=HW)
    return c


def gauss(Bo, rng):
    return orc.from_coeffs(Bo, np.rint(rng.normal(0.0, SIGMA, size=N)).astype(np.int64))


def rotation_key(Bo, mod, sk, k, rng):
    """b_i = -(a_i s) + e_i + (rotate_slots(s, k) on channel i only)."""
    target, _ = orc.rotate_slots(Bo, sk, k)
    ka = orc.uniform_poly(mod, N, rng, batch=L)
    kb = np.zeros_like(ka)
    for i in range(L):
        plain = np.zeros((L, N), dtype=np.uint64)
        plain[i] = target[i]
        kb[i] = orc.add(Bo, orc.add(Bo, orc.neg(Bo, orc.mul(Bo, ka[i], sk)), gauss(Bo, rng)), plain)
    return ka, kb


def run(seed):
    rng = np.random.default_rng(seed)
    mod = orc.generate_primes(31, L, N)
    Bo = orc.Basis(mod, N)
    sk = orc.from_coeffs(Bo, ternary(rng))
    a = orc.uniform_poly(mod, N, rng)
    pk_b = orc.add(Bo, orc.neg(Bo, orc.mul(Bo, a, sk)), gauss(Bo, rng))
    bk = [None if k == 0 else rotation_key(Bo, mod, sk, k, rng) for k in BABY]
    gk = [None if k == 0 else rotation_key(Bo, mod, sk, k, rng) for k in GIANT]
    x = rng.uniform(-1, 1, SLOTS)
    M = np.zeros((SLOTS, SLOTS))
    s = np.arange(SLOTS)
    for d in range(len(BABY) * len(GIANT)):
        M[s, (s + d) % SLOTS] = rng.uniform(-1, 1, SLOTS)
    m = orc.from_coeffs(Bo, enc.encode_fft(x, N, LOGP_X))
    u = orc.from_coeffs(Bo, ternary(rng))
    c0 = orc.add(Bo, orc.add(Bo, orc.mul(Bo, pk_b, u), gauss(Bo, rng)), m)
    c1 = orc.add(Bo, orc.mul(Bo, a, u), gauss(Bo, rng))
    rows = bsgs_diagonal_rows(M, BABY, GIANT).reshape(-1, SLOTS)
    diag = np.stack([orc.from_coeffs(Bo, enc.encode_fft(r, N, LOGP_D)) for r in rows])
    o0, o1 = bsgs_ref(Bo, c0, c1, BABY, GIANT, diag, bk, gk)
    r0, r1 = orc.rescale(Bo, o0), orc.rescale(Bo, o1)
    Bd = Bo.drop_last(1)
    dec = orc.add(Bd, orc.mul(Bd, r1, sk[: L - 1]), r0)
    logp = LOGP_X + LOGP_D - int(mod[-1]).bit_length()
    got = enc.decode_fft(orc.to_coeffs(Bd, dec), N, logp, SLOTS)
    y = M @ x
    return float(np.max(np.abs(got - y))), float(np.max(np.abs(y)))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = 0.0
    for seed in range(n_seeds):
        err, ymax = run(seed)
        worst = max(worst, err)
        print(f"seed {seed}: max|got - y| {err:.3e}  max|y| {ymax:.3f}  relative {err / ymax:.2e}")
    print(f"largest error over {n_seeds} seeds: {worst:.3e}; tolerance 4 x = {4 * worst:.3e}")


if __name__ == "__main__":
    main()
