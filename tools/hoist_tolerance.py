#!/usr/bin/env python3
"""The decode error of the hoisted rotation's end-to-end pipelines, measured on
the CPU: the tolerances of tests/test_gpu_hoist.py's two end-to-end tests.

At N = 64, 4 x 31-bit primes, ciphertext scale 2^58, x uniform in (-1, 1), with
oracle/pyoracle, oracle/encoder.py, numpy draws and tests/hoist_ref.py:

* encode -> encrypt -> hoisted rotation by 1, -3, 7, 16 -> decrypt -> decode
  against the rolled slots (and the same through orc.rotate_ciphertext, to
  show the two forms' noise side by side);
* the 16-diagonal band of tools/bsgs_tolerance.py (baby [0,1,2,3] x giant
  [0,4,8,12], diagonal scale 2^30) through bsgs_hoisted_ref -> rescale ->
  decrypt -> decode against M x.

No device is touched.  Prints one line per seed and the largest errors.

    python tools/hoist_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "toy-heaan-ckks_amd", "tools"):
    sys.path.insert(0, os.path.join(REPO, p))

import encoder as enc  # noqa: E402
import pyoracle as orc  # noqa: E402
from bsgs_tolerance import BABY, GIANT, L, LOGP_D, LOGP_X, N, SLOTS, gauss, rotation_key, ternary  # noqa: E402
from hoist_ref import bsgs_hoisted_ref, rotate_hoisted_ref  # noqa: E402
from rns_ntt import bsgs_diagonal_rows  # noqa: E402

ROT_STEPS = [1, -3, 7, 16]


def _setup(seed):
    rng = np.random.default_rng(seed)
    mod = orc.generate_primes(31, L, N)
    Bo = orc.Basis(mod, N)
    sk = orc.from_coeffs(Bo, ternary(rng))
    a = orc.uniform_poly(mod, N, rng)
    pk_b = orc.add(Bo, orc.neg(Bo, orc.mul(Bo, a, sk)), gauss(Bo, rng))
    return rng, mod, Bo, sk, a, pk_b


def _encrypt(Bo, rng, a, pk_b, x):
    m = orc.from_coeffs(Bo, enc.encode_fft(x, N, LOGP_X))
    u = orc.from_coeffs(Bo, ternary(rng))
    c0 = orc.add(Bo, orc.add(Bo, orc.mul(Bo, pk_b, u), gauss(Bo, rng)), m)
    c1 = orc.add(Bo, orc.mul(Bo, a, u), gauss(Bo, rng))
    return c0, c1


def rolled(x, k):
    """The slots of a rotation by k: slot s holds old slot s + |k|, and for
    k < 0 its conjugate -- rotate_slots (poly.rs:546-569) composes the
    rotation by |k| with X -> X^(2N-1), the conjugation."""
    r = np.roll(x, -abs(int(k)))
    return np.conj(r) if k < 0 else r


def run_rotations(seed):
    """Largest decode error over ROT_STEPS of the hoisted and of the plain
    rotation of one fresh ciphertext."""
    rng, mod, Bo, sk, a, pk_b = _setup(seed)
    keys = {k: rotation_key(Bo, mod, sk, k, rng) for k in ROT_STEPS}
    x = rng.uniform(-1, 1, SLOTS)
    c0, c1 = _encrypt(Bo, rng, a, pk_b, x)
    errs = {"hoisted": 0.0, "plain": 0.0}
    for k in ROT_STEPS:
        want = rolled(x, k)
        for name, (o0, o1) in (("hoisted", rotate_hoisted_ref(Bo, c0, c1, k, *keys[k])),
                               ("plain", orc.rotate_ciphertext(Bo, c0, c1, k, *keys[k]))):
            dec = orc.add(Bo, orc.mul(Bo, o1, sk), o0)
            got = enc.decode_fft(orc.to_coeffs(Bo, dec), N, LOGP_X, SLOTS)
            errs[name] = max(errs[name], float(np.max(np.abs(got - want))))
    return errs


def run_bsgs(seed):
    rng, mod, Bo, sk, a, pk_b = _setup(seed)
    bk = [None if k == 0 else rotation_key(Bo, mod, sk, k, rng) for k in BABY]
    gk = [None if k == 0 else rotation_key(Bo, mod, sk, k, rng) for k in GIANT]
    x = rng.uniform(-1, 1, SLOTS)
    M = np.zeros((SLOTS, SLOTS))
    s = np.arange(SLOTS)
    for d in range(len(BABY) * len(GIANT)):
        M[s, (s + d) % SLOTS] = rng.uniform(-1, 1, SLOTS)
    c0, c1 = _encrypt(Bo, rng, a, pk_b, x)
    rows = bsgs_diagonal_rows(M, BABY, GIANT).reshape(-1, SLOTS)
    diag = np.stack([orc.from_coeffs(Bo, enc.encode_fft(r, N, LOGP_D)) for r in rows])
    o0, o1 = bsgs_hoisted_ref(Bo, c0, c1, BABY, GIANT, diag, bk, gk)
    r0, r1 = orc.rescale(Bo, o0), orc.rescale(Bo, o1)
    Bd = Bo.drop_last(1)
    dec = orc.add(Bd, orc.mul(Bd, r1, sk[: L - 1]), r0)
    logp = LOGP_X + LOGP_D - int(mod[-1]).bit_length()
    got = enc.decode_fft(orc.to_coeffs(Bd, dec), N, logp, SLOTS)
    y = M @ x
    return float(np.max(np.abs(got - y))), float(np.max(np.abs(y)))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst_h = worst_p = worst_b = 0.0
    for seed in range(n_seeds):
        e = run_rotations(seed)
        b, ymax = run_bsgs(seed)
        worst_h, worst_p, worst_b = max(worst_h, e["hoisted"]), max(worst_p, e["plain"]), max(worst_b, b)
        print(f"seed {seed}: rotation hoisted {e['hoisted']:.3e} plain {e['plain']:.3e}  "
              f"bsgs hoisted {b:.3e} (max|y| {ymax:.3f})")
    print(f"rotation, largest error over {n_seeds} seeds: hoisted {worst_h:.3e} (plain {worst_p:.3e}); "
          f"tolerance 4 x = {4 * worst_h:.3e}")
    print(f"bsgs hoisted, largest error over {n_seeds} seeds: {worst_b:.3e}; tolerance 4 x = {4 * worst_b:.3e}")


if __name__ == "__main__":
    main()
