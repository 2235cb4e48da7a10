#!/usr/bin/env python3
"""The decode errors of raise -> CoeffToSlot -> SlotToCoeff measured on the
CPU: the tolerances of tests/test_gpu_homdft.py and tests/test_homdft_ref.py.

The tests' ring -- 7 ciphertext primes of 30 bits (the largest below 2^30), 2
special primes of 31 bits, alpha = 2, ternary secret of Hamming weight 32,
errors of width 3.2 -- at N = 2^8 and 2^10.  For each seed a ciphertext of
slots uniform in the unit square, encoded at 2^20, is encrypted on ONE limb,
raised onto the seven (tests/homdft_ref.py mod_raise_ref) and sent through the
plans of rns_ntt.homdft_plan on tests/homdft_ref.py (one
bsgs_hybrid_rescale_ref per group, diagonals encoded by oracle/encoder.py at the
scale of the prime the group's rescale removes).  With ``a`` the centred CRT of
the raised ciphertext's decryption:

    slot   max |decode(CoeffToSlot) - R (a_j + i a_{j+n}) / 2^20|   (R the bit
           reversal; none for order="natural")
    back   max |decode(centred((t - a) mod q_0))| at 2^20, t the decryption of
           the one-limb ciphertext after SlotToCoeff: the round trip against a

    conj   max |decode(conjugate) - conj(slots)| for a fresh seven-limb
           ciphertext of the same slots and the hybrid rotation key of step -N/2
           (tests/hybrid_ref.py rotate_hybrid_ref): the bound of the conjugation
           and of the real and imaginary parts

all against float64.  |a| is about 2^33 (Q0 times the (h + 1) / 2 bound), so
the slot values are about 2^13 and an error of 1e-3 is 2^-23 of them.  No device
is touched.  Prints one line per seed and case and the largest errors per case;
the tests' tolerance is 4 x those.

    python tools/homdft_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", os.path.join("toy-heaan-ckks_amd", "rns_ntt")):
    sys.path.insert(0, os.path.join(REPO, p))

import pyoracle as orc  # noqa: E402
from homdft import homdft_plan  # noqa: E402  (the pure host module: no library needed)
import encoder as enc  # noqa: E402
from homdft_ref import HomDftModel, run_pipeline  # noqa: E402
from hybrid_ref import rotate_hybrid_ref  # noqa: E402

L, K, ALPHA, LOGP, HAMMING = 7, 2, 2, 20, 32
# (N, depth, order); order="natural" runs the slot side alone
CASES = [(256, 3, "bitrev"), (1024, 3, "bitrev"), (256, 1, "natural")]


def run(seed, n, depth, order):
    q, p = orc.generate_primes(30, L, n), orc.generate_primes(31, K, n)
    model = HomDftModel(q, p, n, ALPHA, HAMMING, seed)
    values = model.rng.uniform(-1, 1, n // 2) + 1j * model.rng.uniform(-1, 1, n // 2)
    c2s = homdft_plan(n, "coeff_to_slot", depth, order=order)
    s2c = homdft_plan(n, "slot_to_coeff", depth) if order == "bitrev" else None
    r = run_pipeline(model, c2s, s2c, values, LOGP)
    return r["slot_err"], r.get("back_err", float("nan"))


def run_conj(seed, n):
    q, p = orc.generate_primes(30, L, n), orc.generate_primes(31, K, n)
    model = HomDftModel(q, p, n, ALPHA, HAMMING, seed)
    values = model.rng.uniform(-1, 1, n // 2) + 1j * model.rng.uniform(-1, 1, n // 2)
    ct = model.encrypt(enc.encode_fft(values, n, LOGP), L)
    cj = rotate_hybrid_ref(model.Bc, model.Be, *ct, -(n // 2), *model.key(-(n // 2)), ALPHA)
    return float(np.max(np.abs(model.decode(cj, LOGP) - np.conj(values))))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = {c: [0.0, 0.0] for c in CASES}
    for seed in range(n_seeds):
        for c in CASES:
            slot, back = run(seed, *c)
            worst[c] = [max(worst[c][0], slot), max(worst[c][1], back) if back == back else float("nan")]
            print(f"seed {seed}: N {c[0]:5d} depth {c[1]} {c[2]:7s} slot {slot:.3e} back {back:.3e}")
    for n in (256, 1024):
        errs = [run_conj(seed, n) for seed in range(n_seeds)]
        print(f"N {n:5d} conj   : largest over {n_seeds} seeds {max(errs):.3e}; tolerance 4 x = {4 * max(errs):.3e}")
    for c in CASES:
        print(f"N {c[0]:5d} depth {c[1]} {c[2]:7s}: largest over {n_seeds} seeds slot {worst[c][0]:.3e} "
              f"back {worst[c][1]:.3e}; tolerance 4 x = {4 * worst[c][0]:.3e} / {4 * worst[c][1]:.3e}")


if __name__ == "__main__":
    main()
