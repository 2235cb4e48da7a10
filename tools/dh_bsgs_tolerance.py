#!/usr/bin/env python3
"""The decode error of the double-hoisted pipelines, measured on the CPU: the
tolerances of tests/test_gpu_dh_bsgs.py's end-to-end tests, beside the figures
of rnt_ct_linear_bsgs_hybrid's model on the SAME draws.

tools/hybrid_tolerance.py's ring -- N = 2^10, 4 x 31-bit ciphertext primes (the
smallest above 2^30) + 2 special primes (the largest below 2^31), alpha = 2,
scale 2^30 -- with oracle/pyoracle, oracle/encoder.py, numpy draws,
tests/dh_bsgs_ref.py and tests/hybrid_hoist_ref.py:

* band: a 16-diagonal band, diagonals at scale 2^30, baby [0, 1, 2, 3] x giant
  [0, 4, 8, 12] -> rescale -> decrypt -> decode against M x
  (tools/hybrid_hoist_tolerance.py's run_band, draw for draw), the plaintexts
  encoded over Q u P for dh_bsgs_ref and over Q for bsgs_hybrid_ref;
* back: slots uniform in the unit square, encrypted on the four limbs ->
  CoeffToSlot (homdft_plan depth 1: one 32 x 16 group) -> SlotToCoeff (depth 1)
  -> decrypt on the two limbs left -> decode against the slots; every group is
  one transform followed by the rescale, its diagonals encoded at the scale of
  the prime the rescale removes (CkksEngine.prepare_homdft's rule), the keys
  the full-level keys restricted to the group's level.

No device is touched.  Prints one line per seed and the largest errors; the
tests assert 4 x the double-hoisted figures.

    python tools/dh_bsgs_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "toy-heaan-ckks_amd", "tools", os.path.join("toy-heaan-ckks_amd", "rns_ntt")):
    sys.path.insert(0, os.path.join(REPO, p))

import encoder as enc  # noqa: E402
import pyoracle as orc  # noqa: E402
from dh_bsgs_ref import dh_bsgs_ref  # noqa: E402
from homdft import homdft_plan  # noqa: E402  (the pure host module: no library needed)
from hybrid_hoist_ref import bsgs_hybrid_ref  # noqa: E402
from hybrid_hoist_tolerance import BABY, DIAGS, GIANT, _setup  # noqa: E402
from hybrid_ref import restrict_key  # noqa: E402
from hybrid_tolerance import ALPHA, K, L, LOGP, N, SLOTS  # noqa: E402
from rns_ntt import bsgs_diagonal_rows  # noqa: E402


def run_band(seed):
    """(double-hoisted, rnt_ct_linear_bsgs_hybrid's model) on one set of draws."""
    rng, mod, modc, Be, Bc, sk, encrypt, rot_key = _setup(seed)
    bk = [None if k == 0 else rot_key(k) for k in BABY]
    gk = [None if k == 0 else rot_key(k) for k in GIANT]
    x = rng.uniform(-1, 1, SLOTS)
    M = np.zeros((SLOTS, SLOTS))
    s = np.arange(SLOTS)
    for d in DIAGS:
        M[s, (s + d) % SLOTS] = rng.uniform(-1, 1, SLOTS)
    c0, c1 = encrypt(x)
    rows = bsgs_diagonal_rows(M, BABY, GIANT).reshape(-1, SLOTS)
    diagE = np.stack([orc.from_coeffs(Be, enc.encode_fft(r, N, LOGP)) for r in rows])
    Bd = Bc.drop_last(1)
    logp = 2 * LOGP - int(modc[-1]).bit_length()
    # logp counts the dropped prime as 31 bits; the true scale is 2^60 / q_last
    y = (M @ x) * (2.0 ** (2 * LOGP - logp) / modc[-1])
    errs = []
    for o0, o1 in (dh_bsgs_ref(Bc, Be, c0, c1, BABY, GIANT, diagE, bk, gk, ALPHA),
                   bsgs_hybrid_ref(Bc, Be, c0, c1, BABY, GIANT, diagE[:, :L], bk, gk, ALPHA)):
        r0, r1 = orc.rescale(Bc, o0), orc.rescale(Bc, o1)
        dec = orc.add(Bd, orc.mul(Bd, r1, sk[: L - 1]), r0)
        got = enc.decode_fft(orc.to_coeffs(Bd, dec), N, logp, SLOTS)
        errs.append(float(np.max(np.abs(got - y))))
    return errs


def _transform(plan, ct, mod, keys, dh):
    """The plan's groups in order on (c0, c1), one level down each."""
    q, p = mod[:L], mod[L:]
    for group in plan.groups:
        lv = ct[0].shape[0]
        Bc, Be = orc.Basis(q[:lv], N), orc.Basis(q[:lv] + p, N)
        bits = q[lv - 1].bit_length()
        drift = q[lv - 1] / 2.0 ** bits
        rows = []
        for g in group.giant_steps:
            for b in group.baby_steps:
                d = group.diags.get((g + b) % SLOTS)
                row = np.zeros(SLOTS, dtype=np.complex128) if d is None else np.roll(d, g) * drift
                rows.append(orc.from_coeffs(Be, enc.encode_fft(row, N, bits)))
        diagE = np.stack(rows)

        def at(steps):
            return [None if s == 0 else tuple(restrict_key(k, L, ALPHA, lv) for k in keys(s)) for s in steps]

        bk, gk = at(group.baby_steps), at(group.giant_steps)
        if dh:
            o = dh_bsgs_ref(Bc, Be, ct[0], ct[1], group.baby_steps, group.giant_steps, diagE, bk, gk, ALPHA)
        else:
            o = bsgs_hybrid_ref(Bc, Be, ct[0], ct[1], group.baby_steps, group.giant_steps, diagE[:, :lv], bk, gk, ALPHA)
        ct = (orc.rescale(Bc, o[0]), orc.rescale(Bc, o[1]))
    return ct


def run_back(seed):
    rng, mod, modc, Be, Bc, sk, encrypt, rot_key = _setup(seed)
    cache = {}

    def keys(step):
        if step not in cache:
            cache[step] = rot_key(step)
        return cache[step]

    x = rng.uniform(-1, 1, SLOTS) + 1j * rng.uniform(-1, 1, SLOTS)
    ct = encrypt(x)
    c2s, s2c = homdft_plan(N, "coeff_to_slot", 1), homdft_plan(N, "slot_to_coeff", 1)
    errs = []
    for dh in (True, False):
        back = _transform(s2c, _transform(c2s, ct, mod, keys, dh), mod, keys, dh)
        lv = back[0].shape[0]
        Bl = orc.Basis(modc[:lv], N)
        dec = orc.add(Bl, orc.mul(Bl, back[1], sk[:lv]), back[0])
        got = enc.decode_fft(orc.to_coeffs(Bl, dec), N, LOGP, SLOTS)
        errs.append(float(np.max(np.abs(got - x))))
    return errs


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    assert K == 2
    worst = [0.0] * 4
    for seed in range(n_seeds):
        e = run_band(seed) + run_back(seed)
        worst = [max(w, v) for w, v in zip(worst, e)]
        print(f"seed {seed}: band double-hoisted {e[0]:.3e}  bsgs hybrid {e[1]:.3e}   "
              f"back double-hoisted {e[2]:.3e}  bsgs hybrid {e[3]:.3e}")
    names = ("band 4 x 4, double-hoisted", "band 4 x 4, rnt_ct_linear_bsgs_hybrid",
             "CoeffToSlot then SlotToCoeff, double-hoisted", "CoeffToSlot then SlotToCoeff, rnt_ct_linear_bsgs_hybrid")
    for name, w in zip(names, worst):
        print(f"{name}, largest error over {n_seeds} seeds: {w:.3e}; tolerance 4 x = {4 * w:.3e}")


if __name__ == "__main__":
    main()
