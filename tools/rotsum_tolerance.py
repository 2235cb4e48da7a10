#!/usr/bin/env python3
"""The decode error of an inner sum formed by the EXISTING chain of
``rotate_ciphertext_hybrid`` and ``add_ciphertexts``, measured on the GPU: the
tolerance of tests/test_gpu_inner_sum.py.

Ring of that test: N = 2^10, 4 ciphertext primes of 30 bits and 2 special
primes of 31, alpha = 2, scale 2^30, ternary secret of weight N / 2, errors of
width 3.2, slots uniform in (-1, 1).  For each seed (a DeviceRng) one secret,
one ciphertext, and for each configuration (n, stride) of the test the chain

    acc = ct;  acc += rotate_ciphertext_hybrid(ct, t stride)  for 0 < t < n

with a fresh rotation key per step; the result is decrypted, decoded and
compared with numpy's sum of the rolled slot vectors.  The new call's error on
the same ciphertext, secret and seed is printed beside it (every radix the test
runs), for the record only: the bound comes from the chain alone.  Both are sums
of independent key-switch errors of one distribution and the new call has fewer
ModDown terms, so the test allows it 4 x the chain's largest error.

Prints one line per seed and configuration and writes the figures to
profiles/rotsum_tolerance.txt.

    python tools/rotsum_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "toy-heaan-ckks_amd"))

import rns_ntt as rn  # noqa: E402
from rns_ntt.engine import CkksEngine  # noqa: E402
from rns_ntt.rotsum import rotsum_plan  # noqa: E402

N, L, K, ALPHA, LOGP = 1024, 4, 2, 2, 30
# (n, stride) -> the plans the test runs on it
CONFIGS = {
    (16, 1): [{"radix": 2}, {"radix": 4}, {"radix": 16}],
    (16, 4): [{"radix": 4}],
    (12, 1): [{"radices": (4, 3)}],
}
OUT = os.path.join(REPO, "profiles", "rotsum_tolerance.txt")


def engine():
    return CkksEngine(rn.generate_primes(30, L, N), N, error_std=3.2, hamming_weight=N // 2,
                      special_moduli=rn.generate_primes(31, K, N))


def expected(x, n, stride):
    return sum(np.roll(x, -t * stride) for t in range(n))


def decode_error(eng, enc, ct, sk, want):
    got = enc.decode(CkksEngine.decrypt_plaintext(ct, CkksEngine.secret_on(sk, ct.c0.basis)))
    return float(np.max(np.abs(got - want)))


def run(seed):
    eng = engine()
    rng = rn.DeviceRng(7000 + seed)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    x = np.random.default_rng(7100 + seed).uniform(-1, 1, N // 2)
    enc = rn.CkksEncoder(N, LOGP)
    ct = eng.encrypt(enc.encode(x, eng.basis), pk, rng)
    res = {}
    for (n, stride), plans in CONFIGS.items():
        want = expected(x, n, stride)
        acc = ct
        for t in range(1, n):
            key = eng.generate_hybrid_rotation_key(sk, t * stride, rng, ALPHA)
            acc = CkksEngine.add_ciphertexts(acc, CkksEngine.rotate_ciphertext_hybrid(ct, key))
        chain = decode_error(eng, enc, acc, sk, want)
        new = []
        for kw in plans:
            plan = rotsum_plan(n, stride, n_slots=N // 2, **kw)
            sets = eng.generate_rotsum_key_sets(sk, plan, rng, ALPHA)
            new.append(decode_error(eng, enc, CkksEngine.inner_sum_hybrid(ct, plan, sets), sk, want))
        res[(n, stride)] = (chain, new)
    return res


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = {c: 0.0 for c in CONFIGS}
    worst_new = {c: 0.0 for c in CONFIGS}
    for seed in range(n_seeds):
        for c, (chain, new) in run(seed).items():
            worst[c] = max(worst[c], chain)
            worst_new[c] = max(worst_new[c], *new)
            print(f"seed {seed}: n = {c[0]}, stride {c[1]}: chain {chain:.3e}; inner_sum_hybrid "
                  + ", ".join(f"{e:.3e}" for e in new), flush=True)
    lines = [f"inner sums at N = {N}, {L} x 30-bit primes + {K} special, alpha = {ALPHA}, scale 2^{LOGP}, "
             f"{n_seeds} seeds: largest decode errors"]
    for c in CONFIGS:
        lines.append(f"n = {c[0]}, stride {c[1]}: chain of rotate_ciphertext_hybrid + add_ciphertexts {worst[c]:.3e}; "
                     f"inner_sum_hybrid (plans {CONFIGS[c]}) {worst_new[c]:.3e}")
    top = max(worst.values())
    lines.append(f"largest chain error {top:.3e}; tolerance of the new call 4 x = {4 * top:.3e}")
    print("\n".join(lines))
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
