"""tests/lincomb_ref.py against an independent big-int computation on a tiny
ring: the sums and the bias limb by limb on Python ints, then the rescale from
its definition out_t = (r_t - [r_last]_{q_t}) (q_last mod q_t)^-1 mod q_t."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from lincomb_ref import lincomb_ref, reduce_weights

N = 8


def _bigint(mods, x0, x1, n_in, w, bias, rescale):
    n_out, Lv = len(w), len(mods)
    B = len(x0) // n_in
    outs = []
    for comp, x in enumerate((x0, x1)):
        r = [[[0] * N for _ in range(Lv)] for _ in range(n_out * B)]
        for j in range(n_out):
            for b in range(B):
                for t, q in enumerate(mods):
                    for c in range(N):
                        v = sum(int(w[j][i][t]) * int(x[i * B + b][t][c]) for i in range(n_in))
                        if comp == 0 and c == 0 and bias is not None:
                            v += int(bias[j][t])
                        r[j * B + b][t][c] = v % q
        if rescale:
            ql = mods[-1]
            r = [[[(p[t][c] - p[-1][c] % q) * pow(ql % q, -1, q) % q for c in range(N)]
                  for t, q in enumerate(mods[:-1])] for p in r]
        outs.append(np.array(r, dtype=np.uint64))
    return outs


@pytest.mark.parametrize("bits", [20, 30, 60])
@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_lincomb_ref_matches_bigint(bits, rescale, with_bias):
    Lv, n_in, n_out, B = 3, 3, 2, 2
    mods = orc.generate_primes(bits, Lv, N)
    Bo = orc.Basis(mods, N)
    rng = np.random.default_rng(bits + 2 * rescale + with_bias)
    x0 = orc.uniform_poly(mods, N, rng, batch=n_in * B)
    x1 = orc.uniform_poly(mods, N, rng, batch=n_in * B)
    ints = [[int(v) for v in row] for row in rng.integers(-(1 << 40), 1 << 40, size=(n_out, n_in))]
    ints[0][0], ints[1][1] = -1, 0
    w = reduce_weights(ints, mods)
    assert w.shape == (n_out, n_in, Lv) and int(w[0, 0, 1]) == mods[1] - 1
    bias = reduce_weights([-(1 << 50), 12345], mods) if with_bias else None
    got = lincomb_ref(Bo, x0, x1, n_in, w, bias, rescale=rescale)
    want = _bigint(mods, x0, x1, n_in, w, bias, rescale)
    for g, h in zip(got, want):
        assert g.shape == h.shape == (n_out * B, Lv - int(rescale), N)
        assert np.array_equal(g, h)


def test_bias_lands_on_coefficient_zero_of_every_poly_of_component_zero_only():
    mods = orc.generate_primes(30, 2, N)
    Bo = orc.Basis(mods, N)
    z = np.zeros((3, 2, N), dtype=np.uint64)
    w = reduce_weights([[1]], mods)
    o0, o1 = lincomb_ref(Bo, z, z, 1, w, reduce_weights([7], mods))
    assert np.all(o0[:, :, 0] == 7) and not o0[:, :, 1:].any() and not o1.any()
