"""The baby-step giant-step yardstick (tests/bsgs_ref.py) on a 2^6 ring with
two 31-bit primes -- against a version whose plaintext products are schoolbook
and, with giant = [0], against the linear transform's yardstick -- and the
slot rule of bsgs_diagonal_rows in numpy: the yardstick and the diagonal
layout are shown right here, before any GPU run relies on them."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from bsgs_ref import bsgs_ref
from lt_ref import linear_ref

BABY = [0, 1, -3, 1]
GIANT = [0, 4, -8, 4]


def _keys(mod, n, rng, steps):
    L = len(mod)
    return [None if k == 0 else (orc.uniform_poly(mod, n, rng, batch=L), orc.uniform_poly(mod, n, rng, batch=L))
            for k in steps]


def _case(seed=21, baby=BABY, giant=GIANT):
    n, L = 64, 2
    mod = orc.generate_primes(31, L, n)
    Bo = orc.Basis(mod, n)
    rng = np.random.default_rng(seed)
    c0, c1 = orc.uniform_poly(mod, n, rng), orc.uniform_poly(mod, n, rng)
    diag = orc.uniform_poly(mod, n, rng, batch=len(baby) * len(giant))
    return Bo, mod, c0, c1, diag, _keys(mod, n, rng, baby), _keys(mod, n, rng, giant)


def test_bsgs_ref_matches_schoolbook_products():
    Bo, mod, c0, c1, diag, bk, gk = _case()
    got = bsgs_ref(Bo, c0, c1, BABY, GIANT, diag, bk, gk)
    want = bsgs_ref(Bo, c0, c1, BABY, GIANT, diag, bk, gk, mul=lambda x, y: orc.mul_naive(Bo, x, y))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    q = np.array(mod, dtype=np.uint64)[:, None]
    assert (got[0] < q).all() and (got[1] < q).all()


def test_bsgs_ref_with_one_zero_giant_is_linear_ref():
    Bo, mod, c0, c1, diag, bk, gk = _case(22, giant=[0])
    got = bsgs_ref(Bo, c0, c1, BABY, [0], diag, bk, [None])
    want = linear_ref(Bo, c0, c1, BABY, diag, bk)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_bsgs_ref_with_one_zero_baby_is_a_sum_of_rotated_products():
    """n1 = 1, b = [0]: out = sum_j rotate(P_j * ct, g_j)."""
    Bo, mod, c0, c1, diag, bk, gk = _case(23, baby=[0])
    got = bsgs_ref(Bo, c0, c1, [0], GIANT, diag, [None], gk)
    acc = None
    for j, g in enumerate(GIANT):
        v = orc.mul_naive(Bo, c0, diag[j]), orc.mul_naive(Bo, c1, diag[j])
        r = v if g == 0 else orc.rotate_ciphertext(Bo, v[0], v[1], g, gk[j][0], gk[j][1])
        acc = r if acc is None else (orc.add(Bo, acc[0], r[0]), orc.add(Bo, acc[1], r[1]))
    assert np.array_equal(got[0], acc[0]) and np.array_equal(got[1], acc[1])


def _rot(x, k):
    """Slot s of a rotation by k holds old slot s + k."""
    return np.roll(x, -k)


@pytest.mark.parametrize("baby,giant", [
    (list(range(8)), [0, 8, 16, 24]),   # dense: every one of the 32 diagonals
    ([0, 1, 2, 3], [0, 4, 8, 12]),      # a band of 16
    ([0, 1, 31], [0, 3]),               # a band that wraps around
])
def test_bsgs_diagonal_rows_slot_identity(baby, giant):
    from rns_ntt import bsgs_diagonal_rows

    slots = 32
    rng = np.random.default_rng(5)
    M = rng.uniform(-1, 1, (slots, slots)) + 1j * rng.uniform(-1, 1, (slots, slots))
    x = rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots)
    rows = bsgs_diagonal_rows(M, baby, giant)
    assert rows.shape == (len(giant), len(baby), slots)
    got = sum(_rot(sum(rows[j][i] * _rot(x, b) for i, b in enumerate(baby)), g) for j, g in enumerate(giant))
    s = np.arange(slots)
    band = np.zeros_like(M)
    for g in giant:
        for b in baby:
            band[s, (s + g + b) % slots] = M[s, (s + g + b) % slots]
    assert np.allclose(got, band @ x, rtol=0, atol=1e-12)
    if len(baby) * len(giant) == slots:
        assert np.array_equal(band, M)


def test_bsgs_diagonal_rows_rejects_bad_steps():
    from rns_ntt import bsgs_diagonal_rows

    M = np.zeros((32, 32))
    with pytest.raises(ValueError, match="negative"):
        bsgs_diagonal_rows(M, [0, -1], [0, 4])
    with pytest.raises(ValueError, match="negative"):
        bsgs_diagonal_rows(M, [0, 1], [0, -4])
    with pytest.raises(ValueError, match="diagonal"):
        bsgs_diagonal_rows(M, [0, 1, 2], [0, 2])  # 0 + 2 == 2 + 0
    with pytest.raises(ValueError, match="diagonal"):
        bsgs_diagonal_rows(M, [0, 1], [0, 32])    # the same diagonals mod slots
