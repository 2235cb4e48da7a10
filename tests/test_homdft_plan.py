"""rns_ntt.homdft_plan (numpy only): the staged factorisation of the encoder's
slot matrix U against U built from its definition, the diagonal bounds, the
sparse product and the BSGS grids."""
from __future__ import annotations

import numpy as np
import pytest

import encoder as enc
from rns_ntt.homdft import bit_reverse_permutation, diag_product, homdft_plan, stage_diagonals

SLOTS = [4, 8, 32, 128, 512]
CASES = [(n, d) for n in SLOTS for d in range(1, n.bit_length())]


def slot_matrix(n):
    """U[k][j] = zeta^(5^k j), zeta = exp(i pi / N), N = 2n."""
    N = 2 * n
    e = [pow(5, k, 2 * N) for k in range(n)]
    return np.exp(1j * np.pi * ((np.array(e)[:, None] * np.arange(n)[None, :]) % (2 * N)) / N)


def dense(diags, n):
    s = np.arange(n)
    M = np.zeros((n, n), dtype=np.complex128)
    for k, d in diags.items():
        M[s, (s + k) % n] += d
    return M


def product(plan):
    """The groups multiplied out, the first applied rightmost."""
    n = plan.slots
    M = np.eye(n, dtype=np.complex128)
    for g in plan.groups:
        M = dense(g.diags, n) @ M
    return M


def test_u_is_the_encoders_slot_map():
    n, N = 32, 64
    rng = np.random.default_rng(1)
    a = rng.integers(-1000, 1000, N)
    w = a[:n] + 1j * a[n:]
    assert np.allclose(slot_matrix(n) @ w, enc.decode_fft(a, N, 0, n), atol=1e-9)


@pytest.mark.parametrize("n,depth", CASES)
def test_groups_multiply_to_the_slot_matrix(n, depth):
    U = slot_matrix(n)
    P = np.zeros((n, n))
    P[np.arange(n), bit_reverse_permutation(n)] = 1  # U = S_m .. S_1 R  =>  S_m .. S_1 = U R^-1 = U R
    s2c, c2s = homdft_plan(2 * n, "slot_to_coeff", depth), homdft_plan(2 * n, "coeff_to_slot", depth)
    M, Mi = product(s2c), product(c2s)
    scale = np.abs(U @ P).max()
    assert np.abs(M - U @ P).max() <= 1e-9 * scale
    assert np.abs(Mi @ M - np.eye(n)).max() <= 1e-9
    assert np.abs(Mi - P @ U.conj().T / n).max() <= 1e-9
    sizes = [len(g.stages) for g in s2c.groups]
    assert len(sizes) == depth and sum(sizes) == n.bit_length() - 1 and max(sizes) - min(sizes) <= 1
    assert [t for g in s2c.groups for t in g.stages] == list(range(1, n.bit_length()))
    assert [t for g in c2s.groups for t in g.stages] == list(range(n.bit_length() - 1, 0, -1))
    # plan.apply is the same map on a vector
    v = np.random.default_rng(n + depth).normal(size=n) + 1j * np.random.default_rng(depth).normal(size=n)
    assert np.allclose(s2c.apply(v), M @ v, atol=1e-9 * scale)


@pytest.mark.parametrize("n,depth", CASES)
def test_diagonal_bound_and_bsgs_grids(n, depth):
    for direction in ("slot_to_coeff", "coeff_to_slot"):
        plan = homdft_plan(2 * n, direction, depth)
        for g in plan.groups:
            nonzero = [k for k, d in g.diags.items() if np.any(d != 0)]
            assert len(nonzero) <= 2 ** (len(g.stages) + 1) - 1
            assert g.stride == 1 << (min(g.stages) - 1) and all(k % g.stride == 0 for k in nonzero)
            steps = g.baby_steps + g.giant_steps
            assert all(0 <= s < n for s in steps) and g.baby_steps[0] == 0
            assert all(b % g.stride == 0 for b in g.baby_steps)
            grid = [(a + b) % n for a in g.giant_steps for b in g.baby_steps]
            assert len(set(grid)) == len(grid), "a diagonal is named twice"
            assert set(nonzero) <= set(grid)
        keyed = plan.rotation_steps()
        assert len(keyed) == depth and all(0 not in b + gs for b, gs in keyed)
        assert plan.n_keyswitches() == sum(len(b) + len(gs) for b, gs in keyed)


def test_stage_has_three_diagonals_and_the_sparse_product_is_the_dense_one():
    n = 32
    for t in range(1, 6):
        S = stage_diagonals(2 * n, t)
        half = (1 << t) // 2
        assert set(S) == {0, half % n, (-half) % n} and len(S) == (2 if t == 5 else 3)
        assert np.allclose(dense(S, n).conj().T @ dense(S, n), 2 * np.eye(n))  # S^-1 = S^H / 2
    A, B = stage_diagonals(2 * n, 3), stage_diagonals(2 * n, 2)
    AB = diag_product(A, B, n)
    assert np.allclose(dense(AB, n), dense(A, n) @ dense(B, n))
    ABC = diag_product(stage_diagonals(2 * n, 4), AB, n)
    assert len(ABC) == 15  # three stages: 2^(3+1) - 1 diagonals
    assert np.allclose(dense(ABC, n), dense(stage_diagonals(2 * n, 4), n) @ dense(AB, n))


@pytest.mark.parametrize("n", [4, 32, 128])
def test_natural_order_is_u_itself(n):
    U = slot_matrix(n)
    p = homdft_plan(2 * n, "slot_to_coeff", 1, order="natural")
    assert len(p.groups) == 1 and np.abs(product(p) - U).max() <= 1e-9 * np.abs(U).max()
    pi = homdft_plan(2 * n, "coeff_to_slot", 1, order="natural")
    assert np.abs(product(pi) @ U - np.eye(n)).max() <= 1e-9
    grid = [(a + b) % n for a in p.groups[0].giant_steps for b in p.groups[0].baby_steps]
    assert sorted(grid) == list(range(n))
    with pytest.raises(ValueError):
        homdft_plan(2 * n, "slot_to_coeff", 2, order="natural")


@pytest.mark.parametrize("constant", [0.25, -3.0, 0.5 + 2j])
def test_constant_multiplies_the_product_once(constant):
    n = 32
    for depth in (1, 2, 5):
        for direction in ("slot_to_coeff", "coeff_to_slot"):
            base = product(homdft_plan(2 * n, direction, depth))
            got = product(homdft_plan(2 * n, direction, depth, constant=constant))
            assert np.abs(got - constant * base).max() <= 1e-9 * max(1.0, np.abs(base).max()) * abs(constant)


def test_the_large_ring_is_planned_without_a_dense_matrix():
    plan = homdft_plan(1 << 16, "coeff_to_slot", 3)
    assert [len(g.stages) for g in plan.groups] == [5, 5, 5]
    assert all(len(g.diags) <= 63 and all(d.shape == (1 << 15,) for d in g.diags.values()) for g in plan.groups)


def test_refused_arguments():
    for bad in (dict(degree=48), dict(direction="both"), dict(depth=0), dict(depth=6), dict(order="reversed")):
        args = dict(degree=64, direction="slot_to_coeff", depth=2)
        args.update(bad)
        with pytest.raises(ValueError):
            homdft_plan(**args)
