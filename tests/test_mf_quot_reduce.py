"""The quotient-estimate reduction of the matrix-core passes (rnt_mfma.hip,
recomb_q) as a Python-integer model.

A pass on a plain (non-Montgomery) matrix turns its digit sums into
    lo = C0 + 2^8 C1,  hi' = C2 + 2^8 (C3 + c)      (c = 48, through the MFMA
                                                     accumulator of plane 3)
    qt = floor(hi' mu / 2^32)                        mu = floor(2^48 / q)
    r  = ((hi' << 16) + lo) - qt q - c 2^24          in 32-bit arithmetic
and hands r on packed, (r + 0x80808080) ^ 0x80808080, or to a signed
Montgomery product.  Checked here for every pass that uses the form:
  - r == T (mod q) for T = lo + 2^16 (C2 + 2^8 C3), computed in wrapping
    32-bit arithmetic as the kernel does;
  - r lies inside the bound mf_build computes for the prime (the same integer
    formula), and that bound inside the packed range, so the word packs;
  - an input-biased pass (pass 0, the standalone inverse's first pass), whose
    accumulators of planes 0 and 2 start at the split compensation
    v = v0 + 2^16 v2 (|v0| <= 2^15, |v2| <= 2^14 + 1);
  - the second step of a two-step pass, REDC(r t) with |t| <= q/2, and the
    product epilogue of k_mf_mul, REDC(a b) with both operands at the bound:
    |a b + m q| < 2^63 and the result inside the packed range.
The words that are made canonical (canon(): r in (-q, q)) come from
Montgomery-form passes only; the last test shows why: the model's |r| reaches
q for the smaller primes.  Needs no GPU and no library.
"""
import itertools
import random

import pytest

from test_mf_twist_fold import PRIMES, generate_primes, is_prime, pack_roundtrip, redc, s32

N = 1 << 16
PACK_HI = 0x7F7F7F7F
CMAX = 1 << 20  # |digit sum| <= 2^20 (64 products of two balanced bytes)
C = 48
SMALLEST_31 = 1073872897  # the smallest NTT-friendly 31-bit prime
ALL_PRIMES = PRIMES[:16] + [SMALLEST_31] + PRIMES[16:]


def bound(q):
    """mf_build's bound on |r| (the same integers)."""
    Bq = (1 << 28) + (1 << 20) + (1 << 15)
    rho = (1 << 48) % q
    neg = Bq + (C << 24) + (((Bq - (C << 8)) * rho) >> 32) + 1
    pos = Bq + q + (((Bq + (C << 8)) * rho) >> 32) + 1 - (C << 24)
    return max(neg, pos)


def recomb_q(c0, c1, c2, c3, q, wk):
    """The kernel's arithmetic: uint32 wrapping, c3 without the offset (the
    MFMA adds it)."""
    mu = (1 << 48) // q
    lo = (c0 + (c1 << 8)) & 0xFFFFFFFF
    hi = (c2 + ((c3 + C) << 8)) & 0xFFFFFFFF
    qt = (s32(hi) * mu) >> 32  # v_mul_hi_i32: floor
    assert s32(qt) == qt
    kq = (0x80808080 if wk else 0) - (C << 24)
    return s32(((hi << 16) + lo) + qt * (-q) + kq)


def digit_sums(rng, extra=0):
    """Corners of the halves (+-(2^28 + 2^20) in every sign combination), the
    single planes at their limit, random ones."""
    out = list(itertools.product((-CMAX, CMAX), repeat=4))
    for a in range(4):
        for sgn in (-CMAX, CMAX):
            v = [0, 0, 0, 0]
            v[a] = sgn
            out.append(tuple(v))
    out += [tuple(rng.randint(-CMAX, CMAX) for _ in range(4)) for _ in range(2000)]
    return out


def split(v):
    v2 = (v + 32768) >> 16
    return v - (v2 << 16), v2


def test_prime_set():
    assert len(ALL_PRIMES) == 19 and len(set(ALL_PRIMES)) == 19
    assert is_prime(SMALLEST_31) and SMALLEST_31 % (2 * N) == 1
    assert not any(is_prime(c) for c in range((1 << 30) + 1, SMALLEST_31, 2 * N))
    assert [p.bit_length() for p in ALL_PRIMES] == [31] * 17 + [30, 29]
    assert PRIMES[:16] == generate_primes(31, 16, N)


@pytest.mark.parametrize("q", ALL_PRIMES)
def test_bounds_mf_build_checks(q):
    """The three inequalities mf_build requires of the prime."""
    rq = bound(q)
    assert (1 << 48) // q <= 0x7FFFFFFF
    assert rq <= PACK_HI
    assert rq * q // (1 << 33) + q // 2 + 1 < PACK_HI
    assert rq * rq // (1 << 32) + q // 2 + 1 < PACK_HI
    assert rq * rq + (1 << 31) * q < 1 << 63


@pytest.mark.parametrize("q", ALL_PRIMES)
@pytest.mark.parametrize("wk", [True, False])
def test_reduction_congruent_and_in_range(q, wk):
    """pass_p1 / ipass_p2 / pass_p4 (k_mf_mul) and the first step of pass_p3 /
    ipass_p4 with packed input: no compensation."""
    rng = random.Random(q)
    rq = bound(q)
    worst = 0
    for c0, c1, c2, c3 in digit_sums(rng):
        T = c0 + (c1 << 8) + ((c2 + (c3 << 8)) << 16)
        r = recomb_q(c0, c1, c2, c3, q, wk)
        if wk:
            r = s32(r - 0x80808080)
        assert (r - T) % q == 0
        assert abs(r) <= rq
        assert pack_roundtrip(r) == r
        worst = max(worst, abs(r))
    print(f"q={q}: max |r|/q = {worst / q:.4f}, bound/q = {rq / q:.4f}, max |r|/0x7F7F7F7F = {worst / PACK_HI:.4f}")


@pytest.mark.parametrize("q", ALL_PRIMES)
def test_biased_pass_with_split_compensation(q):
    """pass 0 and the standalone inverse's first pass: planes 0 and 2 start at
    the halves of the compensation, any residue centred."""
    rng = random.Random(q + 1)
    rq = bound(q)
    comps = [0, q // 2, -(q // 2), 32768, -32769, 65535 << 14] + [rng.randint(-(q // 2), q // 2) for _ in range(40)]
    sums = digit_sums(rng)[:24] + digit_sums(rng)[-100:]
    for v in comps:
        v0, v2 = split(v)
        assert v0 + (v2 << 16) == v and abs(v0) <= 1 << 15 and abs(v2) <= (1 << 14) + 1
        for c0, c1, c2, c3 in sums:
            T = c0 + (c1 << 8) + ((c2 + (c3 << 8)) << 16) + v
            r = s32(recomb_q(c0 + v0, c1, c2 + v2, c3, q, True) - 0x80808080)
            assert (r - T) % q == 0
            assert abs(r) <= rq
            assert pack_roundtrip(r) == r


@pytest.mark.parametrize("q", ALL_PRIMES)
def test_consumers_at_the_bound(q):
    """The second step of a two-step pass (a twist |t| <= q/2) and k_mf_mul's
    product epilogue (two last-pass outputs), operands at the bound and at
    the model's own extremes."""
    rng = random.Random(q + 2)
    nqinv = (-pow(q, -1, 1 << 32)) % (1 << 32)
    rq = bound(q)
    ext = sorted(recomb_q(*cs, q, False) for cs in digit_sums(rng))
    ops = [rq, -rq, ext[0], ext[-1]] + [rng.randint(-rq, rq) for _ in range(40)]
    tws = [q // 2, -(q // 2), 1, 0] + [rng.randint(-(q // 2), q // 2) for _ in range(20)]
    for a in ops:
        for b in tws + ops:
            p = a * b
            m = s32((p & 0xFFFFFFFF) * nqinv)
            assert abs(p + m * q) < 1 << 63
            x = redc(p, q, nqinv)
            assert (x * (1 << 32) - p) % q == 0
            assert abs(x) <= PACK_HI and pack_roundtrip(x) == x
            lim = rq * (q // 2 if b in tws else rq) // (1 << 32) + q // 2 + 1
            assert abs(x) <= lim < PACK_HI


def test_not_for_canon():
    """Why the passes before canon() keep the Montgomery form: r leaves
    (-q/2 - 2^14, q/2 + 2^14) for every prime, and the bound leaves (-q, q)
    for the smaller ones."""
    for q in ALL_PRIMES:
        rng = random.Random(q + 3)
        worst = max(abs(recomb_q(*cs, q, False)) for cs in digit_sums(rng))
        assert worst > q // 2 + (1 << 14)
    assert bound(SMALLEST_31) >= SMALLEST_31
    assert bound(PRIMES[16]) >= PRIMES[16] and bound(PRIMES[17]) >= PRIMES[17]
