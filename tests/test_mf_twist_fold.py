"""The folded recombine-and-twist of the matrix-core passes (rnt_mfma.hip,
recomb_tw) as a Python-integer model, against the two-step form it replaces.

Two-step (a recombination, then the twist as a signed Montgomery product):
    r = REDC(lo + 2^16 hi)          lo = C0 + 2^8 C1, hi = C2 + 2^8 C3
    x = REDC(r tw + K)              tw = centred(t 2^32 mod q)
Folded (one reduction):
    x = REDC(lo twA + hi twB + K)   twA = centred(t), twB = centred(t 2^16 mod q)
Both give T t 2^-32 mod q for T = lo + 2^16 hi.  Checked here: the congruence,
|p| < 2^62 for the folded 64-bit sum p, and that the folded word lies in the
packed range [-0x80808080, 0x7F7F7F7F] (so its four balanced byte digits give
it back).  Needs no GPU and no library.
"""
import itertools
import random

import pytest

N = 1 << 16
K32 = 0x80808080
PACK_LO, PACK_HI = -0x80808080, 0x7F7F7F7F
CMAX = 1 << 20  # |digit sum| <= 2^20 (64 products of two balanced bytes)
MR_BASES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)


def is_prime(n):
    if n < 2:
        return False
    for p in MR_BASES:
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in MR_BASES:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def generate_primes(bits, count, degree):
    """The first `count` primes below 2^bits that are 1 mod 2 degree, downwards
    (the reference's generate_primes)."""
    step = 2 * degree
    c = ((1 << bits) - 1) // step * step + 1
    if c > (1 << bits) - 1:
        c -= step
    out = []
    while len(out) < count and c >= 1 << (bits - 1):
        if is_prime(c):
            out.append(c)
        c -= step
    assert len(out) == count
    return out


PRIMES = generate_primes(31, 16, N) + generate_primes(30, 1, N) + generate_primes(29, 1, N)


def centred(v, q):
    v %= q
    return v - q if v > q // 2 else v


def s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def redc(p, q, nqinv):
    """Signed Montgomery reduction as the kernel does it: m = the low word of p
    times -q^-1 (a signed 32-bit value), (p + m q) / 2^32 exactly."""
    m = s32((p & 0xFFFFFFFF) * nqinv)
    v = p + m * q
    assert v & 0xFFFFFFFF == 0
    return v >> 32


def pack_roundtrip(x):
    """(x + K32) ^ K32 as a 32-bit word, read back as four balanced byte digits."""
    w = ((x + K32) & 0xFFFFFFFF) ^ K32
    return sum(((((w >> (8 * b)) & 0xFF) ^ 0x80) - 0x80) << (8 * b) for b in range(4))


def digit_sums(rng):
    corners = list(itertools.product((-CMAX, CMAX), repeat=4))
    rand = [tuple(rng.randint(-CMAX, CMAX) for _ in range(4)) for _ in range(200)]
    return corners + rand


def twists(q, rng):
    return [0, 1, q - 1, q // 2, q // 2 + 1] + [rng.randrange(q) for _ in range(8)]


@pytest.mark.parametrize("q", PRIMES)
def test_folded_reduction_matches_two_step(q):
    assert q % (2 * N) == 1 and is_prime(q)
    rng = random.Random(q)
    nqinv = (-pow(q, -1, 1 << 32)) % (1 << 32)
    # the host check of mf_build for the folded passes
    assert ((1 << 28) + (1 << 20)) * q / 2.0**32 + q / 2.0 + 1 < PACK_HI
    worst_p = worst_x = 0
    for t in twists(q, rng):
        tw = centred(t << 32, q)
        twA, twB = centred(t, q), centred(t << 16, q)
        for c0, c1, c2, c3 in digit_sums(rng):
            lo, hi = c0 + (c1 << 8), c2 + (c3 << 8)
            assert s32(lo) == lo and s32(hi) == hi
            T = lo + (hi << 16)
            r = redc(T, q, nqinv)
            two = redc(r * tw, q, nqinv)
            p = lo * twA + hi * twB
            x = redc(p, q, nqinv)
            assert (x - two) % q == 0
            assert (x * (1 << 32) - T * t) % q == 0
            assert abs(p) < 1 << 62
            assert PACK_LO <= x <= PACK_HI
            assert pack_roundtrip(x) == x
            # the analytic bound: |p| / 2^32 + |m q| / 2^32, |m| <= 2^31
            assert abs(x) <= ((1 << 28) + (1 << 20)) * q // (1 << 32) + q // 2 + 2
            worst_p, worst_x = max(worst_p, abs(p)), max(worst_x, abs(x))
    print(f"q={q}: max |p| = 2^{worst_p.bit_length()}, max |x|/q = {worst_x / q:.4f}")


def test_prime_set():
    assert len(PRIMES) == 18 and len(set(PRIMES)) == 18
    assert [p.bit_length() for p in PRIMES] == [31] * 16 + [30, 29]
    assert PRIMES[0] == max(PRIMES)
