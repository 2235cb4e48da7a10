"""The decode-side CRT kernel (rnt_kernels.hip, k_crt) as a Python-integer
model, with the bases and inputs its tests share.

Per coefficient with residues r_l the kernel computes
    s_l = r_l inv_l mod q_l                  (a Shoup product, inv_l = (Q/q_l)^-1)
    acc = sum_l s_l (Q/q_l)                  (MW + 1 words of 32 bits; a u64 s_l
                                              goes in as two 32-bit halves)
    acc -= k Q,  k = floor(sum_l s_l / q_l)  (k from a double-precision sum; the
                                              top word wraps)
    acc += Q if acc < 0;  acc -= Q if acc >= Q
    acc -= Q if acc > floor(Q/2)             (centred into (-Q/2, Q/2])
and writes `out_words` little-endian 64-bit two's-complement words.
shoup_s(), accumulate() and finish() below restate that word for word, loop
index for loop index, from the constants crt_tables (rnt_api.cpp) uploads
(CrtConsts).  The quotient k is a parameter of finish(): the device may
contract `f += s * rq` into a fused multiply-add, so a host double cannot
predict its floor(f); estimates() gives both roundings.

accumulate(parent_carry=True) places the carry that leaves the high-half
product loop where the kernel once had it (into acc[MW - 1], one word low).
Needs no GPU and no library.
"""
import random
from fractions import Fraction

M32 = 0xFFFFFFFF
N = 8  # the ring of the CRT tests: the kernel works per coefficient
POLYS = 24  # polys per upload: 192 coefficients

# (id, u64 words?, [(prime bits, count)...] largest first by generate_primes,
#  named small primes appended, MW tier, bits of Q)
BASES = [
    ("u32-31x8+97", False, [(31, 8)], [97], 8, 255),
    ("u32-31x16+p16", False, [(31, 16), (16, 1)], [], 16, 512),
    ("u32-31x33", False, [(31, 33)], [], 32, 1023),
    ("u32-31x66", False, [(31, 66)], [], 64, 2046),
    ("u32-31x132", False, [(31, 132)], [], 128, 4092),
    ("u32-30x17", False, [(30, 17)], [], 16, 510),
    ("u64-61+62+17", True, [(61, 1), (62, 1)], [17], 4, 128),
    ("u64-63x2", True, [(63, 2)], [], 4, 126),
    ("u64-62x4+97", True, [(62, 4)], [97], 8, 255),
    ("u64-62x8+p16", True, [(62, 8), (16, 1)], [], 16, 512),
    ("u64-62x16+p31", True, [(62, 16), (31, 1)], [], 32, 1023),
    ("u64-62x33", True, [(62, 33)], [], 64, 2046),
    ("u64-62x66", True, [(62, 66)], [], 128, 4092),
    ("u64-63x65", True, [(63, 65)], [], 128, 4095),
]
BASE_IDS = [b[0] for b in BASES]
# u64 bases whose Q comes within a few bits of 2^(32 MW): the carry leaves the
# high-half loop on them
NEAR_FULL_U64 = ["u64-62x4+97", "u64-62x8+p16", "u64-62x16+p31", "u64-62x33", "u64-62x66", "u64-63x65"]


def base_moduli(base, generate_primes):
    """The moduli of a BASES row; generate_primes(bits, count, degree) is the
    library's or a Python restatement of it."""
    _, _, groups, named, _, _ = base
    mods = []
    for bits, count in groups:
        mods += [int(q) for q in generate_primes(bits, count, N)]
    return mods + list(named)


def product(mods):
    Q = 1
    for q in mods:
        Q *= q
    return Q


def centered_crt(mods, residues):
    """The exact centred CRT value in Python ints."""
    Q = product(mods)
    x = 0
    for r, q in zip(residues, mods):
        Qi = Q // q
        x += (int(r) * pow(Qi % q, -1, q) % q) * Qi
    x %= Q
    return x - Q if x > Q // 2 else x


def centred(x, Q):
    x %= Q
    return x - Q if x > Q // 2 else x


SMALL = 64


def input_values(Q, seed, count=N * POLYS):
    """(x to upload as residues x mod q_l, the centred value expected back):
    ten edge values (0, +-1, +-2, the centring boundary from both sides, and
    floor(Q/2) + 1, which is -floor(Q/2)), 64 small signed values, the rest
    uniform in (-Q/2, Q/2]."""
    h = Q // 2
    rng = random.Random(seed)
    xs = [0, 1, -1, 2, -2, h, -h, h - 1, 1 - h, h + 1]
    xs += [rng.randint(-999, 999) for _ in range(SMALL)]
    xs += [rng.randint(-h, h) for _ in range(count - len(xs))]
    assert len(xs) == count
    return xs, [centred(x, Q) for x in xs]


def residues(xs, mods):
    """[len(xs)][L] canonical residues."""
    return [[x % q for q in mods] for x in xs]


def to_words(v, n):
    return [(v >> (32 * w)) & M32 for w in range(n)]


class CrtConsts:
    """What crt_tables computes on the host for the first L limbs."""

    def __init__(self, mods, wide):
        self.mods = list(mods)
        self.wide = wide
        self.wbits = 64 if wide else 32
        self.Q = product(mods)
        words = max(1, -(-self.Q.bit_length() // 32))
        mw = 4
        while mw < words:
            mw *= 2
        assert mw <= 128, f"Q has {words} 32-bit words (max 128)"
        self.mw = mw
        self.qi = []
        self.inv = []
        self.inv_p = []
        self.rq = []
        for q in mods:
            Qi = self.Q // q
            self.qi.append(to_words(Qi, mw))  # words past MW dropped, as the host copy does
            inv = pow(Qi % q, -1, q) if len(mods) > 1 else 1
            self.inv.append(inv)
            self.inv_p.append((inv << self.wbits) // q)  # shoup_companion
            self.rq.append(1.0 / float(q))
        self.qw = to_words(self.Q, mw)
        self.qh = [(self.qw[w] >> 1) | ((self.qw[w + 1] << 31) & M32 if w + 1 < mw else 0) for w in range(mw)]


def shoup_s(c, res):
    """s_l = shoup_mul(r_l, inv_l, inv_p_l, q_l) in w-bit wrapping words."""
    mask = (1 << c.wbits) - 1
    out = []
    for r, q, w, wp in zip(res, c.mods, c.inv, c.inv_p):
        hi = (r * wp) >> c.wbits
        t = (r * w - hi * q) & mask
        out.append(t - q if t >= q else t)
    return out


def accumulate(c, s, parent_carry=False):
    """acc[MW + 1] = sum_l s_l (Q/q_l), the kernel's loops."""
    MW = c.mw
    acc = [0] * (MW + 1)
    for l, sl in enumerate(s):
        row = c.qi[l]
        for half in range(2 if c.wide else 1):
            sh = (sl >> (32 * half)) & M32
            carry = 0
            for w in range(MW - half):
                t = sh * row[w] + acc[w + half] + carry
                acc[w + half] = t & M32
                carry = t >> 32
            for w in range(MW - half if parent_carry else MW, MW + 1):
                t = acc[w] + carry
                acc[w] = t & M32
                carry = t >> 32
    return acc


def _mw_add(a, b, MW):
    carry = 0
    for w in range(MW):
        t = a[w] + b[w] + carry
        a[w] = t & M32
        carry = t >> 32
    a[MW] = (a[MW] + carry) & M32


def _mw_sub(a, b, MW):
    borrow = 0
    for w in range(MW):
        d = (a[w] - b[w] - borrow) & 0xFFFFFFFFFFFFFFFF
        a[w] = d & M32
        borrow = (d >> 32) & 1
    a[MW] = (a[MW] - borrow) & M32


def _mw_ge(a, b, MW):
    if a[MW] != 0:
        return True
    for w in range(MW - 1, -1, -1):
        if a[w] != b[w]:
            return a[w] > b[w]
    return True


def finish(c, acc, k, out_words, ge_centre=False, plus_q=True):
    """From the accumulator to the output words: subtract k Q, correct,
    centre, sign-extend or truncate.  ge_centre / plus_q=False are the two
    mutants the GPU tests must catch (a >= centring compare, no +Q step)."""
    MW = c.mw
    acc = list(acc)
    k &= M32
    borrow = 0
    carry = 0
    for w in range(MW):
        kq = k * c.qw[w] + carry
        carry = kq >> 32
        d = (acc[w] - (kq & M32) - borrow) & 0xFFFFFFFFFFFFFFFF
        acc[w] = d & M32
        borrow = (d >> 32) & 1
    acc[MW] = (acc[MW] - (carry & M32) - borrow) & M32
    if plus_q and acc[MW] >> 31:
        _mw_add(acc, c.qw, MW)
    if _mw_ge(acc, c.qw, MW):
        _mw_sub(acc, c.qw, MW)
    gt = ge_centre
    for w in range(MW - 1, -1, -1):
        if acc[w] != c.qh[w]:
            gt = acc[w] > c.qh[w]
            break
    if gt:
        _mw_sub(acc, c.qw, MW)
    sign = M32 if acc[MW] >> 31 else 0
    out = []
    for w in range(out_words):
        lo = acc[2 * w] if 2 * w < MW else sign
        hi = acc[2 * w + 1] if 2 * w + 1 < MW else sign
        out.append(lo | (hi << 32))
    return out


def signed(words):
    """Little-endian 64-bit words as a two's-complement Python int."""
    v = 0
    for w in reversed(words):
        v = (v << 64) | int(w)
    n = 64 * len(words)
    return v - (1 << n) if v >> (n - 1) else v


def exact_words(c):
    """64-bit words that hold any centred value of the basis with its sign
    (RnsPoly.to_coeffs_exact's count)."""
    bits = sum(q.bit_length() for q in c.mods)
    return max(1, (bits + 1 + 63) // 64)


def k_true(c, s):
    """floor(sum_l s_l / q_l), exactly."""
    return sum(sl * (c.Q // q) for sl, q in zip(s, c.mods)) // c.Q


def estimates(c, s):
    """(f with every product rounded on its own, f with each step one fused
    multiply-add rounded once, the exact sum): `f += (double)s * rq[l]`."""
    f_sep = 0.0
    f_fma = 0.0
    exact = Fraction(0)
    for sl, q, rq in zip(s, c.mods, c.rq):
        sd = float(sl)  # (double)s: round to nearest even, as the device converts
        f_sep = f_sep + sd * rq
        f_fma = float(Fraction(f_fma) + Fraction(sd) * Fraction(rq))
        exact += Fraction(sl, q)
    return f_sep, f_fma, exact
