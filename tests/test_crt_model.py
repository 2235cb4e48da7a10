"""k_crt's word arithmetic (crt_model.py) against the exact centred CRT, on
every basis of the GPU test (test_gpu_crt.py): six MW tiers, both word widths.

  - With k = floor(sum s_l / q_l) and one either side of it the model returns
    the exact centred value, as `words` = what holds it, 64 (sign extension)
    and 1 (truncation): the +-Q correction covers an estimate one off.
  - floor of the double-precision estimate is one of those three values,
    whichever way the device rounds `f += s * rq` (every product on its own,
    or one fused multiply-add per step).  The largest |f - exact| per basis is
    printed beside L 2^-52 max(f); a second correction would be needed only
    where the error reaches 1.
  - The shared inputs catch a `>=` centring compare (on floor(Q/2) alone) and
    a missing +Q step (on small negative values), on every basis.
  - With the high half's carry placed one word low, as the kernel had it, the
    u64 bases whose Q nearly fills its MW words come back wrong and every u32
    basis stays exact: what the bug was.
Needs no GPU and no library.
"""
import math

import pytest

import crt_model as cm
from test_mf_twist_fold import generate_primes, is_prime

_cache = {}


def setup(base):
    """(constants, inputs, expected, s per input, accumulators) of a row,
    computed once."""
    name = base[0]
    if name not in _cache:
        mods = cm.base_moduli(base, generate_primes)
        c = cm.CrtConsts(mods, base[1])
        xs, want = cm.input_values(c.Q, name)
        ss = [cm.shoup_s(c, r) for r in cm.residues(xs, mods)]
        _cache[name] = (c, xs, want, ss, [cm.accumulate(c, s) for s in ss])
    return _cache[name]


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_basis_is_what_the_table_says(base):
    name, wide, _, _, mw, bits = base
    mods = cm.base_moduli(base, generate_primes)
    assert len(set(mods)) == len(mods)
    assert all(is_prime(q) and q % (2 * cm.N) == 1 for q in mods)
    assert wide == any(q >= 1 << 31 for q in mods)
    c = cm.CrtConsts(mods, wide)
    assert (c.mw, c.Q.bit_length()) == (mw, bits)
    assert cm.exact_words(c) <= 64
    if name in cm.NEAR_FULL_U64:
        assert 32 * mw - bits <= 4


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_model_is_exact_for_k_within_one(base):
    c, xs, want, ss, accs = setup(base)
    ew = cm.exact_words(c)
    for x, v, s, acc in zip(xs, want, ss, accs):
        assert all(0 <= sl < q for sl, q in zip(s, c.mods))
        assert [sl * (c.Q // q) % q for sl, q in zip(s, c.mods)] == [x % q for q in c.mods]
        kt = cm.k_true(c, s)
        for k in (kt - 1, kt, kt + 1):
            if k < 0:
                continue  # floor of a sum of non-negative terms
            assert cm.signed(cm.finish(c, acc, k, ew)) == v, (x, k - kt)
            assert cm.signed(cm.finish(c, acc, k, 64)) == v, (x, k - kt)
            assert cm.finish(c, acc, k, 1)[0] == v & 0xFFFFFFFFFFFFFFFF, (x, k - kt)


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_double_estimate_is_within_one(base):
    c, xs, _, ss, _ = setup(base)
    L = len(c.mods)
    worst = 0.0
    fmax = 0.0
    for x, s in zip(xs, ss):
        f_sep, f_fma, exact = cm.estimates(c, s)
        kt = cm.k_true(c, s)
        assert kt == math.floor(exact) and kt < L
        for f in (f_sep, f_fma):
            assert math.floor(f) in (kt - 1, kt, kt + 1), (x, f, kt)
            assert 0 <= math.floor(f) < 1 << 32  # k = (uint32_t)f
            worst = max(worst, abs(float(cm.Fraction(f) - exact)))
        fmax = max(fmax, f_sep, f_fma)
    bound = L * 2.0 ** -52 * fmax
    print(f"{base[0]}: L = {L}, max |f - exact| = {worst:.3e}, L 2^-52 max(f) = {bound:.3e}, max(f) = {fmax:.3f}")
    # per term (< 1) three roundings of 2^-53 ((double)s, rq, the product; the
    # fused form drops one), per partial sum (<= max(f)) one: at most
    # L 2^-53 (3 + max(f)) <= 2 L 2^-52 max(f) once max(f) >= 1
    assert fmax >= 1 and worst <= 2 * bound < 1e-9


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_inputs_tell_the_mutants_apart(base):
    """What the shared inputs are for: a `>=` centring compare shows on the
    floor(Q/2) coefficient alone, and without the +Q step the small negative
    values (whose estimate rounds up to an integer) come back wrong, with
    either rounding of the estimate."""
    c, xs, want, ss, accs = setup(base)
    ew = cm.exact_words(c)
    ge = [i for i, (v, s, acc) in enumerate(zip(want, ss, accs))
          if cm.signed(cm.finish(c, acc, cm.k_true(c, s), ew, ge_centre=True)) != v]
    assert ge == [5] and xs[5] == c.Q // 2
    for which in (0, 1):
        bad = [i for i, (v, s, acc) in enumerate(zip(want, ss, accs))
               if cm.signed(cm.finish(c, acc, math.floor(cm.estimates(c, s)[which]), ew, plus_q=False)) != v]
        assert bad and all(xs[i] < 0 for i in bad)
        assert sum(1 for i in bad if i < 10 + cm.SMALL) >= 8, bad


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_parent_carry_placement(base):
    """The regression pin: the carry out of the high-half product loop added
    to acc[MW - 1] instead of acc[MW]."""
    c, xs, want, ss, accs = setup(base)
    ew = cm.exact_words(c)
    bad = 0
    for v, s, acc in zip(want, ss, accs):
        old = cm.accumulate(c, s, parent_carry=True)
        if not c.wide:
            assert old == acc  # one half: the loop bounds coincide
        bad += cm.signed(cm.finish(c, old, cm.k_true(c, s), ew)) != v
    print(f"{base[0]}: {bad} / {len(xs)} wrong with the carry one word low")
    if base[0] in cm.NEAR_FULL_U64:
        assert bad >= 20
        assert want[0] == 0 and cm.signed(cm.finish(c, cm.accumulate(c, ss[0], True), 0, ew)) == 0
    elif not c.wide:
        assert bad == 0
