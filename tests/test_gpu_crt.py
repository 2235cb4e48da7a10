"""The centred CRT kernel (k_crt: rnt_to_coeffs, rnt_crt_centered, rnt_decode)
on every MW tier and both word widths, against Python ints.

One basis per row of crt_model.BASES, N = 8, 24 polys = 192 coefficients:
the centring boundary from both sides, 0, +-1, +-2, 64 small signed values and
uniform ones, every coefficient compared.  Coefficient i of the upload is
input_values()[i]: 0..9 the edge values (5 is floor(Q/2), 9 is floor(Q/2) + 1),
10..73 the small ones, 74.. the uniform ones; a failure names the indices.
The u64 rows whose Q nearly fills its MW words are the ones a carry out of the
high half's product loop reaches (crt_model.py, test_crt_model.py).
"""
from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest

import crt_model as cm
import encoder as enc

pytestmark = pytest.mark.gpu

N = cm.N
M64 = (1 << 64) - 1
_rows = {}


def _upload(rn, xs, mods, basis):
    """[B][L][N] residues of xs (coefficient i -> poly i // N, slot i % N)."""
    ch = np.array([[[xs[b * N + j] % q for j in range(N)] for q in mods] for b in range(len(xs) // N)],
                  dtype=np.uint64)
    return rn.RnsPoly.from_channels(ch, basis), ch


def _row(rn, base):
    """Context, inputs, expected values and the uploaded batch of a row, made
    once and left unchanged."""
    name = base[0]
    if name not in _rows:
        mods = cm.base_moduli(base, rn.generate_primes)
        Q = cm.product(mods)
        xs, want = cm.input_values(Q, name)
        basis = rn.RnsBasis(mods, N)
        poly, ch = _upload(rn, xs, mods, basis)
        _rows[name] = dict(mods=mods, Q=Q, xs=xs, want=want, basis=basis, poly=poly, ch=ch,
                           consts=cm.CrtConsts(mods, base[1]))
    return _rows[name]


def _flat(nested):
    return [v for row in nested for v in row]


def _low64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def _check(got, want, what):
    got = [int(g) for g in got]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, f"{what}: {len(bad)} of {len(want)} wrong, at {bad[:16]}"


def _crt_raw(rn, p, words):
    raw = np.zeros((p.n_polys * N, words), dtype=np.uint64)
    rn._lib.check(rn.load().rnt_crt_centered(p.handle, raw.ctypes.data_as(ctypes.c_void_p), p.n_polys, words))
    return raw


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_every_coefficient_exact(gpu, base):
    r = _row(gpu, base)
    c = r["consts"]
    assert (c.mw, r["Q"].bit_length()) == (base[4], base[5])
    assert r["basis"].moduli() == r["mods"]
    p = r["poly"]
    _check(_flat(p.to_coeffs_exact()), r["want"], "to_coeffs_exact")
    _check(p.to_coeffs().reshape(-1), [_low64(v) for v in r["want"]], "to_coeffs")
    assert not p.is_ntt_domain() and np.array_equal(p.channels(), r["ch"])


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_from_ntt_domain_copy(gpu, base):
    """An NTT-domain input decodes through a temporary copy: same values, the
    input unchanged and still in the NTT domain."""
    r = _row(gpu, base)
    t = r["poly"].clone()
    t.to_ntt_domain()
    before = t.channels()
    _check(_flat(t.to_coeffs_exact()), r["want"], "to_coeffs_exact (NTT domain)")
    _check(t.to_coeffs().reshape(-1), [_low64(v) for v in r["want"]], "to_coeffs (NTT domain)")
    assert t.is_ntt_domain() and np.array_equal(t.channels(), before)
    t.to_coeff_domain()
    assert np.array_equal(t.channels(), r["ch"])


@pytest.mark.parametrize("base", cm.BASES, ids=cm.BASE_IDS)
def test_crt_centered_word_counts(gpu, base):
    """rnt_crt_centered itself: 64 words (sign extension above the MW / 2
    words of Q; on the MW = 128 rows exactly what holds the value) and one."""
    rn = gpu
    r = _row(rn, base)
    mw = r["consts"].mw
    if mw == 128:
        assert cm.exact_words(r["consts"]) == 64
    raw = _crt_raw(rn, r["poly"], 64)
    _check([cm.signed(row) for row in raw], r["want"], "words = 64")
    neg = [i for i, v in enumerate(r["want"]) if v < 0]
    assert len(neg) > 40
    for i, v in enumerate(r["want"]):
        ext = M64 if v < 0 else 0
        assert all(int(w) == ext for w in raw[i, mw // 2:]), f"sign extension of coefficient {i}"
    one = _crt_raw(rn, r["poly"], 1)
    _check(one[:, 0], [v & M64 for v in r["want"]], "words = 1")


# a parent basis one limb longer than the row, so that its Q needs the next MW
# tier: (row, (bits, index) of the extra prime in generate_primes' order)
VIEW_ROWS = [("u32-31x16+p16", (31, 16)), ("u64-62x8+p16", (62, 8)), ("u64-62x16+p31", (62, 16)),
             ("u64-62x33", (62, 33))]


@pytest.mark.parametrize("name,extra", VIEW_ROWS, ids=[v[0] for v in VIEW_ROWS])
def test_drop_last_view_in_another_tier(gpu, name, extra):
    """One context, two entries of the per-L constants cache: the parent's Q
    is in the tier above, its drop_last(1) view's Q is the row's (nearly a
    full MW words).  Both exact over their own moduli, in either order."""
    rn = gpu
    base = cm.BASES[cm.BASE_IDS.index(name)]
    vmods = cm.base_moduli(base, rn.generate_primes)
    bits, at = extra
    mods = vmods + [rn.generate_primes(bits, at + 1, N)[at]]
    assert len(set(mods)) == len(mods)
    Qv, Qp = cm.product(vmods), cm.product(mods)
    assert cm.CrtConsts(mods, base[1]).mw == 2 * cm.CrtConsts(vmods, base[1]).mw == 2 * base[4]
    xs, _ = cm.input_values(Qv, name)
    rng = random.Random(name + " parent")
    xs[-32:] = [rng.randint(-(Qp // 2), Qp // 2) for _ in range(32)]
    parent = rn.RnsBasis(mods, N)
    p, _ = _upload(rn, xs, mods, parent)
    want_p = [cm.centred(x, Qp) for x in xs]
    want_v = [cm.centred(x, Qv) for x in xs]
    assert want_p == xs and want_v[-32:] != xs[-32:]
    _check(_flat(p.to_coeffs_exact()), want_p, "parent")
    v = p.mod_drop_last(1)
    assert v.basis.moduli() == vmods
    _check(_flat(v.to_coeffs_exact()), want_v, "view")
    _check(v.to_coeffs().reshape(-1), [_low64(x) for x in want_v], "view, to_coeffs")
    _check(_flat(p.to_coeffs_exact()), want_p, "parent after the view")
    v.to_ntt_domain()
    _check(_flat(v.to_coeffs_exact()), want_v, "view (NTT domain)")


@pytest.mark.parametrize("name", ["u32-31x16+p16", "u64-62x8+p16"])
def test_decode_on_a_long_basis(gpu, name):
    """rnt_decode on more than four limbs, Q nearly a full MW words:
    test_decode_matches_oracle's inputs, reference and tolerance."""
    rn = gpu
    r = _row(rn, cm.BASES[cm.BASE_IDS.index(name)])
    rng = np.random.default_rng(len(r["mods"]))
    B = 3
    a = rng.integers(-(2 ** 40), 2 ** 40, (B, N))
    poly = rn.RnsPoly.from_coeffs(a, r["basis"])
    assert np.array_equal(poly.to_coeffs(), a)
    scale = 25
    for slots in (N // 2, 3):
        z = rn.CkksEncoder(N, scale).decode_complex(rn.Plaintext(poly, scale, slots))
        for p in range(B):
            want = enc.decode_fft(a[p], N, scale, slots)
            assert np.allclose(z[p], want, atol=1e-9 * np.max(np.abs(want)), rtol=0)
    t = poly.clone()
    t.to_ntt_domain()
    zt = rn.CkksEncoder(N, scale).decode_complex(rn.Plaintext(t, scale, N // 2))
    z0 = rn.CkksEncoder(N, scale).decode_complex(rn.Plaintext(poly, scale, N // 2))
    assert np.array_equal(zt, z0)
    assert t.is_ntt_domain()


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------


def _refused(rn, call, *needles):
    with pytest.raises(rn.RnsNttError) as e:
        rn._lib.check(call())
    assert e.value.kind == "BadArgument"
    for s in needles:
        assert s in str(e.value), str(e.value)


def test_q_of_129_words_is_refused(gpu):
    """31 x 133: the context is created and transforms; the CRT names its
    128-word limit."""
    rn = gpu
    mods = rn.generate_primes(31, 133, N)
    assert -(-cm.product(mods).bit_length() // 32) == 129
    basis = rn.RnsBasis(mods, N)
    rng = np.random.default_rng(133)
    ch = np.stack([rng.integers(0, q, (2, N), dtype=np.uint64) for q in mods], axis=1)
    p = rn.RnsPoly.from_channels(ch, basis)
    p.to_ntt_domain()
    assert p.is_ntt_domain() and not np.array_equal(p.channels(), ch)
    p.to_coeff_domain()
    assert np.array_equal(p.channels(), ch)
    lib = rn.load()
    out = np.zeros((2, N), dtype=np.int64)
    _refused(rn, lambda: lib.rnt_to_coeffs(p.handle, out.ctypes.data_as(ctypes.c_void_p), 2),
             "Q has 129 32-bit words", "max 128")
    z = np.zeros((2, N // 2), dtype=np.complex128)
    _refused(rn, lambda: lib.rnt_decode(p.handle, z.ctypes.data_as(ctypes.c_void_p), N // 2, 25),
             "Q has 129 32-bit words", "max 128")
    # the largest basis that is served sits right below
    q = rn.RnsPoly.from_channels(ch[:, :132], basis.drop_last(1))
    want = [cm.centered_crt(mods[:132], ch[b, :132, j]) for b in range(2) for j in range(N)]
    _check(_flat(q.to_coeffs_exact()), want, "31 x 132 view")


def test_bad_arguments_are_refused(gpu):
    rn = gpu
    r = _row(rn, cm.BASES[0])
    p = r["poly"]
    lib = rn.load()
    B = p.n_polys
    buf = np.zeros((B * N, 65), dtype=np.uint64)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    for words in (0, 65):
        _refused(rn, lambda: lib.rnt_crt_centered(p.handle, ptr, B, words), "rnt_crt_centered", "1..64 words")
    for n_polys in (B - 1, B + 1, 0):
        _refused(rn, lambda: lib.rnt_crt_centered(p.handle, ptr, n_polys, 4), "rnt_crt_centered",
                 f"buffer holds {B} polys, got {n_polys}")
        _refused(rn, lambda: lib.rnt_to_coeffs(p.handle, ptr, n_polys), "rnt_to_coeffs",
                 f"buffer holds {B} polys, got {n_polys}")
    _refused(rn, lambda: lib.rnt_crt_centered(p.handle, None, B, 4), "rnt_crt_centered", "null host pointer")
    _refused(rn, lambda: lib.rnt_to_coeffs(p.handle, None, B), "rnt_to_coeffs", "null host pointer")
    assert not buf.any()
    # and the batch still decodes
    _check(_flat(p.to_coeffs_exact()), r["want"], "after the refusals")


@pytest.mark.parametrize("bits", [31, 62])
def test_repeated_modulus_is_refused(gpu, bits):
    """rnt_ctx_create does not accept a basis that is not pairwise coprime,
    so no CRT over one can be asked for."""
    rn = gpu
    a, b = rn.generate_primes(bits, 2, N)
    for mods in ([a, b, a], [a, a], [b, a, 97, a]):
        with pytest.raises(rn.RnsNttError) as e:
            rn.RnsBasis(mods, N)
        assert e.value.kind == "BadArgument"
        assert f"moduli {a} and {a} are not coprime" in str(e.value)
