"""rnt_mod_raise on the GPU, word for word against Python integers
(tests/homdft_ref.py mod_raise_ref: the centred CRT value, then % q_j).

Every case plants the boundary values of the centring as residues at the edge
coefficients 0, 1, N - 1: the first poly takes 0, 1 and Q0 - 1 there, the last
poly floor(Q0/2), floor(Q0/2) + 1 and the all-(q_i - 1) vector; a case with one
poly takes the second triple at coefficients 2, 3, N - 2.  Each case runs with
its input on a drop_last view of the output's context and on an unrelated root
over the same moduli.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from homdft_ref import mod_raise_ref
from test_gpu_unaligned import guards, shifted

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED, DOMAIN, BASIS = 11, 12, 7, 8

# (log_n, moduli kind, l0, L, B)
CASES = ([(8, "31", l0, l0 + 1, 3) for l0 in (1, 2, 3, 4)] + [(8, "31", l0, 7, 1) for l0 in (1, 2)] +
         [(12, "61", l0, 5, 2) for l0 in (1, 2)] + [(12, "mixed", l0, 5, 2) for l0 in (1, 2)] +
         [(14, "31", 2, 16, 2), (14, "31", 2, 16, 64)])


def moduli_of(kind, L, n):
    if kind == "31":
        return orc.generate_primes(31, L, n)
    if kind == "61":
        return orc.generate_primes(61, L, n)
    a, b = orc.generate_primes(40, L, n), orc.generate_primes(61, L, n)
    return [(a if i % 2 == 0 else b)[i // 2] for i in range(L)]  # 40-, 61-, 40-bit, ...


def planted_input(mod, l0, n, B, rng):
    """[B][l0][N] uniform residues with the boundary values planted."""
    q = [int(v) for v in mod[:l0]]
    Q0 = 1
    for v in q:
        Q0 *= v
    x = orc.uniform_poly(q, n, rng, batch=B)
    res = lambda v: [v % m for m in q]  # noqa: E731
    first = [res(0), res(1), res(Q0 - 1)]
    last = [res(Q0 // 2), res(Q0 // 2 + 1), [m - 1 for m in q]]
    for pos, r in zip((0, 1, n - 1), first):
        x[0, :, pos] = r
    for pos, r in zip((0, 1, n - 1) if B > 1 else (2, 3, n - 2), last):
        x[B - 1, :, pos] = r
    return x


def fast_ref(x, mod, l0):
    """The whole batch in int64 where Q0 < 2^62 (one or two 31-bit limbs):
    x = x0 + q0 ((x1 - x0) q0^-1 mod q1), centred, mod every q_j."""
    q = [int(v) for v in mod]
    x = x.astype(np.int64)
    v, Q0 = x[:, 0], q[0]
    if l0 == 2:
        inv = pow(q[0] % q[1], -1, q[1])
        v = v + q[0] * (((x[:, 1] - x[:, 0]) % q[1]) * inv % q[1])
        Q0 *= q[1]
    v = np.where(v > Q0 // 2, v - Q0, v)
    return np.stack([np.mod(v, m) for m in q], axis=1).astype(np.uint64)


@pytest.mark.parametrize("placement", ["view", "root"])
@pytest.mark.parametrize("log_n,kind,l0,L,B", CASES, ids=[f"n{c[0]}-{c[1]}-l{c[2]}-L{c[3]}-B{c[4]}" for c in CASES])
def test_mod_raise_matches_python_integers(gpu, log_n, kind, l0, L, B, placement):
    rn = gpu
    n = 1 << log_n
    mod = moduli_of(kind, L, n)
    rng = np.random.default_rng(1000 * log_n + 10 * l0 + L)
    top = rn.RnsBasis(mod, n)
    low = top.drop_last(L - l0) if placement == "view" else rn.RnsBasis(mod[:l0], n)
    x = planted_input(mod, l0, n, B, rng)
    src = rn.RnsPoly.from_channels(x, low)
    top.profile_enable(True)
    try:
        out = src.mod_raise(top)
        launches = top.profile_read("mod_raise")[0]
    finally:
        top.profile_enable(False)
    assert launches == 1  # pure streaming: one launch
    assert out.basis is top and out.n_polys == B and not out.is_ntt_domain()
    got = out.channels_batch()
    for b in sorted({0, B // 2, B - 1}):
        assert np.array_equal(got[b], mod_raise_ref(x[b], mod[:l0], mod)), f"poly {b} differs from the integers"
    assert np.array_equal(got[:, :l0], x)  # the input's own limbs are its words
    if kind == "31" and l0 <= 2:
        assert np.array_equal(got, fast_ref(x, mod, l0))  # every poly of the batch
    assert np.array_equal(src.channels_batch(), x)  # the input is unchanged


def test_mod_raise_on_word_aligned_buffers(gpu):
    """Both buffers one word past a 16-byte boundary (the one-word kernel
    form), between guard words that must not change."""
    rn = gpu
    n, l0, L, B = 256, 2, 7, 3
    mod = moduli_of("31", L, n)
    top = rn.RnsBasis(mod, n)
    low = top.drop_last(L - l0)
    x = planted_input(mod, l0, n, B, np.random.default_rng(5))
    src = shifted(rn, low, x)
    out = shifted(rn, top, B)
    rn.check(rn.load().rnt_mod_raise(out.handle, src.handle))
    got = out.channels_batch()
    for b in range(B):
        assert np.array_equal(got[b], mod_raise_ref(x[b], mod[:l0], mod))
    assert np.array_equal(src.channels_batch(), x)
    guards(src, out)


def test_mod_raise_refusals_leave_the_output_untouched(gpu):
    rn = gpu
    lib = rn.load()
    n, L, B = 256, 6, 2
    mod = moduli_of("31", L, n)
    top = rn.RnsBasis(mod, n)
    rng = np.random.default_rng(6)
    sentinel = np.broadcast_to(np.array(mod, dtype=np.uint64)[None, :, None] - np.uint64(2), (B, L, n)).copy()
    out = rn.RnsPoly.from_channels(sentinel, top)

    def refused(o, i, status, fields=None):
        rc = lib.rnt_mod_raise(o.handle if o is not None else None, i.handle if i is not None else None)
        assert rc == status, (rc, lib.rnt_last_error())
        if fields is not None:
            raw = (ctypes.c_uint64 * 2)(7, 7)
            assert lib.rnt_last_error_detail(raw) == status and tuple(raw) == fields
        assert np.array_equal(out.channels_batch(), sentinel)

    def inp(basis, b=B, ntt=False):
        return rn.RnsPoly.from_channels(orc.uniform_poly(basis.moduli(), n, rng, batch=b), basis, in_ntt_domain=ntt)

    good = inp(top.drop_last(L - 2))
    other = orc.generate_primes(30, 2, n)
    refused(out, inp(rn.RnsBasis(other, n)), BASIS)  # the moduli prefix differs
    refused(out, inp(rn.RnsBasis([mod[0], other[0]], n)), BASIS)  # ... in its second limb
    mod_big = orc.generate_primes(31, 2, 2 * n)
    refused(out, rn.RnsPoly(rn.RnsBasis(mod_big, 2 * n), B), BASIS)  # another degree
    refused(out, inp(top), BAD_ARGUMENT)  # l0 == L
    refused(rn.RnsPoly.from_channels(sentinel[:, :2], top.drop_last(L - 2)), inp(top.drop_last(1)), BAD_ARGUMENT)  # l0 > L
    refused(out, inp(top.drop_last(L - 2), b=B + 1), BAD_ARGUMENT)  # batch sizes differ
    refused(None, good, BAD_ARGUMENT)
    refused(out, None, BAD_ARGUMENT)
    refused(out, inp(top.drop_last(1)), UNSUPPORTED, (0, 0))  # l0 = 5 > 4
    refused(out, inp(top.drop_last(L - 2), ntt=True), DOMAIN)
    # different device word widths: a u32 input basis, a u64 output basis with the same first modulus
    wide = rn.RnsBasis([mod[0], orc.generate_primes(61, 1, n)[0]], n)
    wout = rn.RnsPoly(wide, B)
    narrow = inp(rn.RnsBasis(mod[:1], n))  # (held: a temporary would be freed before the call reads its handle)
    rc = lib.rnt_mod_raise(wout.handle, narrow.handle)
    raw = (ctypes.c_uint64 * 2)(7, 7)
    assert rc == UNSUPPORTED and lib.rnt_last_error_detail(raw) == UNSUPPORTED and tuple(raw) == (0, 0)
    assert not wout.channels_batch().any()
    # a key level view in any position
    emod = rn.generate_primes(30, 4, n)
    ext = rn.RnsBasis(emod, n)
    ka, kb = (orc.uniform_poly(emod, n, rng, batch=2) for _ in range(2))
    view = rn.RnsHybridKey.from_channels(ka, kb, ext, 2, n_special=1).at_level(2).a
    refused(out, view, UNSUPPORTED)
    refused(view, good, UNSUPPORTED)
    # and the call still works afterwards
    rn.check(lib.rnt_mod_raise(out.handle, good.handle))
    assert np.array_equal(out.channels_batch()[0], mod_raise_ref(good.channels_batch()[0], mod[:2], mod))
