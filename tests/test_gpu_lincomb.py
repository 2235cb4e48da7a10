"""rnt_ct_lincomb / rnt_ct_lincomb_rescale (k_lincomb) on the GPU, word for word
against the definition (tests/lincomb_ref.py, pinned in
tests/test_lincomb_ref.py) and against the library's own two-step path
(ct_lincomb(rescale=False) then rescale_ciphertext), and every refusal of the
call with its status and fields.

Shapes.  k_lincomb keeps the inputs of a limb in registers in tiers of 4, 8 and
16 (n_in 4|5 and 8|9 are the boundaries) and loops over the outputs at run time;
the launcher splits the output limbs over blockIdx.y until the grid has
SPLIT_BLOCKS workgroups (``grid_runs`` below mirrors lincomb_t's picker).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from lincomb_ref import lincomb_ref, reduce_weights

pytestmark = pytest.mark.gpu

LOG_N = 10
N = 1 << LOG_N
SPLIT_BLOCKS = 1024  # kSplitBlocks (rnt_kernels.hip)


def grid_runs(B, word_bytes, Lv, rescale):
    """(limb runs, limbs per run) lincomb_t picks: blocks of 256 lanes of one
    16-byte vector each over the B N positions, two components."""
    bx = -(-(B * N // (16 // word_bytes)) // 256)
    lo = Lv - 1 if rescale else Lv
    runs = min(lo, max(SPLIT_BLOCKS // (2 * bx), 1))
    tper = -(-lo // runs)
    return -(-lo // tper), tper


class Case:
    """Random inputs, weights and a bias on `Lv` limbs (optionally the
    drop_last view of a larger root), with the un-rescaled biased reference
    computed once: the other three variants follow from it exactly."""

    def __init__(self, rn, bits, Lv, n_in, n_out, B, seed, view=0, edge=False):
        self.rn, self.Lv, self.n_in, self.n_out, self.B = rn, Lv, n_in, n_out, B
        root_mod = rn.generate_primes(bits, Lv + view, N)
        self.mod = root_mod[:Lv]
        self.Bo = orc.Basis(self.mod, N)
        root = rn.RnsBasis(root_mod, N)
        self.basis = root.drop_last(view) if view else root
        rng = np.random.default_rng(seed)
        if edge:  # every residue q - 1, the weights cycling through 0, 1 and q - 1 (= -1)
            top = np.array(self.mod, dtype=np.uint64)[None, :, None] - np.uint64(1)
            self.x0 = np.broadcast_to(top, (n_in * B, Lv, N)).copy()
            self.x1 = self.x0.copy()
            ints = [[(0, 1, -1)[(i + j) % 3] for i in range(n_in)] for j in range(n_out)]
            bias = [-1] * n_out
        else:
            self.x0 = orc.uniform_poly(self.mod, N, rng, batch=n_in * B)
            self.x1 = orc.uniform_poly(self.mod, N, rng, batch=n_in * B)
            ints = [[int(v) for v in row] for row in rng.integers(-(1 << 62), 1 << 62, size=(n_out, n_in))]
            bias = [int(v) for v in rng.integers(-(1 << 62), 1 << 62, size=n_out)]
        self.ints, self.bias_ints = ints, bias
        self.w, self.bias = reduce_weights(ints, self.mod), reduce_weights(bias, self.mod)
        self.ct = rn.Ciphertext(rn.RnsPoly.from_channels(self.x0, self.basis),
                                rn.RnsPoly.from_channels(self.x1, self.basis), 30, 0)
        self._ref = lincomb_ref(self.Bo, self.x0, self.x1, n_in, self.w, self.bias)

    def reference(self, with_bias, rescale):
        r0, r1 = self._ref
        if not with_bias:  # take the bias off coefficient 0 of component 0 again
            r0 = r0.copy()
            for t, q in enumerate(self.mod):
                for j in range(self.n_out):
                    col = r0[j * self.B:(j + 1) * self.B, t, 0].astype(object)
                    r0[j * self.B:(j + 1) * self.B, t, 0] = np.array((col - int(self.bias[j][t])) % q, dtype=np.uint64)
        if rescale:
            r0, r1 = (np.stack([orc.rescale(self.Bo, p) for p in r]) for r in (r0, r1))
        return r0, r1

    def check(self, with_bias, rescale):
        rn = self.rn
        bias = self.bias_ints if with_bias else None
        got = rn.ct_lincomb(self.ct, self.n_in, self.ints, bias, rescale=rescale)
        want0, want1 = self.reference(with_bias, rescale)
        for o in (got.c0, got.c1):
            assert not o.is_ntt_domain() and o.n_polys == self.n_out * self.B
            assert o.basis.channel_count() == self.Lv - int(rescale)
        assert got.c0.basis is got.c1.basis
        assert np.array_equal(got.c0.channels_batch(), want0), "out0 differs from the definition"
        assert np.array_equal(got.c1.channels_batch(), want1), "out1 differs from the definition"
        if rescale:  # the library's own two-step path, every poly
            two = rn.rescale_ciphertext(rn.ct_lincomb(self.ct, self.n_in, self.ints, bias, rescale=False))
            assert np.array_equal(got.c0.channels_batch(), two.c0.channels_batch())
            assert np.array_equal(got.c1.channels_batch(), two.c1.channels_batch())
            assert (got.logp, got.logq) == (two.logp, two.logq)
            assert got.logp == 30 - self.mod[-1].bit_length()
        return got


# (n_in, n_out): the issue's three and both sides of the register tiers 4 | 8 | 16
SHAPES = [(1, 1), (3, 2), (16, 16), (4, 1), (5, 1), (8, 2), (9, 2)]


@pytest.mark.parametrize("n_in,n_out", SHAPES)
@pytest.mark.parametrize("Lv", [2, 5])
@pytest.mark.parametrize("bits", [30, 60])
def test_lincomb_matches_the_definition(gpu, bits, Lv, n_in, n_out):
    """B = 3: a bias that landed once per buffer, not once per poly, differs."""
    c = Case(gpu, bits, Lv, n_in, n_out, 3, seed=bits + 7 * Lv + 31 * n_in + n_out)
    for with_bias in (False, True):
        for rescale in (False, True):
            c.check(with_bias, rescale)


@pytest.mark.parametrize("bits", [30, 60])
def test_lincomb_edge_weights_on_all_q_minus_1_inputs(gpu, bits):
    c = Case(gpu, bits, 5, 3, 2, 3, seed=1, edge=True)
    assert {int(v) for v in c.w[:, :, 0].reshape(-1)} == {0, 1, c.mod[0] - 1}
    for with_bias in (False, True):
        for rescale in (False, True):
            c.check(with_bias, rescale)


@pytest.mark.parametrize("bits", [30, 60])
def test_lincomb_on_a_drop_last_view(gpu, bits):
    c = Case(gpu, bits, 3, 3, 2, 3, seed=2, view=2)
    assert c.basis.channel_count() == 3
    for rescale in (False, True):
        c.check(True, rescale)


@pytest.mark.parametrize("B,Lv,n_in,n_out,rescale,want", [
    (1, 5, 3, 2, True, (4, 1)),     # one ciphertext: every output limb a run of its own
    (1, 5, 3, 2, False, (5, 1)),
    (128, 5, 2, 2, False, (3, 2)),  # runs of two limbs, the last one ragged
    (512, 2, 1, 1, False, (1, 2)),  # the vectors alone fill the device: no split
    (512, 2, 1, 1, True, (1, 1)),
])
def test_lincomb_split_and_unsplit_grids(gpu, B, Lv, n_in, n_out, rescale, want):
    assert grid_runs(B, 4, Lv, rescale) == want
    Case(gpu, 30, Lv, n_in, n_out, B, seed=B + Lv).check(True, rescale)


def test_lincomb_u64_split_grid(gpu):
    assert grid_runs(1, 8, 5, True) == (4, 1)
    Case(gpu, 60, 5, 3, 2, 1, seed=5).check(True, True)


def test_lincomb_launch_count(gpu):
    c = Case(gpu, 30, 3, 3, 2, 2, seed=3)
    c.basis.profile_enable(True)
    try:
        c.check(True, False)
        assert c.basis.profile_read("lincomb")[0] == 1
        assert c.basis.profile_read("rescale")[0] == 0
    finally:
        c.basis.profile_enable(False)


# ---- refusals: host-side validation only -------------------------------------

def _raw(rn, rescale, out0, out1, x0, x1, n_in, n_out, w, bias=None):
    f = rn.load().rnt_ct_lincomb_rescale if rescale else rn.load().rnt_ct_lincomb
    u64p = ctypes.POINTER(ctypes.c_uint64)
    wp = None if w is None else np.ascontiguousarray(w, dtype=np.uint64).ctypes.data_as(u64p)
    bp = None if bias is None else np.ascontiguousarray(bias, dtype=np.uint64).ctypes.data_as(u64p)
    status = f(out0.handle, out1.handle, x0.handle, x1.handle, n_in, n_out, wp, bp)
    fields = (ctypes.c_uint64 * 2)()
    detail = rn.load().rnt_last_error_detail(fields) if status else 0
    return status, (int(fields[0]), int(fields[1])), detail


class Refusals:
    def __init__(self, rn):
        self.rn = rn
        self.mod = rn.generate_primes(30, 3, N)
        self.basis = rn.RnsBasis(self.mod, N)
        self.low = self.basis.drop_last(1)
        rng = np.random.default_rng(11)
        self.B, self.n_in, self.n_out = 2, 2, 2
        up = lambda b, k: rn.RnsPoly.from_channels(orc.uniform_poly(b.moduli(), N, rng, batch=k), b)  # noqa: E731
        self.x0, self.x1 = up(self.basis, 4), up(self.basis, 4)
        self.o0, self.o1 = up(self.basis, 4), up(self.basis, 4)    # outputs hold known words
        self.r0, self.r1 = up(self.low, 4), up(self.low, 4)
        self.w = reduce_weights([[1, 2], [3, 4]], self.mod)
        self.before = [p.channels_batch() for p in (self.o0, self.o1, self.r0, self.r1)]

    def untouched(self):
        for p, was in zip((self.o0, self.o1, self.r0, self.r1), self.before):
            assert np.array_equal(p.channels_batch(), was), "a refused call wrote to an output"
            assert not p.is_ntt_domain()


@pytest.fixture(scope="module")
def rf(gpu):
    return Refusals(gpu)


BAD_ARGUMENT, UNSUPPORTED, NON_REDUCED, DOMAIN, BASIS, MOD_DROP = 11, 12, 6, 7, 8, 4


@pytest.mark.parametrize("rescale", [False, True])
def test_refused_counts_and_aliasing(gpu, rf, rescale):
    rn = gpu
    o0, o1 = (rf.r0, rf.r1) if rescale else (rf.o0, rf.o1)
    ok = lambda *a, **k: _raw(rn, rescale, *a, **k)  # noqa: E731
    assert ok(o0, o1, rf.x0, rf.x1, 0, 2, rf.w)[0] == BAD_ARGUMENT
    assert ok(o0, o1, rf.x0, rf.x1, 2, 0, rf.w)[0] == BAD_ARGUMENT
    assert ok(o0, o1, rf.x0, rf.x1, 2, 2, None)[0] == BAD_ARGUMENT
    assert ok(o0, o1, rf.x0, rf.x1, 3, 2, reduce_weights([[1] * 3] * 2, rf.mod))[0] == BAD_ARGUMENT  # 4 polys, 3 terms
    assert ok(o0, o1, rf.x0, rf.x1, 2, 3, reduce_weights([[1] * 2] * 3, rf.mod))[0] == BAD_ARGUMENT  # outputs of 4, not 6
    assert ok(o0, o0, rf.x0, rf.x1, 2, 2, rf.w)[0] == BAD_ARGUMENT  # out0 is out1
    if not rescale:
        assert ok(rf.x0, o1, rf.x0, rf.x1, 2, 2, rf.w)[0] == BAD_ARGUMENT  # an output is an input
        assert ok(o0, rf.x1, rf.x0, rf.x1, 2, 2, rf.w)[0] == BAD_ARGUMENT
    xs = rn.RnsPoly(rf.basis, 2)
    assert ok(o0, o1, rf.x0, xs, 2, 2, rf.w)[0] == BAD_ARGUMENT  # components of different batch sizes
    # 17 terms / outputs: beyond the kernel's tiers, fields 0, 0
    big = rn.RnsPoly(rf.basis, 34)
    st, fields, detail = ok(o0, o1, big, big, 17, 2, reduce_weights([[1] * 17] * 2, rf.mod))
    assert (st, fields, detail) == (UNSUPPORTED, (0, 0), UNSUPPORTED)
    st, fields, _ = ok(o0, o1, rf.x0, rf.x1, 2, 17, reduce_weights([[1] * 2] * 17, rf.mod))
    assert (st, fields) == (UNSUPPORTED, (0, 0))
    rf.untouched()


@pytest.mark.parametrize("rescale", [False, True])
def test_refused_values_domains_and_bases(gpu, rf, rescale):
    rn = gpu
    o0, o1 = (rf.r0, rf.r1) if rescale else (rf.o0, rf.o1)
    ok = lambda *a, **k: _raw(rn, rescale, *a, **k)  # noqa: E731
    w = rf.w.copy()
    w[1, 0, 2] = rf.mod[2]  # == its modulus
    assert ok(o0, o1, rf.x0, rf.x1, 2, 2, w) == (NON_REDUCED, (rf.mod[2], rf.mod[2]), NON_REDUCED)
    bias = reduce_weights([5, 6], rf.mod)
    bias[1, 0] = rf.mod[0] + 3
    assert ok(o0, o1, rf.x0, rf.x1, 2, 2, rf.w, bias) == (NON_REDUCED, (rf.mod[0] + 3, rf.mod[0]), NON_REDUCED)
    xn = rf.x1.clone()
    xn.to_ntt_domain()
    assert ok(o0, o1, rf.x0, xn, 2, 2, rf.w)[0] == DOMAIN
    other = rn.RnsBasis(rf.mod, N)  # the same moduli, another context
    xo = rn.RnsPoly(other, 4)
    assert ok(o0, o1, rf.x0, xo, 2, 2, rf.w)[0] == BASIS
    if rescale:
        assert ok(rf.o0, rf.o1, rf.x0, rf.x1, 2, 2, rf.w)[0] == BASIS  # outputs not on drop_last(1)
        r_other = rn.RnsPoly(rf.basis.drop_last(1), 4)                 # outputs on two drop_last(1) contexts
        assert ok(rf.r0, r_other, rf.x0, rf.x1, 2, 2, rf.w)[0] == BASIS
        one = rf.basis.drop_last(2)
        x_one = rn.RnsPoly(one, 4)
        st, fields, detail = ok(rf.r0, rf.r1, x_one, x_one.clone(), 2, 2, reduce_weights([[1, 2], [3, 4]], rf.mod[:1]))
        assert (st, fields, detail) == (MOD_DROP, (1, 1), MOD_DROP)
    else:
        assert ok(rf.r0, rf.r1, rf.x0, rf.x1, 2, 2, rf.w)[0] == BASIS  # outputs on another context than the inputs'
    rf.untouched()


@pytest.mark.parametrize("rescale", [False, True])
def test_refused_key_level_view_and_recording(gpu, rf, rescale):
    rn = gpu
    o0, o1 = (rf.r0, rf.r1) if rescale else (rf.o0, rf.o1)
    ok = lambda *a, **k: _raw(rn, rescale, *a, **k)  # noqa: E731
    # a key level view in any position
    emod = rn.generate_primes(30, 4, N)
    ext = rn.RnsBasis(emod, N)
    rng = np.random.default_rng(12)
    ka, kb = (orc.uniform_poly(emod, N, rng, batch=2) for _ in range(2))
    key = rn.RnsHybridKey.from_channels(ka, kb, ext, 2, n_special=1)
    view = key.at_level(2).a
    for args in ((view, o1, rf.x0, rf.x1), (o0, view, rf.x0, rf.x1), (o0, o1, view, rf.x1), (o0, o1, rf.x0, view)):
        st, fields, _ = ok(*args, 2, 2, rf.w)
        assert (st, fields) == (UNSUPPORTED, (0, 0))
    # between capture_begin and capture_end the call is refused and records nothing
    a, b = rn.RnsPoly(rf.basis, 4), rn.RnsPoly(rf.basis, 4)
    a += b  # (the recorded op, run once un-recorded first)
    with rf.basis.capture():
        a += b
        st, fields, _ = ok(o0, o1, rf.x0, rf.x1, 2, 2, rf.w)
    assert (st, fields) == (UNSUPPORTED, (0, 0))
    rf.basis.sync()
    rf.untouched()
    # and the same call outside a recording is accepted
    assert ok(o0, o1, rf.x0, rf.x1, 2, 2, rf.w)[0] == 0
    rf.before = [p.channels_batch() for p in (rf.o0, rf.o1, rf.r0, rf.r1)]
