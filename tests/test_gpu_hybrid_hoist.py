"""Hoisted rotations and the baby-step giant-step transform on hybrid keys on
the GPU (rnt_ct_rotate_hybrid_hoisted, rnt_ct_linear_bsgs_hybrid):

    out0 = sigma_k(c0 + ModDown(sum_d D_d sigma_k^-1(key_b[d]))),  D_d = ModUp_d(c1)
    out1 = sigma_k(     ModDown(sum_d D_d sigma_k^-1(key_a[d])))

with one ModUp and one forward transform for every step, and k_moddown_auto
(ModDown, the addend and the automorphism in one kernel) per step and
component.  Exact arithmetic with canonical outputs, so the calls must
reproduce the CPU yardstick (tests/hybrid_hoist_ref.py, itself checked in
tests/test_hybrid_hoist_ref.py) word for word, on every kind of ring the
transforms treat differently.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from hybrid_hoist_ref import bsgs_hybrid_ref, hybrid_hoisting_form_coeff, rotate_hybrid_hoisted_ref
from hybrid_ref import n_digits, restrict_key

pytestmark = pytest.mark.gpu


HOIST_T = 4  # steps per k_hoist_mac launch (kHoistT)
# a zero, a negative step, a duplicate, and five nonzero steps: a full group of
# k_hoist_mac and a partial one
STEPS = [0, 1, -3, 1, 5, 2]
# two zero giants, a gap between the nonzero ones, a negative giant
BABY, GIANT = [0, 1, -3], [4, 0, -8, 0]
SMALL_BSGS = ([0, 1], [0, 2])

# log_n, Lv, K, alpha, B, bits, ws_mb, edge
SHAPES = [
    (8, 3, 2, 2, 3, 31, None, False),   # small four-step grid, partial last digit
    (8, 3, 2, 2, 3, 31, None, True),    # the same with an all-(q-1) ciphertext and all-(m-1) keys
    (8, 3, 1, 1, 2, 31, None, False),   # one-limb digits
    (8, 3, 3, 3, 2, 31, None, False),   # a single digit
    (12, 3, 2, 2, 2, 31, None, False),  # whole-plane ring
    (12, 3, 2, 2, 2, 61, None, False),  # u64 kernels
    (14, 3, 2, 2, 3, 31, "1", False),   # several chunks
    (14, 2, 1, 2, 2, 61, None, False),  # u64 four-step
    (16, 4, 2, 2, 2, 31, None, False),  # matrix-core transforms
    (17, 4, 2, 2, 1, 31, None, False),  # largest ring
]


def _rand(rng, mod, n, batch):
    return orc.uniform_poly(mod, n, rng, batch=batch)


def _keys(rng, emod, n, beta, steps, edge=False):
    out = [None if k == 0 else (_rand(rng, emod, n, beta), _rand(rng, emod, n, beta)) for k in steps]
    if edge:
        mm1 = np.array(emod, dtype=np.uint64)[:, None] - np.uint64(1)
        for kk in out:
            if kk is not None:
                kk[0][:] = np.broadcast_to(mm1, kk[0].shape)
                kk[1][:] = np.broadcast_to(mm1, kk[1].shape)
    return out


def _upload(rn, ext, alpha, steps, keys, hoisted):
    out = []
    for k, kk in zip(steps, keys):
        hk = None if kk is None else rn.RnsHybridKey.from_channels(kk[0], kk[1], ext, alpha, rotation=k)
        if hk is not None and hoisted:
            hk.prepare_hoisted()
        out.append(hk)
    return out


class Case:
    """Random ciphertexts over q_0..q_{Lv-1}, random ORDINARY key channels over
    q_0..q_{Lv-1}, p_0..p_{K-1} for every nonzero step; the keys uploaded,
    turned into their hoisting form and packed.  `place`: "view" puts the
    ciphertexts on the drop_last(K) view of the key's root, "root" on an
    unrelated root basis."""

    def __init__(self, rn, log_n, Lv, K, alpha, B, bits, steps=STEPS, edge=False, place="view", seed=0):
        self.rn, self.n, self.Lv, self.K, self.alpha, self.B = rn, 1 << log_n, Lv, K, alpha, B
        self.steps = list(steps)
        n = self.n
        self.emod = rn.generate_primes(bits, Lv + K, n)
        self.mod = self.emod[:Lv]
        self.beta = n_digits(Lv, alpha)
        rng = np.random.default_rng(6300 + 43 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        if edge:
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.c0[B - 1] = self.c1[B - 1] = np.broadcast_to(qm1, (Lv, n))
        self.keys = _keys(rng, self.emod, n, self.beta, self.steps, edge)
        self.ext = rn.RnsBasis(self.emod, n)
        self.basis = self.ext.drop_last(K) if place == "view" else rn.RnsBasis(self.mod, n)
        self.Bc, self.Be = orc.Basis(self.mod, n), orc.Basis(self.emod, n)
        self.hk = _upload(rn, self.ext, alpha, self.steps, self.keys, True)
        self.kset = rn.RnsHybridKeySet(self.hk, alpha)
        up = lambda x: rn.RnsPoly.from_channels(x, self.basis)  # noqa: E731
        self.ct = rn.Ciphertext(up(self.c0), up(self.c1))

    def run(self, out=None):
        return self.rn.rotate_ciphertext_hybrid_hoisted(self.ct, self.kset, out=out)

    def reference(self, p, t, c0=None, c1=None):
        c0 = self.c0 if c0 is None else c0
        c1 = self.c1 if c1 is None else c1
        return rotate_hybrid_hoisted_ref(self.Bc, self.Be, c0[p], c1[p], self.steps[t],
                                         *(self.keys[t] or (None, None)), self.alpha)


def _check_rotations(c, g0, g1, c0=None, c1=None, polys=None):
    for p in (sorted({0, c.B - 1}) if polys is None else polys):
        done = {}
        for t, k in enumerate(c.steps):
            key = (k, id(c.keys[t]))
            if key not in done:
                done[key] = c.reference(p, t, c0, c1)
            r0, r1 = done[key]
            assert np.array_equal(g0[t * c.B + p], r0), f"out0 of step {t} ({k}), ciphertext {p}"
            assert np.array_equal(g1[t * c.B + p], r1), f"out1 of step {t} ({k}), ciphertext {p}"


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb,edge", SHAPES)
def test_rotate_hybrid_hoisted_parity(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb, edge):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    c = Case(gpu, log_n, Lv, K, alpha, B, bits, edge=edge)
    out = c.run()
    n_steps = len(c.steps)
    assert out.c0.n_polys == n_steps * B and out.c1.n_polys == n_steps * B
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    g0, g1 = out.c0.channels(), out.c1.channels()
    _check_rotations(c, g0, g1)
    z = c.steps.index(0)  # the step-0 slot is the ciphertext itself, every poly of it
    assert np.array_equal(g0[z * B:(z + 1) * B], c.c0) and np.array_equal(g1[z * B:(z + 1) * B], c.c1)


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb,edge", SHAPES)
def test_rotate_hybrid_hoisted_unfused_tail(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb, edge):
    """RNT_MODDOWN_AUTO=0 (read at rnt_ctx_create): k_moddown, the automorphism
    launch and a strided copy in place of k_moddown_auto -- the same words.  It
    is the library's own choice from 16 MiB a component on, so every ring runs it."""
    monkeypatch.setenv("RNT_MODDOWN_AUTO", "0")
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)
    c = Case(gpu, log_n, Lv, K, alpha, B, bits, steps=[0, 1, -3], edge=edge)
    out = c.run()
    _check_rotations(c, out.c0.channels(), out.c1.channels())


def test_more_than_eight_special_primes(gpu):
    """K = 9: the 16-limb tier of k_moddown (the transform's two ModDowns) and
    the recomputing form of k_moddown_auto, which has no 16-limb tier (the z_k
    are recomputed per output limb)."""
    c = Case(gpu, 8, 3, 9, 3, 2, 31, steps=[0, 1, -3], seed=10)
    out = c.run()
    _check_rotations(c, out.c0.channels(), out.c1.channels())
    b = BsgsCase(gpu, 8, 3, 9, 3, 2, 31, seed=10)
    o = b.run()
    r0, r1 = b.reference(1)
    assert np.array_equal(o.c0.channels_of(1)[0], r0) and np.array_equal(o.c1.channels_of(1)[0], r1)


def test_default_tail_by_chunk_size(gpu):
    """Without RNT_MODDOWN_AUTO the tail is k_moddown_auto while one component
    of the chunk is below 16 MiB and the three un-fused launches from there on
    (DESIGN.md section 4): 2^16 x 4 limbs is 1 MiB a ciphertext, so 15
    ciphertexts take the one and 16 the other, both with the reference's words."""
    for B, fused in ((15, True), (16, False)):
        c = Case(gpu, 16, 4, 2, 2, B, 31, steps=[1], seed=9)
        counts = _counts(c.basis, c.run)
        assert counts["moddown_auto"] == (2 if fused else 0) and counts["moddown"] == (0 if fused else 2), (B, counts)
        out = c.run()
        r0, r1 = c.reference(B - 1, 0)
        assert np.array_equal(out.c0.channels_of(B - 1)[0], r0) and np.array_equal(out.c1.channels_of(B - 1)[0], r1), B


class BsgsCase:
    def __init__(self, rn, log_n, Lv, K, alpha, B, bits, baby=BABY, giant=GIANT, edge=False, seed=0):
        self.rn, self.n, self.Lv, self.K, self.alpha, self.B = rn, 1 << log_n, Lv, K, alpha, B
        self.baby, self.giant = list(baby), list(giant)
        n, nt = self.n, len(baby) * len(giant)
        self.emod = rn.generate_primes(bits, Lv + K, n)
        self.mod = self.emod[:Lv]
        self.beta = n_digits(Lv, alpha)
        rng = np.random.default_rng(7300 + 47 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.diag = _rand(rng, self.mod, n, nt)  # coefficient domain, poly j n1 + i
        if edge:
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.c0[B - 1] = self.c1[B - 1] = np.broadcast_to(qm1, (Lv, n))
        self.bkeys = _keys(rng, self.emod, n, self.beta, self.baby, edge)
        self.gkeys = _keys(rng, self.emod, n, self.beta, self.giant, edge)
        self.ext = rn.RnsBasis(self.emod, n)
        self.basis = self.ext.drop_last(K)
        self.Bc, self.Be = orc.Basis(self.mod, n), orc.Basis(self.emod, n)
        self.bset = rn.RnsHybridKeySet(_upload(rn, self.ext, alpha, self.baby, self.bkeys, True), alpha)
        self.gset = rn.RnsHybridKeySet(_upload(rn, self.ext, alpha, self.giant, self.gkeys, False), alpha)
        self.d = rn.RnsPoly.from_channels(self.diag, self.basis)
        self.d.to_ntt_domain()
        up = lambda x: rn.RnsPoly.from_channels(x, self.basis)  # noqa: E731
        self.ct = rn.Ciphertext(up(self.c0), up(self.c1))

    def run(self, out=None):
        return self.rn.linear_transform_bsgs_hybrid(self.ct, self.d, self.bset, self.gset, out=out)

    def reference(self, p, c0=None, c1=None):
        c0 = self.c0 if c0 is None else c0
        c1 = self.c1 if c1 is None else c1
        return bsgs_hybrid_ref(self.Bc, self.Be, c0[p], c1[p], self.baby, self.giant, self.diag, self.bkeys,
                               self.gkeys, self.alpha)


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb,edge", SHAPES)
def test_bsgs_hybrid_parity(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb, edge):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)
    big = log_n >= 16  # (the CPU reference within seconds)
    baby, giant = SMALL_BSGS if big else (BABY, GIANT)
    c = BsgsCase(gpu, log_n, Lv, K, alpha, B, bits, baby=baby, giant=giant, edge=edge)
    out = c.run()
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    g0, g1 = out.c0.channels(), out.c1.channels()
    for p in ([0] if big else sorted({0, B - 1})):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0), f"out0 of ciphertext {p} differs from bsgs_hybrid_ref"
        assert np.array_equal(g1[p], r1), f"out1 of ciphertext {p} differs from bsgs_hybrid_ref"


@pytest.mark.parametrize("log_n", [8, 12])
def test_bsgs_hybrid_in_place_and_unfused_tail(gpu, monkeypatch, log_n):
    c = BsgsCase(gpu, log_n, 3, 2, 2, 2, 31, seed=1)
    out = c.run()
    w0, w1 = out.c0.channels(), out.c1.channels()
    monkeypatch.setenv("RNT_MODDOWN_AUTO", "0")
    u = BsgsCase(gpu, log_n, 3, 2, 2, 2, 31, seed=1)  # a context of its own: the switch is read at creation
    o = u.run()
    assert np.array_equal(o.c0.channels(), w0) and np.array_equal(o.c1.channels(), w1)
    same = c.run(out=c.ct)
    assert same is c.ct
    assert np.array_equal(c.ct.c0.channels(), w0) and np.array_equal(c.ct.c1.channels(), w1)


@pytest.mark.parametrize("log_n", [8, 12])
def test_linear_transform_hybrid_is_the_bsgs_call_with_one_zero_giant(gpu, log_n):
    c = BsgsCase(gpu, log_n, 3, 2, 2, 2, 31, baby=[0, 1, -3], giant=[0], seed=2)
    rn = c.rn
    a = c.run()
    b = rn.linear_transform_hybrid(c.ct, c.d, c.bset)
    assert np.array_equal(a.c0.channels(), b.c0.channels()) and np.array_equal(a.c1.channels(), b.c1.channels())
    r0, r1 = c.reference(1)
    assert np.array_equal(b.c0.channels_of(1)[0], r0) and np.array_equal(b.c1.channels_of(1)[0], r1)
    # all steps 0 on both stages: no key at all
    z = rn.RnsHybridKeySet([None], c.alpha)
    d1 = rn.RnsPoly.from_channels(c.diag[:1], c.basis)
    d1.to_ntt_domain()
    o = rn.linear_transform_bsgs_hybrid(c.ct, d1, z, z)
    assert np.array_equal(o.c0.channels_of(0)[0], orc.mul(c.Bc, c.c0[0], c.diag[0]))
    assert np.array_equal(o.c1.channels_of(0)[0], orc.mul(c.Bc, c.c1[0], c.diag[0]))


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits", [(8, 3, 2, 2, 3, 31), (12, 3, 2, 2, 2, 31)])
def test_single_step_calls_equal_the_multi_step_call(gpu, log_n, Lv, K, alpha, B, bits):
    c = Case(gpu, log_n, Lv, K, alpha, B, bits, seed=1)
    rn = c.rn
    out = c.run()
    g0, g1 = out.c0.channels(), out.c1.channels()
    for t, k in enumerate(c.steps):
        one = rn.rotate_ciphertext_hybrid_hoisted(c.ct, rn.RnsHybridKeySet([c.hk[t]], alpha))
        assert one.c0.n_polys == B
        assert np.array_equal(one.c0.channels(), g0[t * B:(t + 1) * B]), (t, k)
        assert np.array_equal(one.c1.channels(), g1[t * B:(t + 1) * B]), (t, k)


@pytest.mark.parametrize("log_n,Lv,K,alpha,bits", [(8, 3, 2, 2, 31), (12, 3, 2, 2, 61), (16, 2, 1, 2, 31)])
def test_key_prepare_hoisted_on_the_key_basis(gpu, log_n, Lv, K, alpha, bits):
    """rnt_key_prepare_hoisted on a beta-poly buffer over E gives
    NTT(sigma_k^-1(key)) as the oracle computes it, from both entry domains."""
    rn, lib = gpu, gpu.load()
    n = 1 << log_n
    emod = rn.generate_primes(bits, Lv + K, n)
    ext, Be = rn.RnsBasis(emod, n), orc.Basis(emod, n)
    beta = n_digits(Lv, alpha)
    rng = np.random.default_rng(61 + log_n)
    ka, kb = _rand(rng, emod, n, beta), _rand(rng, emod, n, beta)
    for k in (1, -3):
        want = [np.stack([orc.to_ntt(Be, p) for p in hybrid_hoisting_form_coeff(Be, x, k)]) for x in (ka, kb)]
        for from_ntt in (False, True):
            a, b = rn.RnsPoly.from_channels(ka, ext), rn.RnsPoly.from_channels(kb, ext)
            if from_ntt:
                a.to_ntt_domain()
                b.to_ntt_domain()
            rn.check(lib.rnt_key_prepare_hoisted(a.handle, b.handle, k))
            assert a.is_ntt_domain() and b.is_ntt_domain()
            assert np.array_equal(a.channels(), want[0]) and np.array_equal(b.channels(), want[1]), (k, from_ntt)
        hk = rn.RnsHybridKey.from_channels(ka, kb, ext, alpha, rotation=k).prepare_hoisted()
        assert hk.hoisted and np.array_equal(hk.a.channels(), want[0]) and np.array_equal(hk.b.channels(), want[1])


@pytest.mark.parametrize("log_n", [8, 12, 14])
def test_levelled(gpu, log_n):
    """A 4-limb chain with alpha = 2: one level down the keys are the full
    hoisting-form keys restricted to a fresh root over q_0..q_2, p_0, p_1 and
    the ciphertext sits on drop_last(1) of an unrelated 4-limb root."""
    rn = gpu
    steps = [0, 1, -3]
    top = Case(rn, log_n, 4, 2, 2, 2, 31, steps=steps, seed=2)
    out = top.run()
    _check_rotations(top, out.c0.channels(), out.c1.channels())
    n, q, p = top.n, top.mod, top.emod[4:]
    low = Case.__new__(Case)
    low.rn, low.n, low.Lv, low.K, low.alpha, low.B, low.steps = rn, n, 3, 2, 2, 2, steps
    low.mod, low.emod = q[:3], q[:3] + p
    low.c0 = np.ascontiguousarray(top.c0[:, :3, :])
    low.c1 = np.ascontiguousarray(top.c1[:, :3, :])
    low.ext = rn.RnsBasis(low.emod, n)
    low.hk = [None if k is None else k.restrict(low.ext) for k in top.hk]
    assert low.hk[1].hoisted and low.hk[1].a.n_polys == 2 and low.hk[1].a.basis is low.ext
    low.kset = rn.RnsHybridKeySet(low.hk, 2)
    assert low.kset.hoisted
    low.keys = [None if kk is None else (restrict_key(kk[0], 4, 2, 3), restrict_key(kk[1], 4, 2, 3)) for kk in top.keys]
    low.Bc, low.Be = orc.Basis(low.mod, n), orc.Basis(low.emod, n)
    low.basis = rn.RnsBasis(q, n).drop_last(1)
    up = lambda x: rn.RnsPoly.from_channels(x, low.basis)  # noqa: E731
    low.ct = rn.Ciphertext(up(low.c0), up(low.c1))
    out = low.run()
    _check_rotations(low, out.c0.channels(), out.c1.channels())
    # the transform at that level: baby keys the restricted hoisting-form ones,
    # giant keys restricted ordinary ones
    rng = np.random.default_rng(90 + log_n)
    gk = _keys(rng, top.emod, n, 2, [2, 0])
    gtop = _upload(rn, top.ext, 2, [2, 0], gk, False)
    gset = rn.RnsHybridKeySet([None if k is None else k.restrict(low.ext) for k in gtop], 2)
    diag = _rand(rng, low.mod, n, 6)
    d = rn.RnsPoly.from_channels(diag, low.basis)
    d.to_ntt_domain()
    o = rn.linear_transform_bsgs_hybrid(low.ct, d, low.kset, gset)
    glow = [None if kk is None else (restrict_key(kk[0], 4, 2, 3), restrict_key(kk[1], 4, 2, 3)) for kk in gk]
    r0, r1 = bsgs_hybrid_ref(low.Bc, low.Be, low.c0[1], low.c1[1], steps, [2, 0], diag, low.keys, glow, 2)
    assert np.array_equal(o.c0.channels_of(1)[0], r0) and np.array_equal(o.c1.channels_of(1)[0], r1)


def test_unaligned_planes(gpu):
    """The scalar instantiations: the inputs, the key sets and the outputs
    wrapped at an offset of one word, so none of their planes is 16-byte
    aligned."""
    import torch

    c = Case(gpu, 8, 3, 2, 2, 3, 31, seed=3)
    rn, lib, Bd = c.rn, c.rn.load(), c.basis
    dev = torch.device("cuda", Bd.device)

    def shifted(basis, n_polys, src=None, ntt=False):
        words = n_polys * basis.channel_count() * c.n
        t = torch.zeros(words + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(basis, t.data_ptr() + 4, n_polys, in_ntt_domain=ntt, owner=t)
        assert v.device_ptr()[0] % 16 == 4
        if src is not None:
            v.copy_polys(src)
        return v

    want = c.run()
    ns = len(c.steps)
    g0, g1 = shifted(Bd, ns * c.B), shifted(Bd, ns * c.B)
    s0, s1 = shifted(Bd, c.B, c.ct.c0), shifted(Bd, c.B, c.ct.c1)
    ka = shifted(c.ext, c.kset.a.n_polys, c.kset.a, ntt=True)
    kb = shifted(c.ext, c.kset.b.n_polys, c.kset.b, ntt=True)
    steps = (ctypes.c_int32 * ns)(*c.steps)
    rn.check(lib.rnt_ct_rotate_hybrid_hoisted(g0.handle, g1.handle, s0.handle, s1.handle, steps, ns, ka.handle,
                                              kb.handle, c.alpha))
    assert np.array_equal(g0.channels(), want.c0.channels()) and np.array_equal(g1.channels(), want.c1.channels())
    b = BsgsCase(gpu, 8, 3, 2, 2, 3, 31, seed=3)
    wantb = b.run()
    o0, o1 = shifted(b.basis, b.B), shifted(b.basis, b.B)
    t0, t1 = shifted(b.basis, b.B, b.ct.c0), shifted(b.basis, b.B, b.ct.c1)
    d = shifted(b.basis, b.d.n_polys, b.d, ntt=True)
    sets = [shifted(b.ext, x.n_polys, x, ntt=True) for x in (b.bset.a, b.bset.b, b.gset.a, b.gset.b)]
    baby, giant = (ctypes.c_int32 * len(b.baby))(*b.baby), (ctypes.c_int32 * len(b.giant))(*b.giant)
    rn.check(lib.rnt_ct_linear_bsgs_hybrid(o0.handle, o1.handle, t0.handle, t1.handle, baby, len(b.baby), giant,
                                           len(b.giant), d.handle, *[x.handle for x in sets], b.alpha))
    assert np.array_equal(o0.channels(), wantb.c0.channels()) and np.array_equal(o1.channels(), wantb.c1.channels())


def test_large_batch_grids(gpu, monkeypatch):
    """64 ciphertexts at 2^14 (1024 workgroups of vectors): the un-split grids
    of k_modup, k_moddown and k_moddown_auto."""
    monkeypatch.setenv("RNT_MODDOWN_AUTO", "2")  # k_moddown_auto at every size
    c = Case(gpu, 14, 3, 2, 2, 64, 31, steps=[1, -3], seed=8)
    out = c.run()
    _check_rotations(c, out.c0.channels(), out.c1.channels())
    b = BsgsCase(gpu, 14, 3, 2, 2, 64, 31, baby=[1, -3], giant=[2, 0], seed=8)
    o = b.run()
    r0, r1 = b.reference(63)
    assert np.array_equal(o.c0.channels_of(63)[0], r0) and np.array_equal(o.c1.channels_of(63)[0], r1)


NAMES = ("modup", "moddown", "moddown_auto", "hoist_mac", "automorphism", "copy", "ks_decompose", "ks_rows",
         "ks_whole", "hoist_digits")


def _counts(basis, run):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in NAMES}
    basis.profile_enable(False)
    print(counts)
    return counts


def test_launch_counts(gpu):
    """One chunk, five nonzero steps: one ModUp, ceil(5 / 4) multiply-accumulate
    launches, a k_moddown_auto per step and component, no stand-alone
    automorphism, no copy (the call has no step of 0) and none of the gadget
    key-switch's kernels."""
    c = Case(gpu, 14, 3, 2, 2, 2, 31, steps=[1, -3, 1, 5, 2], seed=4)
    counts = _counts(c.basis, c.run)
    assert counts["modup"] == 1
    assert counts["hoist_mac"] == -(-5 // HOIST_T) == 2
    assert counts["moddown_auto"] == 10
    assert counts["moddown"] == 0 and counts["automorphism"] == 0 and counts["copy"] == 0
    for k in ("ks_decompose", "ks_rows", "ks_whole", "hoist_digits"):
        assert counts[k] == 0, k


def test_launch_counts_bsgs(gpu):
    """One chunk: one ModUp for the baby stage and one per nonzero giant, and
    exactly two ModDowns however many giants there are."""
    c = BsgsCase(gpu, 14, 3, 2, 2, 2, 31, seed=4)
    counts = _counts(c.basis, c.run)
    nzg = sum(g != 0 for g in c.giant)
    assert nzg == 2
    assert counts["modup"] == 1 + nzg
    assert counts["moddown"] == 2
    assert counts["moddown_auto"] == 2 * sum(b != 0 for b in c.baby)
    assert counts["hoist_mac"] == 1 + nzg
    for k in ("ks_decompose", "ks_rows", "ks_whole", "hoist_digits"):
        assert counts[k] == 0, k


@pytest.mark.parametrize("log_n", [12, 14])
def test_captured(gpu, log_n):
    """Both calls record into a graph after one plain run; two replays on
    refreshed inputs give the words of the plain calls."""
    c = Case(gpu, log_n, 3, 2, 2, 2, 31, steps=[0, 1, -3], seed=5)
    b = BsgsCase(gpu, log_n, 3, 2, 2, 2, 31, seed=5)
    rn = c.rn
    nb = len(c.steps) * c.B
    rout = rn.Ciphertext(rn.RnsPoly(c.basis, nb), rn.RnsPoly(c.basis, nb))
    bout = rn.Ciphertext(rn.RnsPoly(b.basis, b.B), rn.RnsPoly(b.basis, b.B))
    c.run(out=rout)
    b.run(out=bout)
    with c.basis.capture() as g:
        c.run(out=rout)
    with b.basis.capture() as gb:
        b.run(out=bout)
    rng = np.random.default_rng(57 + log_n)
    for _ in range(2):
        n0, n1 = _rand(rng, c.mod, c.n, c.B), _rand(rng, c.mod, c.n, c.B)
        for case in (c, b):
            case.ct.c0.copy_polys(rn.RnsPoly.from_channels(n0, case.basis))
            case.ct.c1.copy_polys(rn.RnsPoly.from_channels(n1, case.basis))
        g.replay()
        c.basis.sync()
        gb.replay()
        b.basis.sync()
        got = [x.channels() for x in (rout.c0, rout.c1, bout.c0, bout.c1)]
        plain, plainb = c.run(), b.run()
        want = [x.channels() for x in (plain.c0, plain.c1, plainb.c0, plainb.c1)]
        for i in range(4):
            assert np.array_equal(got[i], want[i]), i
        _check_rotations(c, got[0], got[1], n0, n1, polys=[0])
        r0, r1 = b.reference(0, n0, n1)
        assert np.array_equal(got[2][0], r0) and np.array_equal(got[3][0], r1)


def test_errors(gpu):
    """Every row of the error table, with its status and fields; a refused
    call leaves the outputs untouched."""
    c = Case(gpu, 8, 3, 2, 2, 2, 31, steps=[0, 1, -3], seed=6)
    b = BsgsCase(gpu, 8, 3, 2, 2, 2, 31, baby=[0, 1, -3], giant=[4, 0, -8], seed=6)
    rn, lib, Bd, Lv, B, n, beta = c.rn, c.rn.load(), c.basis, c.Lv, c.B, c.n, c.beta
    rng = np.random.default_rng(58)
    mark0, mark1 = _rand(rng, c.mod, n, 3 * B), _rand(rng, c.mod, n, 3 * B)
    o0, o1 = rn.RnsPoly.from_channels(mark0, Bd), rn.RnsPoly.from_channels(mark1, Bd)
    bm0, bm1 = _rand(rng, c.mod, n, B), _rand(rng, c.mod, n, B)
    p0, p1 = rn.RnsPoly.from_channels(bm0, b.basis), rn.RnsPoly.from_channels(bm1, b.basis)
    steps = (ctypes.c_int32 * 3)(0, 1, -3)
    baby, giant = (ctypes.c_int32 * 3)(*b.baby), (ctypes.c_int32 * 3)(*b.giant)
    h = lambda x: None if x is None else x.handle  # noqa: E731

    def rot(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, st=steps, ns=3, ka=c.kset.a, kb=c.kset.b, alpha=c.alpha):
        return lib.rnt_ct_rotate_hybrid_hoisted(h(out0), h(out1), h(c0), h(c1), st, ns, h(ka), h(kb), alpha)

    def lin(out0=p0, out1=p1, c0=b.ct.c0, c1=b.ct.c1, bs=baby, nb=3, gs=giant, ng=3, d=b.d, ka=b.bset.a, kb=b.bset.b,
            ga=b.gset.a, gb=b.gset.b, alpha=b.alpha):
        return lib.rnt_ct_linear_bsgs_hybrid(h(out0), h(out1), h(c0), h(c1), bs, nb, gs, ng, h(d), h(ka), h(kb),
                                             h(ga), h(gb), alpha)

    def fails(kind, fn, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(fn(**kw))
        assert e.value.kind == kind, (kind, fn.__name__, kw.keys(), str(e.value))
        if fields is not None:
            assert e.value.fields == fields, e.value.fields
        assert np.array_equal(o0.channels(), mark0) and np.array_equal(o1.channels(), mark1), kw.keys()
        assert np.array_equal(p0.channels(), bm0) and np.array_equal(p1.channels(), bm1), kw.keys()

    def keypoly(count, basis=c.ext, ntt=True):
        L = basis.channel_count()
        nn = basis.degree
        return rn.RnsPoly.from_channels(np.zeros((count, L, nn), np.uint64), basis, in_ntt_domain=ntt)

    for fn in (rot, lin):
        fails("BadArgument", fn, alpha=0)
        fails("BadArgument", fn, out1=(o0 if fn is rot else p0))  # out0 aliases out1
    fails("BadArgument", rot, ns=0)
    fails("BadArgument", rot, st=None)
    fails("BadArgument", lin, nb=0)
    fails("BadArgument", lin, gs=None)
    fails("BadArgument", rot, out0=rn.RnsPoly(Bd, B))  # outputs of the wrong size
    fails("BadArgument", rot, out1=rn.RnsPoly(Bd, 3 * B + 1))
    fails("BadArgument", lin, out0=rn.RnsPoly(b.basis, B + 1))
    fails("BadArgument", lin, d=keypoly(8, b.basis))  # 8 plaintexts for 3 x 3
    one = (ctypes.c_int32 * 1)(1)
    k1 = rn.RnsHybridKeySet([c.hk[1]], c.alpha)
    fails("BadArgument", rot, out0=c.ct.c0, out1=rn.RnsPoly(Bd, B), st=one, ns=1, ka=k1.a, kb=k1.b)  # aliases an input
    fails("BadArgument", rot, out0=rn.RnsPoly(Bd, B), out1=c.ct.c1, st=one, ns=1, ka=k1.a, kb=k1.b)
    fails("BadArgument", lin, out0=b.ct.c1, out1=rn.RnsPoly(b.basis, B))  # an input other than its own component
    fails("BadArgument", rot, ka=None)
    fails("BadArgument", lin, gb=None)
    # degree, device or moduli-prefix mismatch; E without a special limb
    half = rn.RnsBasis(rn.generate_primes(31, Lv + c.K, n // 2), n // 2)
    other = rn.RnsBasis(c.emod[1:] + c.emod[:1], n)  # the same primes in another order
    for basis in (half, other, Bd, c.ext.drop_last(c.K + 1)):
        fails("BasisMismatch", rot, ka=keypoly(3 * beta, basis), kb=keypoly(3 * beta, basis))
    fails("BasisMismatch", lin, ka=keypoly(3 * beta, other), kb=keypoly(3 * beta, other))
    fails("BasisMismatch", lin, ga=keypoly(3 * beta, b.basis), gb=keypoly(3 * beta, b.basis))
    twin = rn.RnsBasis(c.emod, n)  # the same moduli, another key basis: one E for both stages
    fails("BasisMismatch", lin, ga=keypoly(3 * beta, twin), gb=keypoly(3 * beta, twin))
    fails("BasisMismatch", rot, c1=rn.RnsPoly.from_channels(c.c1, rn.RnsBasis(c.mod, n)))
    fails("BasisMismatch", lin, d=keypoly(9, rn.RnsBasis(c.mod, n)))
    # different device word widths: a 61-bit special prime makes E a u64 basis
    wide = rn.RnsBasis(c.mod + rn.generate_primes(61, 1, n), n)
    fails("Unsupported", rot, {"degree": 0, "max_degree": 0}, ka=keypoly(3 * beta, wide), kb=keypoly(3 * beta, wide))
    fails("Unsupported", lin, {"degree": 0, "max_degree": 0}, ka=keypoly(3 * beta, wide), kb=keypoly(3 * beta, wide))
    # the key-count rule: n beta polys
    fails("ChannelCountMismatch", rot, {"expected": 3 * beta, "actual": 2 * beta}, ka=keypoly(2 * beta))
    fails("ChannelCountMismatch", rot, {"expected": 3 * beta, "actual": beta}, kb=keypoly(beta))
    fails("ChannelCountMismatch", rot, {"expected": 3 * Lv, "actual": 3 * beta}, alpha=1)
    fails("ChannelCountMismatch", lin, {"expected": 3 * beta, "actual": 3 * beta + 1}, kb=keypoly(3 * beta + 1, b.ext))
    fails("ChannelCountMismatch", lin, {"expected": 3 * beta, "actual": beta}, ga=keypoly(beta, b.ext))
    for fn, ext in ((rot, c.ext), (lin, b.ext)):
        fails("DomainMismatch", fn, ka=keypoly(3 * beta, ext, ntt=False))
        fails("DomainMismatch", fn, kb=keypoly(3 * beta, ext, ntt=False))
    fails("DomainMismatch", lin, gb=keypoly(3 * beta, b.ext, ntt=False))
    fails("DomainMismatch", lin, d=keypoly(9, b.basis, ntt=False))
    ntt = c.ct.c1.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", rot, c0=ntt)
    fails("DomainMismatch", rot, c1=ntt)
    nb_ = b.ct.c1.clone()
    nb_.to_ntt_domain()
    fails("DomainMismatch", lin, c0=nb_)
    # the valid calls still run after all that, and calls without any key
    v0, v1 = rn.RnsPoly(Bd, 3 * B), rn.RnsPoly(Bd, 3 * B)
    rn.check(rot(out0=v0, out1=v1))
    _check_rotations(c, v0.channels(), v1.channels())
    z = (ctypes.c_int32 * 3)(0, 0, 0)
    rn.check(rot(out0=v0, out1=v1, st=z, ka=None, kb=None))
    assert np.array_equal(v0.channels(), np.concatenate([c.c0] * 3))
    assert np.array_equal(v1.channels(), np.concatenate([c.c1] * 3))
    w0, w1 = rn.RnsPoly(b.basis, B), rn.RnsPoly(b.basis, B)
    rn.check(lin(out0=w0, out1=w1))
    r0, r1 = b.reference(0)
    assert np.array_equal(w0.channels_of(0)[0], r0) and np.array_equal(w1.channels_of(0)[0], r1)


def test_python_layer_guards_the_key_class_and_form(gpu):
    """The library cannot tell the two key forms apart, nor a gadget key set
    from a hybrid one; the wrappers do."""
    c = Case(gpu, 8, 3, 2, 2, 2, 31, steps=[0, 1, -3], seed=7)
    rn = c.rn
    plain = _upload(rn, c.ext, c.alpha, c.steps, c.keys, False)
    pset = rn.RnsHybridKeySet(plain, c.alpha)
    assert c.kset.hoisted and not pset.hoisted and c.hk[1].hoisted and not plain[1].hoisted
    rng = np.random.default_rng(59)
    d = rn.RnsPoly.from_channels(_rand(rng, c.mod, c.n, 3), c.basis)
    d.to_ntt_domain()
    gk = rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.Lv), _rand(rng, c.mod, c.n, c.Lv), c.basis, rotation=1)
    gset = rn.RnsGadgetKeySet([None, gk, None], c.basis)
    zero = rn.RnsHybridKeySet([None], c.alpha)
    for call in (lambda: rn.rotate_ciphertext_hybrid_hoisted(c.ct, pset),       # ordinary keys
                 lambda: rn.rotate_ciphertext_hybrid_hoisted(c.ct, gset),       # a gadget key set
                 lambda: rn.linear_transform_hybrid(c.ct, d, pset),
                 lambda: rn.linear_transform_hybrid(c.ct, d, gset),
                 lambda: rn.linear_transform_bsgs_hybrid(c.ct, d, pset, zero),
                 lambda: rn.linear_transform_bsgs_hybrid(c.ct, d, zero, c.kset),  # hoisting-form giants
                 lambda: rn.linear_transform_bsgs_hybrid(c.ct, d, c.kset, gset),
                 lambda: rn.rotate_ciphertext_hybrid(c.ct, c.hk[1]),            # a hoisting-form key
                 lambda: rn.keyswitch_hybrid(c.ct.c1, c.hk[1]),
                 lambda: rn.RnsHybridKeySet([c.hk[1], plain[2]], c.alpha),      # a mix of forms
                 lambda: rn.RnsHybridKeySet([gk], c.alpha),
                 lambda: rn.RnsHybridKeySet([None]),                            # no alpha
                 lambda: rn.RnsHybridKeySet([c.hk[1]], c.alpha + 1),
                 lambda: c.hk[1].prepare_hoisted()):                            # already in hoisting form
        with pytest.raises(ValueError):
            call()
    relin = rn.RnsHybridKey.from_channels(c.keys[1][0], c.keys[1][1], c.ext, c.alpha)
    with pytest.raises(ValueError):
        relin.prepare_hoisted()  # no rotation
    # a set without any key serves both forms
    out = rn.rotate_ciphertext_hybrid_hoisted(c.ct, rn.RnsHybridKeySet([None, None], c.alpha))
    assert np.array_equal(out.c0.channels(), np.concatenate([c.c0] * 2))


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _rolled(x, k):
    r = np.roll(x, -abs(int(k)))
    return np.conj(r) if k < 0 else r


# tools/hybrid_hoist_tolerance.py, eight seeds, the same ring and parameters on
# the CPU (oracle/pyoracle, oracle/encoder.py, tests/hybrid_hoist_ref.py): the
# largest decode errors.  The tolerances are 4 x these, the project's margin for
# another noise draw (the device's sampler), the arithmetic being identical.
ROT_ERR_MEASURED = 5.850e-5
BSGS_ERR_MEASURED = 9.210e-5
LIN_ERR_MEASURED = 9.028e-5


def _engine(rn):
    from rns_ntt.engine import CkksEngine

    n, L, K = 1024, 4, 2
    q, c = [], (1 << 30) + 1  # tools/hybrid_tolerance.py's ring
    while len(q) < L:
        if rn.is_ntt_friendly_prime(c, n):
            q.append(c)
        c += 2 * n
    eng = CkksEngine(q, n, error_std=3.2, hamming_weight=n // 2, special_moduli=rn.generate_primes(31, K, n))
    return CkksEngine, eng, q


def test_engine_rotate_hoisted_hybrid_end_to_end(gpu):
    """N = 2^10, 4 x 31-bit + 2 special primes, alpha = 2, a DeviceRng, scale
    2^30: encode -> encrypt -> rotate_hoisted_hybrid by [1, -3, 7] -> decrypt ->
    decode against the rolled slots."""
    rn = gpu
    CkksEngine, eng, q = _engine(rn)
    n, slots, L, alpha, logp = 1024, 512, 4, 2, 30
    rng = rn.DeviceRng(91)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    steps = [1, -3, 7]
    kset = eng.generate_hybrid_rotation_key_set(sk, steps, rng, alpha, hoisted=True)
    assert kset.hoisted and kset.a.n_polys == len(steps) * 2 and kset.steps == steps
    x = np.random.default_rng(92).uniform(-1, 1, slots)
    enc = rn.CkksEncoder(n, logp)
    ct = eng.encrypt(enc.encode(x, eng.basis), pk, rng)
    out = CkksEngine.rotate_hoisted_hybrid(ct, kset)
    assert out.c0.n_polys == len(steps) and out.logp == logp and out.logq == ct.logq
    dec = out.c1 * rn.RnsPoly.from_channels(np.broadcast_to(sk.channels(), (len(steps), L, n)).copy(), eng.basis)
    got = enc.decode(rn.Plaintext(dec + out.c0, logp, slots))
    worst = 0.0
    for t, k in enumerate(steps):
        err = float(np.max(np.abs(got[t] - _rolled(x, k))))
        print(f"hoisted hybrid rotation by {k}: decode error {err:.3e}")
        worst = max(worst, err)
    assert worst <= 4 * ROT_ERR_MEASURED


def test_engine_linear_transforms_hybrid_end_to_end(gpu):
    """A 16-diagonal band at diagonal scale 2^30 through
    linear_transform_bsgs_hybrid (4 x 4) and through linear_transform_hybrid
    (the sixteen steps hoisted) -> rescale -> decrypt -> decode against M x."""
    rn = gpu
    CkksEngine, eng, q = _engine(rn)
    n, slots, alpha, logp = 1024, 512, 2, 30
    rng = rn.DeviceRng(93)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    host = np.random.default_rng(94)
    x = host.uniform(-1, 1, slots)
    M = np.zeros((slots, slots))
    s = np.arange(slots)
    for d in range(16):
        M[s, (s + d) % slots] = host.uniform(-1, 1, slots)
    enc = rn.CkksEncoder(n, logp)
    ct = eng.encrypt(enc.encode(x, eng.basis), pk, rng)
    baby, giant = [0, 1, 2, 3], [0, 4, 8, 12]
    bset = eng.generate_hybrid_rotation_key_set(sk, baby, rng, alpha, hoisted=True)
    gset = eng.generate_hybrid_rotation_key_set(sk, giant, rng, alpha)
    lset = eng.generate_hybrid_rotation_key_set(sk, list(range(16)), rng, alpha, hoisted=True)
    assert bset.hoisted and not gset.hoisted
    outs = {
        "bsgs": CkksEngine.linear_transform_bsgs_hybrid(ct, eng.encode_diagonals_bsgs(M, baby, giant, enc), bset, gset),
        "diagonal": CkksEngine.linear_transform_hybrid(ct, eng.encode_diagonals(M, list(range(16)), enc), lset),
    }
    errs = {}
    for name, out in outs.items():
        assert out.logp == 2 * logp and out.logq == ct.logq
        res = CkksEngine.rescale_ciphertext(out)
        got = enc.decode(CkksEngine.decrypt_plaintext(res, CkksEngine.secret_on(sk, res.c0.basis)))
        # logp counts the dropped prime as 31 bits; the true scale is 2^60 / q_last
        y = (M @ x) * (2.0 ** (2 * logp - res.logp) / q[-1])
        errs[name] = float(np.max(np.abs(got - y)))
        print(f"hybrid linear transform ({name}): decode error {errs[name]:.3e}, max|y| {np.max(np.abs(y)):.3f}")
    assert errs["bsgs"] <= 4 * BSGS_ERR_MEASURED
    assert errs["diagonal"] <= 4 * LIN_ERR_MEASURED
