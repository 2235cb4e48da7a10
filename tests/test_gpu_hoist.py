"""Hoisted rotations on the GPU (rnt_key_prepare_hoisted, rnt_ct_rotate_hoisted,
rnt_ct_linear_bsgs_hoisted):

    out0 = sigma_k(c0) + sum_i sigma_k(D_i) key_b[i],  out1 = sum_i sigma_k(D_i) key_a[i],
    D_i = alpha_i(c1),

computed as sigma_k(c0 + sum_i D_i sigma_k^-1(key_b[i])) with one decomposition
for every step.  Exact arithmetic mod q_j with canonical outputs, so the calls
must reproduce the CPU yardstick (tests/hoist_ref.py, itself checked in
tests/test_hoist_ref.py) word for word, on every kind of ring the transforms
treat differently.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from hoist_ref import bsgs_hoisted_ref, hoisting_form_coeff, rotate_hoisted_ref

pytestmark = pytest.mark.gpu

T = orc.host_threads()
HOIST_T = 4  # steps per k_hoist_mac launch (kHoistT)
# a zero, a negative step, a duplicate, and five nonzero steps: a full group of
# k_hoist_mac and a partial one
STEPS = [0, 1, -3, 1, 5, 2]
SMALL = [0, 1, -3]
BABY = [0, 1, -3, 1]
GIANT = [0, 4, -8, 4]
SMALL_BSGS = ([0, 1], [0, 2, -4])


def _rand(rng, mod, n, batch):
    return orc.uniform_poly(mod, n, rng, batch=batch)


def _keys(rng, mod, n, L, steps):
    return [None if k == 0 else (_rand(rng, mod, n, L), _rand(rng, mod, n, L)) for k in steps]


def _place(rn, root_mod, n, drop):
    """(root, basis): a root basis of `root_mod`, and the basis under test --
    the root itself, or its drop_last(drop) view."""
    root = rn.RnsBasis(root_mod, n)
    return root, (root.drop_last(drop) if drop else root)


def _upload_keys(rn, basis, steps, keys, hoisted):
    out = []
    for k, kk in zip(steps, keys):
        gk = None if kk is None else rn.RnsGadgetKey.from_channels(kk[0], kk[1], basis, rotation=k)
        if gk is not None and hoisted:
            gk.prepare_hoisted()
        out.append(gk)
    return out


class Case:
    """Random ciphertexts and ordinary key channels on one ring; the keys
    uploaded and turned into their hoisting form.  With `drop`, the L limbs
    are a drop_last(drop) view of a root basis of L + drop primes (`root`)."""

    def __init__(self, rn, log_n, L, B, bits, steps=STEPS, seed=0, edge=False, drop=0):
        self.rn, self.n, self.L, self.B, self.steps = rn, 1 << log_n, L, B, list(steps)
        n = self.n
        self.root_mod = rn.generate_primes(bits, L + drop, n)
        self.mod = self.root_mod[:L]
        rng = np.random.default_rng(4100 + 37 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.keys = _keys(rng, self.mod, n, L, self.steps)
        if edge:  # an all-(q-1) ciphertext and an all-(q-1) key
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.c0[B - 1] = self.c1[B - 1] = np.broadcast_to(qm1, (L, n))
            t = next(i for i, k in enumerate(self.steps) if k != 0)
            self.keys[t][0][:] = np.broadcast_to(qm1, (L, L, n))
            self.keys[t][1][:] = np.broadcast_to(qm1, (L, L, n))
        self.root, self.basis = _place(rn, self.root_mod, n, drop)
        Bd = self.basis
        self.Bo = orc.Basis(self.mod, n)
        self.gk = _upload_keys(rn, Bd, self.steps, self.keys, True)
        self.kset = rn.RnsGadgetKeySet(self.gk, Bd)
        self.ct = rn.Ciphertext(rn.RnsPoly.from_channels(self.c0, Bd), rn.RnsPoly.from_channels(self.c1, Bd))

    def run(self, out=None):
        return self.rn.rotate_ciphertext_hoisted(self.ct, self.kset, out=out)

    def reference(self, p, t, c0=None, c1=None):
        c0 = self.c0 if c0 is None else c0
        c1 = self.c1 if c1 is None else c1
        return rotate_hoisted_ref(self.Bo, c0[p], c1[p], self.steps[t], *(self.keys[t] or (None, None)))


def _check_rotations(c, g0, g1, c0=None, c1=None):
    for p in sorted({0, c.B - 1}):
        for t in range(len(c.steps)):
            r0, r1 = c.reference(p, t, c0, c1)
            assert np.array_equal(g0[t * c.B + p], r0), f"out0 of step {t} ({c.steps[t]}), ciphertext {p}"
            assert np.array_equal(g1[t * c.B + p], r1), f"out1 of step {t} ({c.steps[t]}), ciphertext {p}"


@pytest.mark.parametrize("log_n,L,B,bits,ws_mb,edge,steps", [
    (8, 3, 3, 31, None, False, STEPS),   # small four-step grid
    (8, 3, 3, 31, None, True, STEPS),    # the same with an all-(q-1) ciphertext and key
    (14, 3, 3, 31, "1", False, STEPS),   # three one-ciphertext chunks
    (12, 3, 2, 61, None, False, STEPS),  # u64 kernels
    (14, 2, 2, 61, None, False, STEPS),  # u64 rows of 128 words
    (16, 4, 2, 31, None, False, SMALL),  # the matrix-core ring
    (17, 4, 1, 31, None, False, SMALL),  # the KSPLIT ring
    (12, 3, 2, 31, None, False, STEPS),  # whole-plane ring
])
def test_rotate_hoisted_parity(gpu, monkeypatch, log_n, L, B, bits, ws_mb, edge, steps):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    c = Case(gpu, log_n, L, B, bits, steps=steps, edge=edge)
    out = c.run()
    assert out.c0.n_polys == len(steps) * B and out.c1.n_polys == len(steps) * B
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    g0, g1 = out.c0.channels(), out.c1.channels()
    _check_rotations(c, g0, g1)
    # the step-0 slots are the ciphertext itself, every poly of it
    z = steps.index(0)
    assert np.array_equal(g0[z * B:(z + 1) * B], c.c0) and np.array_equal(g1[z * B:(z + 1) * B], c.c1)


@pytest.mark.parametrize("log_n,L,bits", [(8, 3, 31), (12, 3, 61), (16, 2, 31)])
def test_key_prepare_hoisted(gpu, log_n, L, bits):
    """NTT(sigma_k^-1(key)) as the oracle computes it, from both entry
    domains; k = 0 is rnt_key_prepare."""
    rn, lib = gpu, gpu.load()
    n = 1 << log_n
    mod = rn.generate_primes(bits, L, n)
    Bd, Bo = rn.RnsBasis(mod, n), orc.Basis(mod, n)
    rng = np.random.default_rng(51 + log_n)
    ka, kb = _rand(rng, mod, n, L), _rand(rng, mod, n, L)
    for k in (1, -3, 5, 0):
        want = [np.stack([orc.to_ntt(Bo, p) for p in (hoisting_form_coeff(Bo, x, k) if k else x)]) for x in (ka, kb)]
        for from_ntt in (False, True):
            a, b = rn.RnsPoly.from_channels(ka, Bd), rn.RnsPoly.from_channels(kb, Bd)
            if from_ntt:
                a.to_ntt_domain()
                b.to_ntt_domain()
            rn.check(lib.rnt_key_prepare_hoisted(a.handle, b.handle, k))
            assert a.is_ntt_domain() and b.is_ntt_domain()
            assert np.array_equal(a.channels(), want[0]), (k, from_ntt)
            assert np.array_equal(b.channels(), want[1]), (k, from_ntt)
    # k = 0 against rnt_key_prepare itself
    a, b = rn.RnsPoly.from_channels(ka, Bd), rn.RnsPoly.from_channels(kb, Bd)
    rn.check(lib.rnt_key_prepare(a.handle, b.handle))
    assert np.array_equal(a.channels(), want[0]) and np.array_equal(b.channels(), want[1])


@pytest.mark.parametrize("log_n,L,B,bits", [(8, 3, 3, 31), (12, 3, 2, 31)])
def test_single_step_calls_equal_the_multi_step_call(gpu, log_n, L, B, bits):
    """Group and ordering independence: n_steps = 1, a call per step."""
    c = Case(gpu, log_n, L, B, bits, seed=1)
    rn = c.rn
    out = c.run()
    g0, g1 = out.c0.channels(), out.c1.channels()
    for t, k in enumerate(c.steps):
        one = rn.rotate_ciphertext_hoisted(c.ct, rn.RnsGadgetKeySet([c.gk[t]], c.basis))
        assert one.c0.n_polys == B
        assert np.array_equal(one.c0.channels(), g0[t * B:(t + 1) * B]), (t, k)
        assert np.array_equal(one.c1.channels(), g1[t * B:(t + 1) * B]), (t, k)


def test_unaligned_planes(gpu):
    """The scalar instantiations: c1 and the key set wrapped at an offset of
    one word, so no plane is 16-byte aligned."""
    import torch

    c = Case(gpu, 8, 3, 3, 31, seed=2)
    rn, Bd = c.rn, c.basis
    dev = torch.device("cuda", Bd.device)

    def shifted(src):
        words = src.n_polys * c.L * c.n
        t = torch.zeros(words + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(Bd, t.data_ptr() + 4, src.n_polys, in_ntt_domain=src.is_ntt_domain(), owner=t)
        assert v.device_ptr()[0] % 16 == 4
        v.copy_polys(src)
        return v

    want = c.run()
    ks = rn.RnsGadgetKeySet(c.gk, Bd)
    ks.a, ks.b = shifted(c.kset.a), shifted(c.kset.b)
    ct = rn.Ciphertext(c.ct.c0, shifted(c.ct.c1))
    got = rn.rotate_ciphertext_hoisted(ct, ks)
    assert np.array_equal(got.c0.channels(), want.c0.channels())
    assert np.array_equal(got.c1.channels(), want.c1.channels())


def test_launch_counts(gpu):
    """One chunk, five nonzero steps: no key-switch rows and no per-step
    decomposition -- the digits once, ceil(5 / 4) k_hoist_mac launches."""
    c = Case(gpu, 14, 3, 2, 31)
    c.run()  # warm: workspaces cached
    c.basis.profile_enable(True)
    c.run()
    names = ("ks_rows", "ks_decompose", "hoist_digits", "hoist_mac", "automorphism")
    counts = {k: c.basis.profile_read(k)[0] for k in names}
    c.basis.profile_enable(False)
    print(counts)
    nz = sum(k != 0 for k in c.steps)
    assert nz == 5
    assert counts["ks_rows"] == 0 and counts["ks_decompose"] == 0
    assert counts["hoist_digits"] == 1
    assert counts["hoist_mac"] == -(-nz // HOIST_T) == 2
    assert counts["automorphism"] == 2 * nz


@pytest.mark.parametrize("log_n,L,B,bits", [(14, 3, 2, 31), (12, 3, 2, 31)])
def test_captured(gpu, log_n, L, B, bits):
    """The call records into a graph; a replay after the input changed gives
    the new input's words."""
    c = Case(gpu, log_n, L, B, bits, seed=3)
    rn = c.rn
    eager = c.run()
    w0, w1 = eager.c0.channels(), eager.c1.channels()
    nb = len(c.steps) * B
    out = rn.Ciphertext(rn.RnsPoly(c.basis, nb), rn.RnsPoly(c.basis, nb))
    with c.basis.capture() as g:
        c.run(out=out)
    g.replay()
    c.basis.sync()
    assert np.array_equal(out.c0.channels(), w0) and np.array_equal(out.c1.channels(), w1)
    rng = np.random.default_rng(43)
    n0, n1 = _rand(rng, c.mod, c.n, B), _rand(rng, c.mod, c.n, B)
    c.ct.c0.copy_polys(rn.RnsPoly.from_channels(n0, c.basis))
    c.ct.c1.copy_polys(rn.RnsPoly.from_channels(n1, c.basis))
    g.replay()
    c.basis.sync()
    g0, g1 = out.c0.channels(), out.c1.channels()
    assert not np.array_equal(g0, w0)
    _check_rotations(c, g0, g1, n0, n1)


def test_errors(gpu):
    """Every validation rule of rnt_ct_rotate_hoisted, with its status and
    fields; a refused call leaves the outputs untouched."""
    c = Case(gpu, 8, 3, 2, 31, steps=[0, 1, -3])
    rn, lib, Bd, L, B, n = c.rn, c.rn.load(), c.basis, c.L, c.B, c.n
    rng = np.random.default_rng(44)
    mark0, mark1 = _rand(rng, c.mod, n, 3 * B), _rand(rng, c.mod, n, 3 * B)
    o0, o1 = rn.RnsPoly.from_channels(mark0, Bd), rn.RnsPoly.from_channels(mark1, Bd)
    steps = (ctypes.c_int32 * 3)(0, 1, -3)

    def call(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, st=steps, ns=3, ka=c.kset.a, kb=c.kset.b):
        h = lambda x: None if x is None else x.handle  # noqa: E731
        return lib.rnt_ct_rotate_hoisted(h(out0), h(out1), h(c0), h(c1), st, ns, h(ka), h(kb))

    def fails(kind, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(call(**kw))
        assert e.value.kind == kind, (kind, kw.keys())
        if fields is not None:
            assert e.value.fields == fields
        assert np.array_equal(o0.channels(), mark0) and np.array_equal(o1.channels(), mark1), kw.keys()

    def zeros(count, basis=Bd, ntt=True):
        return rn.RnsPoly.from_channels(np.zeros((count, L, n), np.uint64), basis, in_ntt_domain=ntt)

    fails("BadArgument", ns=0)
    fails("BadArgument", st=None)
    fails("BadArgument", out0=rn.RnsPoly(Bd, B))          # outputs of the wrong size
    fails("BadArgument", out1=rn.RnsPoly(Bd, 3 * B + 1))
    fails("BadArgument", ns=2, ka=zeros(2 * L), kb=zeros(2 * L))  # 3 B polys for 2 steps
    fails("BadArgument", out1=o0)                         # out0 aliases out1
    one = (ctypes.c_int32 * 1)(1)
    k1 = rn.RnsGadgetKeySet([c.gk[1]], Bd)
    fails("BadArgument", out0=c.ct.c0, out1=rn.RnsPoly(Bd, B), st=one, ns=1, ka=k1.a, kb=k1.b)
    fails("BadArgument", out0=rn.RnsPoly(Bd, B), out1=c.ct.c1, st=one, ns=1, ka=k1.a, kb=k1.b)
    other = rn.RnsBasis(c.mod, n)
    fails("BasisMismatch", c1=rn.RnsPoly.from_channels(c.c1, other))
    fails("BasisMismatch", out0=rn.RnsPoly(other, 3 * B))
    fails("BasisMismatch", ka=zeros(3 * L, other))
    ntt = c.ct.c0.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", c0=ntt)
    fails("DomainMismatch", c1=ntt)
    fails("DomainMismatch", ka=zeros(3 * L, ntt=False))
    fails("DomainMismatch", kb=zeros(3 * L, ntt=False))
    fails("BadArgument", ka=None)
    fails("BadArgument", kb=None)
    fails("ChannelCountMismatch", {"expected": 3 * L, "actual": 2 * L}, ka=zeros(2 * L))
    fails("ChannelCountMismatch", {"expected": 3 * L, "actual": L}, kb=zeros(L))
    # the valid call, and one whose steps are all 0 without key buffers
    v0, v1 = rn.RnsPoly(Bd, 3 * B), rn.RnsPoly(Bd, 3 * B)
    rn.check(call(out0=v0, out1=v1))
    _check_rotations(c, v0.channels(), v1.channels())
    z = (ctypes.c_int32 * 3)(0, 0, 0)
    rn.check(call(out0=v0, out1=v1, st=z, ka=None, kb=None))
    assert np.array_equal(v0.channels(), np.concatenate([c.c0] * 3))
    assert np.array_equal(v1.channels(), np.concatenate([c.c1] * 3))


def test_python_layer_guards_the_key_form(gpu):
    """The library cannot tell the two key forms apart; the wrappers do."""
    c = Case(gpu, 8, 3, 2, 31, steps=[0, 1, -3])
    rn, Bd = c.rn, c.basis
    plain = _upload_keys(rn, Bd, c.steps, c.keys, False)
    pset = rn.RnsGadgetKeySet(plain, Bd)
    assert c.kset.hoisted and not pset.hoisted and c.gk[1].hoisted and not plain[1].hoisted
    d = rn.RnsPoly.from_channels(_rand(np.random.default_rng(45), c.mod, c.n, 3), Bd)
    d.to_ntt_domain()
    with pytest.raises(ValueError):
        rn.rotate_ciphertext_hoisted(c.ct, pset)
    with pytest.raises(ValueError):
        rn.rotate_ciphertext(c.ct, c.gk[1])
    with pytest.raises(ValueError):
        rn.linear_transform(c.ct, d, c.kset)
    one = rn.RnsGadgetKeySet([None], Bd)
    d1 = rn.RnsPoly.from_channels(_rand(np.random.default_rng(46), c.mod, c.n, 3), Bd)
    d1.to_ntt_domain()
    with pytest.raises(ValueError):
        rn.linear_transform_bsgs(c.ct, d1, c.kset, one)
    with pytest.raises(ValueError):
        rn.linear_transform_bsgs_hoisted(c.ct, d1, pset, one)
    with pytest.raises(ValueError):
        rn.linear_transform_bsgs_hoisted(c.ct, d1, one, c.kset)
    with pytest.raises(ValueError):
        rn.RnsGadgetKeySet([c.gk[1], plain[2]], Bd)
    with pytest.raises(ValueError):
        c.gk[1].prepare_hoisted()  # already in hoisting form
    relin = rn.RnsGadgetKey.from_channels(c.keys[1][0], c.keys[1][1], Bd)
    with pytest.raises(ValueError):
        relin.prepare_hoisted()  # no rotation
    # a set without any key serves both forms
    out = rn.rotate_ciphertext_hoisted(c.ct, rn.RnsGadgetKeySet([None, None], Bd))
    assert np.array_equal(out.c0.channels(), np.concatenate([c.c0] * 2))


# ---------------------------------------------------------------------------
# rnt_ct_linear_bsgs_hoisted
# ---------------------------------------------------------------------------
class BsgsCase:
    def __init__(self, rn, log_n, L, B, bits, baby=BABY, giant=GIANT, seed=0, drop=0):
        self.rn, self.n, self.L, self.B = rn, 1 << log_n, L, B
        self.baby, self.giant = list(baby), list(giant)
        n, nt = self.n, len(baby) * len(giant)
        self.root_mod = rn.generate_primes(bits, L + drop, n)
        self.mod = self.root_mod[:L]
        rng = np.random.default_rng(5100 + 41 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.diag = _rand(rng, self.mod, n, nt)  # coefficient domain, poly j n1 + i
        self.bkeys, self.gkeys = _keys(rng, self.mod, n, L, baby), _keys(rng, self.mod, n, L, giant)
        self.root, self.basis = _place(rn, self.root_mod, n, drop)
        Bd = self.basis
        self.bset = rn.RnsGadgetKeySet(_upload_keys(rn, Bd, self.baby, self.bkeys, True), Bd)
        self.gset = rn.RnsGadgetKeySet(_upload_keys(rn, Bd, self.giant, self.gkeys, False), Bd)
        self.d = rn.RnsPoly.from_channels(self.diag, Bd)
        self.d.to_ntt_domain()
        self.ct = rn.Ciphertext(rn.RnsPoly.from_channels(self.c0, Bd), rn.RnsPoly.from_channels(self.c1, Bd))

    def run(self, out=None):
        return self.rn.linear_transform_bsgs_hoisted(self.ct, self.d, self.bset, self.gset, out=out)

    def reference(self, p):
        Bo = orc.Basis(self.mod, self.n)
        return bsgs_hoisted_ref(Bo, self.c0[p], self.c1[p], self.baby, self.giant, self.diag, self.bkeys,
                                self.gkeys, threads=T)


@pytest.mark.parametrize("log_n,L,B,bits,ws_mb,steps", [
    (8, 3, 3, 31, None, None),         # small four-step grid
    (14, 3, 3, 31, "1", None),         # three one-ciphertext chunks
    (12, 3, 2, 61, None, None),        # u64 kernels
    (16, 4, 2, 31, None, SMALL_BSGS),  # the matrix-core ring
    (12, 3, 2, 31, None, None),        # whole-plane ring
])
def test_bsgs_hoisted_parity(gpu, monkeypatch, log_n, L, B, bits, ws_mb, steps):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)
    baby, giant = steps or (BABY, GIANT)
    c = BsgsCase(gpu, log_n, L, B, bits, baby=baby, giant=giant)
    out = c.run()
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    g0, g1 = out.c0.channels(), out.c1.channels()
    for p in sorted({0, B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from bsgs_hoisted_ref"


@pytest.mark.parametrize("log_n,L,B,bits", [(8, 3, 3, 31), (12, 3, 2, 31)])
def test_bsgs_hoisted_in_place(gpu, log_n, L, B, bits):
    c = BsgsCase(gpu, log_n, L, B, bits, seed=1)
    out = c.run()
    w0, w1 = out.c0.channels(), out.c1.channels()
    same = c.run(out=c.ct)
    assert same is c.ct
    assert np.array_equal(c.ct.c0.channels(), w0) and np.array_equal(c.ct.c1.channels(), w1)


def test_bsgs_hoisted_decomposition_count(gpu):
    """4 x 3 in one chunk: one digit launch for the three nonzero babies and
    one k_hoist_mac launch; a decomposition and a rows launch per nonzero
    giant only (rnt_ct_linear_bsgs runs 5 of each)."""
    c = BsgsCase(gpu, 14, 3, 2, 31, baby=[0, 1, 2, 3], giant=[0, 4, 8])
    c.run()
    c.basis.profile_enable(True)
    c.run()
    counts = {k: c.basis.profile_read(k)[0] for k in ("ks_rows", "ks_decompose", "hoist_digits", "hoist_mac")}
    c.basis.profile_enable(False)
    print(counts)
    assert counts == {"ks_rows": 2, "ks_decompose": 2, "hoist_digits": 1, "hoist_mac": 1}


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _rolled(x, k):
    """Slot s of a rotation by k holds old slot s + |k|, conjugated for k < 0:
    rotate_slots composes the rotation by |k| with X -> X^(2N-1)."""
    r = np.roll(x, -abs(int(k)))
    return np.conj(r) if k < 0 else r


def test_engine_rotate_hoisted_end_to_end(gpu):
    """Encode -> encrypt -> CkksEngine.rotate_hoisted by [1, -3, 7, 16] ->
    decrypt -> decode at N = 64, 4 x 31-bit primes, scale 2^58, x uniform in
    (-1, 1), against the rolled slots.  The same pipeline on the CPU
    (tools/hoist_tolerance.py: oracle/pyoracle, encoder.py, numpy draws,
    tests/hoist_ref.py) decodes with a largest absolute error of 1.305e-5 over
    eight seeds (the plain rotation's: 1.255e-5).  Tolerance: 4 x 1.305e-5 =
    5.22e-5, the margin tools/bsgs_tolerance.py established for other random
    draws, the arithmetic being identical."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L = 64, 32, 4
    eng = CkksEngine(rn.generate_primes(31, L, n), n, error_std=3.2, hamming_weight=n // 2)
    rng = np.random.default_rng(79)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    steps = [1, -3, 7, 16]
    kset = eng.generate_rotation_key_set(sk, steps, rng, hoisted=True)
    assert kset.hoisted
    x = rng.uniform(-1, 1, slots)
    enc = rn.CkksEncoder(n, 58)
    ct = eng.encrypt(enc.encode(x, eng.basis), pk, rng)
    out = CkksEngine.rotate_hoisted(ct, kset)
    assert out.c0.n_polys == len(steps) and out.logp == 58 and out.logq == ct.logq
    dec = out.c1 * rn.RnsPoly.from_channels(np.broadcast_to(sk.channels(), (len(steps), L, n)).copy(), eng.basis)
    dec = dec + out.c0
    got = enc.decode(rn.Plaintext(dec, 58, slots))
    worst = 0.0
    for t, k in enumerate(steps):
        err = float(np.max(np.abs(got[t] - _rolled(x, k))))
        print(f"hoisted rotation by {k}: decode error {err:.3e}")
        worst = max(worst, err)
    assert worst <= 4 * 1.305e-5


def test_engine_linear_transform_bsgs_hoisted_end_to_end(gpu):
    """The 16-diagonal band of tools/bsgs_tolerance.py (baby [0,1,2,3] x giant
    [0,4,8,12], ciphertext scale 2^58, diagonal scale 2^30) through
    CkksEngine.linear_transform_bsgs_hoisted -> rescale -> decrypt -> decode
    against M x.  tools/hoist_tolerance.py measures 1.383e-5 as the largest
    error of bsgs_hoisted_ref over eight seeds; tolerance 4 x = 5.53e-5."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L = 64, 32, 4
    eng = CkksEngine(rn.generate_primes(31, L, n), n, error_std=3.2, hamming_weight=n // 2)
    rng = np.random.default_rng(80)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    baby, giant = [0, 1, 2, 3], [0, 4, 8, 12]
    bset = eng.generate_rotation_key_set(sk, baby, rng, hoisted=True)
    gset = eng.generate_rotation_key_set(sk, giant, rng)
    x = rng.uniform(-1, 1, slots)
    M = np.zeros((slots, slots))
    s = np.arange(slots)
    for d in range(16):
        M[s, (s + d) % slots] = rng.uniform(-1, 1, slots)
    enc_x, enc_d = rn.CkksEncoder(n, 58), rn.CkksEncoder(n, 30)
    ct = eng.encrypt(enc_x.encode(x, eng.basis), pk, rng)
    diags = eng.encode_diagonals_bsgs(M, baby, giant, enc_d)
    out = CkksEngine.linear_transform_bsgs_hoisted(ct, diags, bset, gset)
    assert out.logp == 58 + 30 and out.logq == ct.logq
    res = CkksEngine.rescale_ciphertext(out)
    pt = CkksEngine.decrypt_plaintext(res, CkksEngine.secret_on(sk, res.c0.basis))
    got = enc_x.decode(pt)
    y = M @ x
    err = float(np.max(np.abs(got - y)))
    print(f"hoisted bsgs linear transform decode error {err:.3e}, max|y| {np.max(np.abs(y)):.3f}")
    assert err <= 4 * 1.383e-5
