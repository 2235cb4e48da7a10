"""Rotate-and-sum on hybrid keys on the GPU (rnt_ct_rotsum_hybrid):

    A0   = sum_{t in NZ} sum_d sigma_{k_t}(D_d) key_b[t][d],   D_d = ModUp_d(c1)
    out0 = z c0 + sum_{t in NZ} sigma_{k_t}(c0) + ModDown(A0)
    out1 = z c1 +                                ModDown(A1)

with one ModUp and one forward transform for every step, the automorphism a
gather in the NTT domain (k_rotsum_mac), and two ModDowns however many steps
there are.  Exact arithmetic with canonical outputs, so the call must reproduce
the CPU yardstick (tests/rotsum_ref.py, itself checked in
tests/test_rotsum_ref.py) word for word, on every kind of ring the transforms
treat differently (the shapes of tests/test_gpu_hybrid_hoist.py, for the same
reasons).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from hybrid_ref import n_digits, restrict_key
from rns_ntt import _lib
from rotsum_ref import rotsum_hybrid_ref
from test_gpu_hybrid_hoist import SHAPES

pytestmark = pytest.mark.gpu

T = 8  # steps per k_rotsum_mac / k_rotsum_c0 launch (kRotsumT)
# two zeros (z = 2), a negative step, a repeated step, and ten nonzero steps: a
# full group of k_rotsum_mac and a partial one
STEPS = [0, 1, -3, 1, 5, 2, 0, 7, -1, 4, 3, 6]
assert sum(k != 0 for k in STEPS) > T
# from 2^16 on the CPU reference of the full list takes 4 to 8 s a ciphertext:
# those rings (whose transforms differ, not the key products) run a short list
BIG_STEPS = [0, 1, -3, 1, 0]


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


class Case:
    """Random ciphertexts over q_0..q_{Lv-1} and random ORDINARY key channels
    over q_0..q_{Lv-1}, p_0..p_{K-1} for every nonzero step, uploaded and
    packed.  `place`: "view" puts the ciphertexts on the drop_last(K) view of
    the key's root, "root" on an unrelated root basis."""

    def __init__(self, rn, log_n, Lv, K, alpha, B, bits, steps=STEPS, edge=False, place="view", seed=0,
                 n_special=None):
        self.rn, self.n, self.Lv, self.K, self.alpha, self.B = rn, 1 << log_n, Lv, K, alpha, B
        self.steps = list(steps)
        n = self.n
        self.emod = rn.generate_primes(bits, Lv + K, n)
        self.mod = self.emod[:Lv]
        self.beta = n_digits(Lv, alpha)
        rng = np.random.default_rng(9300 + 43 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        if edge:
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.c0[B - 1] = self.c1[B - 1] = np.broadcast_to(qm1, (Lv, n))
        self.keys = _keys(rng, self.emod, n, self.beta, self.steps, edge)
        self.ext = rn.RnsBasis(self.emod, n)
        self.basis = self.ext.drop_last(K) if place == "view" else rn.RnsBasis(self.mod, n)
        self.Bc, self.Be = orc.Basis(self.mod, n), orc.Basis(self.emod, n)
        self.hk = [None if kk is None else rn.RnsHybridKey.from_channels(kk[0], kk[1], self.ext, alpha, rotation=k,
                                                                        n_special=n_special)
                   for k, kk in zip(self.steps, self.keys)]
        self.kset = rn.RnsHybridKeySet(self.hk, alpha)
        self.ct = rn.Ciphertext(rn.RnsPoly.from_channels(self.c0, self.basis),
                                rn.RnsPoly.from_channels(self.c1, self.basis))

    def run(self, out=None):
        return self.rn.rotsum_ciphertext_hybrid(self.ct, self.kset, out=out)

    def reference(self, p, c0=None, c1=None):
        c0 = self.c0 if c0 is None else c0
        c1 = self.c1 if c1 is None else c1
        return rotsum_hybrid_ref(self.Bc, self.Be, c0[p], c1[p], self.steps, self.keys, self.alpha)

    def check(self, out, polys=None, c0=None, c1=None):
        assert out.c0.n_polys == self.B and out.c1.n_polys == self.B
        assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
        for p in (sorted({0, self.B - 1}) if polys is None else polys):
            r0, r1 = self.reference(p, c0, c1)
            assert np.array_equal(out.c0.channels_of(p)[0], r0), f"out0 of ciphertext {p} differs from rotsum_hybrid_ref"
            assert np.array_equal(out.c1.channels_of(p)[0], r1), f"out1 of ciphertext {p} differs from rotsum_hybrid_ref"


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb,edge", SHAPES)
def test_parity(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb, edge):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    c = Case(gpu, log_n, Lv, K, alpha, B, bits, steps=BIG_STEPS if log_n >= 16 else STEPS, edge=edge)
    c.check(c.run())


def test_more_than_eight_special_primes(gpu):
    """K = 9: the 16-limb tier of k_moddown."""
    c = Case(gpu, 8, 3, 9, 3, 2, 31, seed=10)
    c.check(c.run())


@pytest.mark.parametrize("log_n,bits", [(8, 31), (12, 61)])
def test_unrelated_root_placement(gpu, log_n, bits):
    c = Case(gpu, log_n, 3, 2, 2, 2, bits, place="root", seed=1)
    c.check(c.run())


@pytest.mark.parametrize("log_n", [8, 12])
def test_levelled_key_view_equals_the_restricted_copy(gpu, log_n):
    """A 5-limb chain with alpha = 2 and a ciphertext two limbs down: the key is
    the at_level view of the full key set (chosen by the wrapper from
    n_special), and the words are those of the call with restrict_key's copy on
    a root over q_0..q_2, p_0, p_1 -- and the reference's."""
    rn = gpu
    steps = STEPS
    top = Case(rn, log_n, 5, 2, 2, 2, 31, steps=steps, seed=2, n_special=2)
    n, q, p = top.n, top.mod, top.emod[5:]
    low_basis = top.ext.drop_last(4)
    c0, c1 = np.ascontiguousarray(top.c0[:, :3, :]), np.ascontiguousarray(top.c1[:, :3, :])
    ct = rn.Ciphertext(rn.RnsPoly.from_channels(c0, low_basis), rn.RnsPoly.from_channels(c1, low_basis))
    got = rn.rotsum_ciphertext_hybrid(ct, top.kset)  # the view at level 3, by itself
    explicit = rn.rotsum_ciphertext_hybrid(ct, top.kset.at_level(3))
    low = Case.__new__(Case)
    low.rn, low.n, low.Lv, low.K, low.alpha, low.B, low.steps = rn, n, 3, 2, 2, 2, steps
    low.mod, low.emod = q[:3], q[:3] + p
    low.c0, low.c1 = c0, c1
    low.keys = [None if kk is None else (restrict_key(kk[0], 5, 2, 3), restrict_key(kk[1], 5, 2, 3)) for kk in top.keys]
    low.ext = rn.RnsBasis(low.emod, n)
    low.hk = [None if kk is None else rn.RnsHybridKey.from_channels(kk[0], kk[1], low.ext, 2, rotation=k)
              for k, kk in zip(steps, low.keys)]
    low.kset = rn.RnsHybridKeySet(low.hk, 2)
    low.basis = rn.RnsBasis(q, n).drop_last(2)
    low.ct = rn.Ciphertext(rn.RnsPoly.from_channels(c0, low.basis), rn.RnsPoly.from_channels(c1, low.basis))
    low.Bc, low.Be = orc.Basis(low.mod, n), orc.Basis(low.emod, n)
    copy = low.run()
    for a in (got, explicit):
        assert np.array_equal(a.c0.channels(), copy.c0.channels()) and np.array_equal(a.c1.channels(), copy.c1.channels())
    low.check(got)


@pytest.mark.parametrize("log_n,bits", [(8, 31), (12, 31), (12, 61)])
def test_in_place(gpu, log_n, bits):
    c = Case(gpu, log_n, 3, 2, 2, 3, bits, seed=3)
    fresh = c.run()
    w0, w1 = fresh.c0.channels(), fresh.c1.channels()
    same = c.run(out=c.ct)
    assert same is c.ct
    assert np.array_equal(c.ct.c0.channels(), w0) and np.array_equal(c.ct.c1.channels(), w1)


def test_in_place_across_chunks(gpu, monkeypatch):
    monkeypatch.setenv("RNT_KS_WS_MB", "1")
    c = Case(gpu, 14, 3, 2, 2, 3, 31, steps=[0, 1, -3], seed=3)
    fresh = c.run()
    w0, w1 = fresh.c0.channels(), fresh.c1.channels()
    c.run(out=c.ct)
    assert np.array_equal(c.ct.c0.channels(), w0) and np.array_equal(c.ct.c1.channels(), w1)


@pytest.mark.parametrize("bits", [31, 61])
def test_all_steps_zero_with_null_keys(gpu, bits):
    rn = gpu
    c = Case(rn, 8, 3, 2, 2, 3, bits, steps=[0, 0, 0], seed=4)
    assert c.kset.a is None
    out = c.run()
    q = np.array(c.mod, dtype=np.uint64)[None, :, None]
    assert np.array_equal(out.c0.channels(), (3 * c.c0.astype(object) % q.astype(object)).astype(np.uint64))
    assert np.array_equal(out.c1.channels(), (3 * c.c1.astype(object) % q.astype(object)).astype(np.uint64))
    one = rn.rotsum_ciphertext_hybrid(c.ct, rn.RnsHybridKeySet([None], c.alpha))
    assert np.array_equal(one.c0.channels(), c.c0) and np.array_equal(one.c1.channels(), c.c1)
    c.run(out=c.ct)  # in place as well
    assert np.array_equal(c.ct.c0.channels(), out.c0.channels())


@pytest.mark.parametrize("bits", [31, 61])
def test_word_aligned_wrapped_buffers(gpu, bits):
    """The one-word instantiations: c0, c1, the key sets and the outputs wrapped
    one word past a 16-byte boundary, between guard words."""
    import torch

    c = Case(gpu, 8, 3, 2, 2, 3, bits, seed=5)
    rn, lib, Bd = c.rn, c.rn.load(), c.basis
    wb = 4 if bits == 31 else 8
    dev = torch.device("cuda", Bd.device)
    sentinel = np.uint32(0xA5A5A5A5)
    tensors = []

    def shifted(basis, n_polys, src=None, ntt=False):
        body = n_polys * basis.channel_count() * c.n * wb // 4
        t = torch.full((body + 8,), int(sentinel.astype(np.int32)), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(basis, t.data_ptr() + 16 + wb, n_polys, in_ntt_domain=ntt, owner=t)
        assert v.device_ptr()[0] % 16 == wb
        if src is not None:
            v.copy_polys(src)
        tensors.append((t, body))
        return v

    want = c.run()
    o0, o1 = shifted(Bd, c.B), shifted(Bd, c.B)
    s0, s1 = shifted(Bd, c.B, c.ct.c0), shifted(Bd, c.B, c.ct.c1)
    ka = shifted(c.ext, c.kset.a.n_polys, c.kset.a, ntt=True)
    kb = shifted(c.ext, c.kset.b.n_polys, c.kset.b, ntt=True)
    ns = len(c.steps)
    steps = (ctypes.c_int32 * ns)(*c.steps)
    rn.check(lib.rnt_ct_rotsum_hybrid(o0.handle, o1.handle, s0.handle, s1.handle, steps, ns, ka.handle, kb.handle,
                                      c.alpha))
    assert np.array_equal(o0.channels(), want.c0.channels()) and np.array_equal(o1.channels(), want.c1.channels())
    # in place on the shifted inputs
    rn.check(lib.rnt_ct_rotsum_hybrid(s0.handle, s1.handle, s0.handle, s1.handle, steps, ns, ka.handle, kb.handle,
                                      c.alpha))
    assert np.array_equal(s0.channels(), want.c0.channels()) and np.array_equal(s1.channels(), want.c1.channels())
    Bd.sync()
    torch.cuda.synchronize(dev)
    lead = 4 + wb // 4
    for t, body in tensors:
        h = t.cpu().numpy().view(np.uint32)
        assert (h[:lead] == sentinel).all() and (h[lead + body:] == sentinel).all()


def test_refusals_leave_the_outputs_untouched(gpu):
    c = Case(gpu, 8, 3, 2, 2, 2, 31, steps=[0, 1, -3], seed=6)
    rn, lib, Bd, Lv, B, n, beta = c.rn, c.rn.load(), c.basis, c.Lv, c.B, c.n, c.beta
    rng = np.random.default_rng(9358)
    mark0, mark1 = _rand(rng, c.mod, n, B), _rand(rng, c.mod, n, B)
    o0, o1 = rn.RnsPoly.from_channels(mark0, Bd), rn.RnsPoly.from_channels(mark1, Bd)
    steps = (ctypes.c_int32 * 3)(*c.steps)
    h = lambda x: None if x is None else x.handle  # noqa: E731

    def call(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, st=steps, ns=3, ka=c.kset.a, kb=c.kset.b, alpha=c.alpha):
        return lib.rnt_ct_rotsum_hybrid(h(out0), h(out1), h(c0), h(c1), st, ns, h(ka), h(kb), alpha)

    def fails(kind, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(call(**kw))
        assert e.value.kind == kind, (kind, kw.keys(), str(e.value))
        if fields is not None:
            assert e.value.fields == fields, e.value.fields
        assert np.array_equal(o0.channels(), mark0) and np.array_equal(o1.channels(), mark1), kw.keys()
        assert np.array_equal(c.ct.c0.channels(), c.c0) and np.array_equal(c.ct.c1.channels(), c.c1), kw.keys()

    def keypoly(count, basis=c.ext, ntt=True):
        return rn.RnsPoly.from_channels(np.zeros((count, basis.channel_count(), basis.degree), np.uint64), basis,
                                        in_ntt_domain=ntt)

    # hoisting-form keys: refused in Python, the library cannot tell
    hoisted = [None if kk is None else rn.RnsHybridKey.from_channels(kk[0], kk[1], c.ext, c.alpha, rotation=k)
               for k, kk in zip(c.steps, c.keys)]
    for k in hoisted:
        if k is not None:
            k.prepare_hoisted()
    with pytest.raises(ValueError, match="ordinary prepared"):
        rn.rotsum_ciphertext_hybrid(c.ct, rn.RnsHybridKeySet(hoisted, c.alpha), out=rn.Ciphertext(o0, o1))
    with pytest.raises(ValueError):
        rn.rotsum_ciphertext_hybrid(c.ct, c.hk[1])  # a key, not a set
    assert np.array_equal(o0.channels(), mark0) and np.array_equal(o1.channels(), mark1)
    # the key-count rule: n_steps beta polys
    fails("ChannelCountMismatch", {"expected": 3 * beta, "actual": 2 * beta}, ka=keypoly(2 * beta))
    fails("ChannelCountMismatch", {"expected": 3 * beta, "actual": beta}, kb=keypoly(beta))
    fails("ChannelCountMismatch", {"expected": 3 * Lv, "actual": 3 * beta}, alpha=1)
    ntt = c.ct.c1.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", c0=ntt)
    fails("DomainMismatch", c1=ntt)
    fails("DomainMismatch", ka=keypoly(3 * beta, ntt=False))
    fails("BadArgument", out1=o0)  # out0 == out1
    # an output that aliases a key: a buffer on C wrapped over the key set's own memory
    alias = rn.RnsPoly.wrap(Bd, c.kset.a.device_ptr()[0], B, in_ntt_domain=False, owner=c.kset.a)
    keywords = c.kset.a.channels()
    fails("BadArgument", out0=alias)
    fails("BadArgument", out1=alias)
    assert np.array_equal(c.kset.a.channels(), keywords)
    fails("BadArgument", out0=c.ct.c1)  # the other component
    fails("BadArgument", out1=c.ct.c0)
    fails("BadArgument", alpha=0)
    fails("BadArgument", ns=0)
    fails("BadArgument", st=None)
    fails("BadArgument", ka=None)
    fails("BadArgument", out0=rn.RnsPoly(Bd, B + 1))
    fails("BasisMismatch", c1=rn.RnsPoly.from_channels(c.c1, rn.RnsBasis(c.mod, n)))
    other = rn.RnsBasis(c.emod[1:] + c.emod[:1], n)
    fails("BasisMismatch", ka=keypoly(3 * beta, other), kb=keypoly(3 * beta, other))
    wide = rn.RnsBasis(c.mod + rn.generate_primes(61, 1, n), n)
    zero = {"degree": 0, "max_degree": 0}
    fails("Unsupported", zero, ka=keypoly(3 * beta, wide), kb=keypoly(3 * beta, wide))
    # a key level view in a ciphertext position
    full = Case(rn, 8, 4, 2, 2, 2, 31, steps=[0, 1, -3], seed=7, n_special=2)
    view = full.kset.at_level(3)
    for pos in ("out0", "out1", "c0", "c1"):
        fails("Unsupported", zero, **{pos: view.a})
    # the valid call still runs after all that
    out = rn.Ciphertext(o0, o1)
    c.check(c.run(out=out))


def _counts(basis, run):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in _lib.PROFILE_NAMES}
    basis.profile_enable(False)
    print({k: v for k, v in counts.items() if v})
    return counts


TRANSFORMS = ("col_fwd", "row_fwd", "row_inv", "col_inv", "mf_ntt_fwd", "mf_ntt_inv", "whole_fwd", "whole_inv")
SILENT = ("moddown_auto", "automorphism", "hoist_mac", "elementwise", "hoist_digits", "ks_decompose", "ks_rows",
          "ks_whole", "automorph_ntt", "moddown_rescale", "copy")


@pytest.mark.parametrize("log_n", [12, 14])
def test_launch_table(gpu, log_n):
    """One chunk, over every profile name: 1 ModUp, ceil(|NZ| / T) key-product
    launches, ceil(n_steps / T) launches of the c0 sum (plus one for z c1 where
    a step is 0), 2 ModDowns -- and ModUp, ModDown and the transforms the same
    for 3 and for T + 2 rotating steps."""
    seen = {}
    for steps in ([1, -3, 5], [0, 1, -3, 1, 5, 2, 0, 7, -1, 4, 3, 6], list(range(1, T + 3))):
        c = Case(gpu, log_n, 3, 2, 2, 2, 31, steps=steps, seed=8)
        counts = _counts(c.basis, c.run)
        nz = sum(k != 0 for k in steps)
        z = len(steps) - nz
        assert counts["modup"] == 1 and counts["moddown"] == 2, counts
        assert counts["rotsum_mac"] == -(-nz // T)
        assert counts["rotsum_c0"] == -(-len(steps) // T) + (1 if z else 0)
        for k in SILENT:
            assert counts[k] == 0, k
        seen[len(steps)] = tuple(counts[k] for k in TRANSFORMS)
        known = {"modup", "moddown", "rotsum_mac", "rotsum_c0", *TRANSFORMS}
        assert all(v == 0 for k, v in counts.items() if k not in known), counts
    assert len(set(seen.values())) == 1 and sum(next(iter(seen.values()))) > 0, seen


def test_launch_table_chunked(gpu, monkeypatch):
    """RNT_KS_WS_MB=1 at 2^14 x (3 + 2) limbs: a chunk is one ciphertext, so
    every per-chunk count is multiplied by B."""
    monkeypatch.setenv("RNT_KS_WS_MB", "1")
    B = 3
    c = Case(gpu, 14, 3, 2, 2, B, 31, steps=[0, 1, -3, 5], seed=9)
    counts = _counts(c.basis, c.run)
    assert counts["modup"] == B and counts["moddown"] == 2 * B
    assert counts["rotsum_mac"] == B and counts["rotsum_c0"] == 2 * B
    for k in SILENT:
        assert counts[k] == 0, k


@pytest.mark.parametrize("log_n", [12, 14])
def test_captured(gpu, log_n):
    """After one plain run the call records into a graph; two replays on
    refreshed inputs give the eager words."""
    c = Case(gpu, log_n, 3, 2, 2, 2, 31, steps=[0, 1, -3, 5], seed=11)
    rn = c.rn
    rout = rn.Ciphertext(rn.RnsPoly(c.basis, c.B), rn.RnsPoly(c.basis, c.B))
    c.run(out=rout)
    with c.basis.capture() as g:
        c.run(out=rout)
    rng = np.random.default_rng(9357 + log_n)
    for _ in range(2):
        n0, n1 = _rand(rng, c.mod, c.n, c.B), _rand(rng, c.mod, c.n, c.B)
        c.ct.c0.copy_polys(rn.RnsPoly.from_channels(n0, c.basis))
        c.ct.c1.copy_polys(rn.RnsPoly.from_channels(n1, c.basis))
        g.replay()
        c.basis.sync()
        got0, got1 = rout.c0.channels(), rout.c1.channels()
        plain = c.run()
        assert np.array_equal(got0, plain.c0.channels()) and np.array_equal(got1, plain.c1.channels())
        c.check(rout, polys=[0], c0=n0, c1=n1)
