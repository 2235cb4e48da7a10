"""The double-hoisted baby-step giant-step transform on hybrid keys on the GPU
(rnt_ct_linear_bsgs_hybrid_dh and its _rescale form): the baby key products stay
over E in the NTT domain, k_dh_bsgs_mac reads them through sigma's permutation
and forms the inner sums over E, k_dh_bsgs_fold starts the giant accumulators,
and only one component per rotating giant and the two final sums see a ModDown.
Exact arithmetic with canonical outputs, so the calls must reproduce the CPU
yardstick (tests/dh_bsgs_ref.py, itself pinned in tests/test_dh_bsgs_ref.py)
word for word, on every kind of ring the transforms treat differently.
"""
from __future__ import annotations

import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pyoracle as orc
from dh_bsgs_ref import dh_bsgs_ref
from hybrid_ref import n_digits, restrict_key

pytestmark = pytest.mark.gpu

DH_JT, DH_BT, HOIST_T = 4, 16, 4  # giants / babies per k_dh_bsgs_mac launch, steps per k_hoist_mac launch
# a zero and a negative baby; two zero giants, a gap between the nonzero ones, a negative giant
BABY, GIANT = [0, 1, -3], [4, 0, -8, 0]

# log_n, Lv, K, alpha, B, bits, ws_mb, edge
SHAPES = [
    (8, 3, 2, 2, 3, 31, None, False),   # small four-step grid, partial last digit
    (8, 3, 2, 2, 3, 31, None, True),    # all-(q-1) ciphertext, all-(m-1) keys and plaintexts
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


def _upload(rn, ext, alpha, steps, keys, hoisted, n_special=None):
    out = []
    for k, kk in zip(steps, keys):
        hk = None if kk is None else rn.RnsHybridKey.from_channels(kk[0], kk[1], ext, alpha, rotation=k,
                                                                   n_special=n_special)
        if hk is not None and hoisted:
            hk.prepare_hoisted()
        out.append(hk)
    return out


class DhCase:
    """Random ciphertexts over q_0..q_{Lv-1}, random ORDINARY key channels and
    random plaintext words over q_0..q_{Lv-1}, p_0..p_{K-1}; the baby keys in
    hoisting form, the giant keys ordinary (the key sets rnt_ct_linear_bsgs_hybrid
    takes), the plaintexts on the keys' root in the NTT domain."""

    def __init__(self, rn, log_n, Lv, K, alpha, B, bits, baby=BABY, giant=GIANT, edge=False, seed=0, n_special=None):
        self.rn, self.n, self.Lv, self.K, self.alpha, self.B = rn, 1 << log_n, Lv, K, alpha, B
        self.baby, self.giant = list(baby), list(giant)
        n, nt = self.n, len(baby) * len(giant)
        self.emod = rn.generate_primes(bits, Lv + K, n)
        self.mod = self.emod[:Lv]
        self.beta = n_digits(Lv, alpha)
        rng = np.random.default_rng(8300 + 53 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.diagE = _rand(rng, self.emod, n, nt)  # coefficient domain over E, poly j n1 + i
        if edge:
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.c0[B - 1] = self.c1[B - 1] = np.broadcast_to(qm1, (Lv, n))
            self.diagE[:] = np.array(self.emod, dtype=np.uint64)[None, :, None] - np.uint64(1)
        self.bkeys = _keys(rng, self.emod, n, self.beta, self.baby, edge)
        self.gkeys = _keys(rng, self.emod, n, self.beta, self.giant, edge)
        self.ext = rn.RnsBasis(self.emod, n)
        self.basis = self.ext.drop_last(K)
        self.Bc, self.Be = orc.Basis(self.mod, n), orc.Basis(self.emod, n)
        self.bset = rn.RnsHybridKeySet(_upload(rn, self.ext, alpha, self.baby, self.bkeys, True, n_special), alpha)
        self.gset = rn.RnsHybridKeySet(_upload(rn, self.ext, alpha, self.giant, self.gkeys, False, n_special), alpha)
        self.d = rn.RnsPoly.from_channels(self.diagE, self.ext)
        self.d.to_ntt_domain()
        up = lambda x: rn.RnsPoly.from_channels(x, self.basis)  # noqa: E731
        self.ct = rn.Ciphertext(up(self.c0), up(self.c1))

    def run(self, out=None, rescale=False):
        return self.rn.linear_bsgs_hybrid_dh(self.ct, self.d, self.bset, self.gset, rescale=rescale, out=out)

    def reference(self, p, c0=None, c1=None):
        c0 = self.c0 if c0 is None else c0
        c1 = self.c1 if c1 is None else c1
        args = (self.Bc, self.Be, c0[p], c1[p], self.baby, self.giant, self.diagE, self.bkeys, self.gkeys, self.alpha)
        if self.n < (1 << 16):
            return dh_bsgs_ref(*args)
        with ThreadPoolExecutor(4) as pool:  # (the babies, then the giants, side by side: seconds at 2^17)
            return dh_bsgs_ref(*args, pmap=pool.map)

    def check(self, out, polys=None, c0=None, c1=None):
        assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
        for p in (sorted({0, self.B - 1}) if polys is None else polys):
            r0, r1 = self.reference(p, c0, c1)
            assert np.array_equal(out.c0.channels_of(p)[0], r0), f"out0 of ciphertext {p} differs from dh_bsgs_ref"
            assert np.array_equal(out.c1.channels_of(p)[0], r1), f"out1 of ciphertext {p} differs from dh_bsgs_ref"


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb,edge", SHAPES)
def test_parity(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb, edge):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    c = DhCase(gpu, log_n, Lv, K, alpha, B, bits, edge=edge)
    out = c.run()
    assert out.c0.n_polys == B and out.c0.basis is c.basis
    c.check(out)


@pytest.mark.parametrize("log_n,bits", [(8, 31), (12, 61)])
def test_no_zero_step_anywhere(gpu, log_n, bits):
    c = DhCase(gpu, log_n, 3, 2, 2, 2, bits, baby=[1, 2], giant=[3, -5], seed=1)
    c.check(c.run())


@pytest.mark.parametrize("log_n,bits", [(8, 31), (12, 31), (12, 61)])
@pytest.mark.parametrize("baby,giant", [([0], [0]), ([0, 0], [0, 0])])
def test_all_zero_steps_without_keys_is_the_device_product(gpu, log_n, bits, baby, giant):
    """ModDown(P x) = x: no key buffer is read (both sets are NULL) and the
    words are those of rnt_mul and rnt_add on the device."""
    rn = gpu
    c = DhCase(rn, log_n, 3, 2, 2, 2, bits, baby=baby, giant=giant, seed=2)
    assert c.bset.a is None and c.gset.a is None
    out = c.run()
    w0 = w1 = None
    for t in range(len(baby) * len(giant)):
        dc = rn.RnsPoly.from_channels(np.broadcast_to(c.diagE[t][:c.Lv], (c.B, c.Lv, c.n)).copy(), c.basis)
        p0, p1 = c.ct.c0 * dc, c.ct.c1 * dc
        w0, w1 = (p0, p1) if w0 is None else (w0 + p0, w1 + p1)
    assert np.array_equal(out.c0.channels(), w0.channels()) and np.array_equal(out.c1.channels(), w1.channels())
    c.check(out, polys=[1])


@pytest.mark.parametrize("log_n,Lv,bits,baby,giant", [(8, 3, 31, BABY, GIANT), (12, 3, 61, BABY, GIANT),
                                                      (14, 2, 31, [0, 2], [0]), (16, 3, 31, [1], [0, 2])])
def test_rescale_form_is_the_call_then_the_rescale(gpu, log_n, Lv, bits, baby, giant):
    rn = gpu
    c = DhCase(rn, log_n, Lv, 2, 2, 2, bits, baby=baby, giant=giant, seed=3)
    plain = c.run()
    want = rn.rescale_ciphertext(plain)
    got = c.run(rescale=True)
    assert got.c0.basis.channel_count() == Lv - 1 and not got.c0.is_ntt_domain()
    assert np.array_equal(got.c0.channels(), want.c0.channels())
    assert np.array_equal(got.c1.channels(), want.c1.channels())


@pytest.mark.parametrize("log_n", [8, 12])
def test_in_place(gpu, log_n):
    c = DhCase(gpu, log_n, 3, 2, 2, 2, 31, seed=4)
    out = c.run()
    w0, w1 = out.c0.channels(), out.c1.channels()
    same = c.run(out=c.ct)
    assert same is c.ct
    assert np.array_equal(c.ct.c0.channels(), w0) and np.array_equal(c.ct.c1.channels(), w1)


@pytest.mark.parametrize("log_n", [8, 12, 14])
def test_levelled_through_key_level_views(gpu, log_n):
    """A 4-limb chain with alpha = 2: one level down the call reads the full
    key sets through their level views, the plaintexts live on a root over
    q_0..q_2, p_0, p_1, and the words are the call's with the restricted keys."""
    rn = gpu
    top = DhCase(rn, log_n, 4, 2, 2, 2, 31, baby=[0, 1, -3], giant=[2, 0], seed=5, n_special=2)
    top.check(top.run(), polys=[1])
    n, q, p = top.n, top.mod, top.emod[4:]
    low_emod = q[:3] + p
    c0, c1 = np.ascontiguousarray(top.c0[:, :3, :]), np.ascontiguousarray(top.c1[:, :3, :])
    basis = top.ext.drop_last(3)
    ct = rn.Ciphertext(rn.RnsPoly.from_channels(c0, basis), rn.RnsPoly.from_channels(c1, basis))
    rng = np.random.default_rng(95 + log_n)
    diagE = _rand(rng, low_emod, n, 6)
    d = rn.RnsPoly.from_channels(diagE, rn.RnsBasis(low_emod, n))
    d.to_ntt_domain()
    assert rn.hybrid_level_moduli(top.ext, 2, 3) == low_emod
    out = rn.linear_bsgs_hybrid_dh(ct, d, top.bset, top.gset)
    assert top.bset.at_level(3).a.basis is top.ext.hybrid_level(2, 3)
    low = lambda keys: [None if kk is None else (restrict_key(kk[0], 4, 2, 3), restrict_key(kk[1], 4, 2, 3))  # noqa: E731
                        for kk in keys]
    r0, r1 = dh_bsgs_ref(orc.Basis(q[:3], n), orc.Basis(low_emod, n), c0[1], c1[1], top.baby, top.giant, diagE,
                         low(top.bkeys), low(top.gkeys), 2)
    assert np.array_equal(out.c0.channels_of(1)[0], r0) and np.array_equal(out.c1.channels_of(1)[0], r1)
    res = rn.linear_bsgs_hybrid_dh(ct, d, top.bset, top.gset, rescale=True)
    want = rn.rescale_ciphertext(out)
    assert np.array_equal(res.c0.channels(), want.c0.channels()) and np.array_equal(res.c1.channels(), want.c1.channels())


@pytest.mark.parametrize("off,bits", [("ciphertext", 31), ("keys", 31), ("plaintexts", 31), ("plaintexts", 61)])
def test_unaligned_planes(gpu, off, bits):
    """One operand wrapped at an offset of one word, the others 16-byte aligned.
    The plaintexts are the only caller's buffer k_dh_bsgs_mac reads (its other
    operands are blocks of the call's workspace), so the "plaintexts" cases are
    the ones that run its one-word form, u32 and u64; k_dh_bsgs_fold reads
    workspace alone and has no one-word form.  With the ciphertext and the
    outputs, or the four key sets, off, the one-word forms of the call's other
    kernels (the copies, k_hoist_mac, k_moddown) run around the 16-byte inner
    sums."""
    import torch

    c = DhCase(gpu, 8, 3, 2, 2, 3, bits, seed=6)
    rn, lib = c.rn, c.rn.load()
    dev = torch.device("cuda", c.basis.device)
    wb = 4 if bits <= 32 else 8

    def shifted(basis, n_polys, src=None, ntt=False, on=True):
        words = n_polys * basis.channel_count() * c.n
        t = torch.zeros(words * wb // 4 + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(basis, t.data_ptr() + (wb if on else 0), n_polys, in_ntt_domain=ntt, owner=t)
        assert v.device_ptr()[0] % 16 == (wb if on else 0)
        if src is not None:
            v.copy_polys(src)
        return v

    want = c.run()
    ct_off, k_off, d_off = off == "ciphertext", off == "keys", off == "plaintexts"
    o0, o1 = shifted(c.basis, c.B, on=ct_off), shifted(c.basis, c.B, on=ct_off)
    t0, t1 = shifted(c.basis, c.B, c.ct.c0, on=ct_off), shifted(c.basis, c.B, c.ct.c1, on=ct_off)
    d = shifted(c.ext, c.d.n_polys, c.d, ntt=True, on=d_off)
    sets = [shifted(c.ext, x.n_polys, x, ntt=True, on=k_off) for x in (c.bset.a, c.bset.b, c.gset.a, c.gset.b)]
    baby, giant = (ctypes.c_int32 * len(c.baby))(*c.baby), (ctypes.c_int32 * len(c.giant))(*c.giant)
    rn.check(lib.rnt_ct_linear_bsgs_hybrid_dh(o0.handle, o1.handle, t0.handle, t1.handle, baby, len(c.baby), giant,
                                              len(c.giant), d.handle, *[x.handle for x in sets], c.alpha))
    assert np.array_equal(o0.channels(), want.c0.channels()) and np.array_equal(o1.channels(), want.c1.channels())


def test_plaintexts_in_the_making_on_their_own_stream_are_waited_for(gpu):
    """Below the top level the plaintexts live on a root context of their own,
    with its own stream.  The call orders itself after what that stream holds:
    forty transforms back and forth are queued on the plaintexts right before
    the call -- in between they are coefficient-domain words -- and no sync."""
    rn = gpu
    c = DhCase(rn, 14, 3, 2, 2, 2, 31, seed=15)
    want = c.run()
    w0, w1 = want.c0.channels(), want.c1.channels()
    other = rn.RnsBasis(c.emod, c.n)
    assert other.stream() != c.basis.stream()
    d = rn.RnsPoly.from_channels(c.diagE, other)
    d.to_ntt_domain()
    c.basis.sync()
    other.sync()
    for _ in range(40):
        d.to_coeff_domain()
        d.to_ntt_domain()
    out = rn.linear_bsgs_hybrid_dh(c.ct, d, c.bset, c.gset)
    assert np.array_equal(out.c0.channels(), w0) and np.array_equal(out.c1.channels(), w1)


def test_large_batch_grids(gpu):
    """64 ciphertexts at 2^14 (1024 workgroups of vectors): the un-split grids
    of k_modup and k_moddown under the new call."""
    c = DhCase(gpu, 14, 3, 2, 2, 64, 31, baby=[1, -3], giant=[2, 0], seed=7)
    c.check(c.run(), polys=[63])


def test_more_than_eight_special_primes(gpu):
    """K = 9: the 16-limb tier of k_moddown, and inner sums over 12 limbs for a
    ciphertext of 3."""
    c = DhCase(gpu, 8, 3, 9, 3, 2, 31, seed=8)
    c.check(c.run(), polys=[1])


def test_more_babies_and_giants_than_one_launch_takes(gpu):
    """17 babies and 5 giants: two baby groups (the second accumulates) and two
    giant groups (the second fold accumulates) of k_dh_bsgs_mac."""
    baby = [0] + list(range(1, DH_BT + 1))
    giant = [0, 17, 34, -3, 51]
    c = DhCase(gpu, 8, 3, 2, 2, 2, 31, baby=baby, giant=giant, seed=9)
    from rns_ntt import _lib

    counts = _counts(c.basis, c.run, _lib.PROFILE_NAMES)
    assert counts["dh_bsgs_mac"] == 2 * 2 and counts["dh_bsgs_fold"] == 2
    c.check(c.run(), polys=[1])


TRANSFORMS_FWD = ("col_fwd", "row_fwd", "mf_ntt_fwd", "whole_fwd")
TRANSFORMS_INV = ("row_inv", "col_inv", "mf_ntt_inv", "whole_inv")


def _counts(basis, run, names):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in names}
    basis.profile_enable(False)
    print({k: v for k, v in counts.items() if v})
    return counts


def test_launch_counts(gpu):
    """One chunk at 2^14 (a transform is one whole-plane launch): one ModUp for
    the baby stage plus one per rotating giant; |NZ| + 2 ModDowns and as many
    inverse transforms over E; no k_moddown_auto, no plaintext pass; one
    k_dh_bsgs_mac and one k_dh_bsgs_fold."""
    from rns_ntt import _lib

    c = DhCase(gpu, 14, 3, 2, 2, 2, 31, seed=10)
    counts = _counts(c.basis, c.run, _lib.PROFILE_NAMES)
    nzg = sum(g != 0 for g in c.giant)
    nzb = sum(b != 0 for b in c.baby)
    assert nzg == 2 and nzb == 2
    assert counts["modup"] == 1 + nzg
    assert counts["moddown"] + counts["moddown_rescale"] + counts["moddown_auto"] == nzg + 2
    assert counts["moddown"] == nzg + 2 and counts["moddown_auto"] == 0
    assert counts["whole_inv"] == nzg + 2 and sum(counts[k] for k in TRANSFORMS_INV) == nzg + 2
    assert counts["whole_fwd"] == 2 + 1 + nzg and sum(counts[k] for k in TRANSFORMS_FWD) == 3 + nzg
    assert counts["dh_bsgs_mac"] == -(-len(c.giant) // DH_JT) * -(-len(c.baby) // DH_BT) == 1
    assert counts["dh_bsgs_fold"] == 1
    assert counts["hoist_mac"] == -(-nzb // HOIST_T) + nzg
    assert counts["automorphism"] == nzg
    known = {"modup", "moddown", "whole_inv", "whole_fwd", "dh_bsgs_mac", "dh_bsgs_fold", "hoist_mac", "automorphism"}
    assert all(v == 0 for k, v in counts.items() if k not in known), counts
    # the rescaling form closes with two k_moddown_rescale instead
    counts = _counts(c.basis, lambda: c.run(rescale=True), _lib.PROFILE_NAMES)
    assert counts["moddown"] == nzg and counts["moddown_rescale"] == 2 and counts["moddown_auto"] == 0


@pytest.mark.parametrize("log_n", [12, 14])
def test_captured(gpu, log_n):
    """The call records into a graph after one plain run; two replays on
    refreshed inputs give the words of the eager call."""
    c = DhCase(gpu, log_n, 3, 2, 2, 2, 31, seed=11)
    rn = c.rn
    out = rn.Ciphertext(rn.RnsPoly(c.basis, c.B), rn.RnsPoly(c.basis, c.B))
    c.run(out=out)
    with c.basis.capture() as g:
        c.run(out=out)
    rng = np.random.default_rng(67 + log_n)
    for _ in range(2):
        n0, n1 = _rand(rng, c.mod, c.n, c.B), _rand(rng, c.mod, c.n, c.B)
        c.ct.c0.copy_polys(rn.RnsPoly.from_channels(n0, c.basis))
        c.ct.c1.copy_polys(rn.RnsPoly.from_channels(n1, c.basis))
        g.replay()
        c.basis.sync()
        got0, got1 = out.c0.channels(), out.c1.channels()
        plain = c.run()
        assert np.array_equal(got0, plain.c0.channels()) and np.array_equal(got1, plain.c1.channels())
        c.check(out, polys=[0], c0=n0, c1=n1)


def test_errors(gpu):
    """Every row of the error table, with its status and fields; a refused
    call leaves the outputs untouched."""
    b = DhCase(gpu, 8, 3, 2, 2, 2, 31, baby=[0, 1, -3], giant=[4, 0, -8], seed=12)
    rn, lib, Bd, Lv, B, n, beta = b.rn, b.rn.load(), b.basis, b.Lv, b.B, b.n, b.beta
    rng = np.random.default_rng(68)
    bm0, bm1 = _rand(rng, b.mod, n, B), _rand(rng, b.mod, n, B)
    p0, p1 = rn.RnsPoly.from_channels(bm0, Bd), rn.RnsPoly.from_channels(bm1, Bd)
    low = Bd.drop_last(1)
    rm0, rm1 = _rand(rng, b.mod[:-1], n, B), _rand(rng, b.mod[:-1], n, B)
    q0, q1 = rn.RnsPoly.from_channels(rm0, low), rn.RnsPoly.from_channels(rm1, low)
    baby, giant = (ctypes.c_int32 * 3)(*b.baby), (ctypes.c_int32 * 3)(*b.giant)
    h = lambda x: None if x is None else x.handle  # noqa: E731

    def lin(out0=p0, out1=p1, c0=b.ct.c0, c1=b.ct.c1, bs=baby, nb=3, gs=giant, ng=3, d=b.d, ka=b.bset.a, kb=b.bset.b,
            ga=b.gset.a, gb=b.gset.b, alpha=b.alpha):
        return lib.rnt_ct_linear_bsgs_hybrid_dh(h(out0), h(out1), h(c0), h(c1), bs, nb, gs, ng, h(d), h(ka), h(kb),
                                                h(ga), h(gb), alpha)

    def res(out0=q0, out1=q1, c0=b.ct.c0, c1=b.ct.c1, bs=baby, nb=3, gs=giant, ng=3, d=b.d, ka=b.bset.a, kb=b.bset.b,
            ga=b.gset.a, gb=b.gset.b, alpha=b.alpha):
        return lib.rnt_ct_linear_bsgs_hybrid_dh_rescale(h(out0), h(out1), h(c0), h(c1), bs, nb, gs, ng, h(d), h(ka),
                                                        h(kb), h(ga), h(gb), alpha)

    def fails(kind, fn, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(fn(**kw))
        assert e.value.kind == kind, (kind, fn.__name__, kw.keys(), str(e.value))
        if fields is not None:
            assert e.value.fields == fields, e.value.fields
        assert np.array_equal(p0.channels(), bm0) and np.array_equal(p1.channels(), bm1), kw.keys()
        assert np.array_equal(q0.channels(), rm0) and np.array_equal(q1.channels(), rm1), kw.keys()

    def poly(count, basis=b.ext, ntt=True):
        L = basis.channel_count()
        return rn.RnsPoly.from_channels(np.zeros((count, L, basis.degree), np.uint64), basis, in_ntt_domain=ntt)

    zero = {"degree": 0, "max_degree": 0}
    for fn in (lin, res):
        fails("BadArgument", fn, alpha=0)
        fails("BadArgument", fn, nb=0)
        fails("BadArgument", fn, ng=0)
        fails("BadArgument", fn, bs=None)
        fails("BadArgument", fn, gs=None)
        fails("BadArgument", fn, ka=None)  # a rotating stage without its keys
        fails("BadArgument", fn, gb=None)
        # the plaintexts: E's moduli at this level by value, one poly per pair, NTT domain
        fails("BasisMismatch", fn, d=poly(9, Bd))  # the ciphertext's own basis: no special limb
        fails("BasisMismatch", fn, d=poly(9, b.ext.drop_last(1)))  # one special prime short
        fails("BasisMismatch", fn, d=poly(9, rn.RnsBasis(b.emod[1:] + b.emod[:1], n)))  # another order
        fails("BasisMismatch", fn, d=poly(9, rn.RnsBasis(b.emod[:Lv] + rn.generate_primes(30, b.K, n), n)))
        fails("BasisMismatch", fn, d=poly(9, rn.RnsBasis(rn.generate_primes(31, Lv + b.K, n // 2), n // 2)))
        fails("ChannelCountMismatch", fn, {"expected": 9, "actual": 8}, d=poly(8))
        fails("ChannelCountMismatch", fn, {"expected": 9, "actual": 10}, d=poly(10))
        fails("DomainMismatch", fn, d=poly(9, ntt=False))
        # the keys, as rnt_ct_linear_bsgs_hybrid
        other = rn.RnsBasis(b.emod[1:] + b.emod[:1], n)
        fails("BasisMismatch", fn, ka=poly(3 * beta, other), kb=poly(3 * beta, other))
        fails("BasisMismatch", fn, ga=poly(3 * beta, Bd), gb=poly(3 * beta, Bd))
        twin = rn.RnsBasis(b.emod, n)  # the same moduli, another key basis: one E for both stages
        fails("BasisMismatch", fn, ga=poly(3 * beta, twin), gb=poly(3 * beta, twin))
        wide = rn.RnsBasis(b.mod + rn.generate_primes(61, 1, n), n)
        fails("Unsupported", fn, zero, ka=poly(3 * beta, wide), kb=poly(3 * beta, wide))
        fails("ChannelCountMismatch", fn, {"expected": 3 * beta, "actual": 3 * beta + 1}, kb=poly(3 * beta + 1))
        fails("ChannelCountMismatch", fn, {"expected": 3 * beta, "actual": beta}, ga=poly(beta))
        fails("ChannelCountMismatch", fn, {"expected": 3 * Lv, "actual": 3 * beta}, alpha=1)
        fails("DomainMismatch", fn, ka=poly(3 * beta, ntt=False))
        fails("DomainMismatch", fn, gb=poly(3 * beta, ntt=False))
        ntt = b.ct.c1.clone()
        ntt.to_ntt_domain()
        fails("DomainMismatch", fn, c0=ntt)
        fails("DomainMismatch", fn, c1=ntt)
        fails("BasisMismatch", fn, c1=rn.RnsPoly.from_channels(b.c1, rn.RnsBasis(b.mod, n)))
    # the outputs of the plain form
    fails("BadArgument", lin, out1=p0)  # out0 aliases out1
    fails("BadArgument", lin, out0=rn.RnsPoly(Bd, B + 1))
    fails("BadArgument", lin, out0=b.ct.c1, out1=rn.RnsPoly(Bd, B))  # an input other than its own component
    fails("BasisMismatch", lin, out0=q0, out1=q1)
    # another handle on an output's storage is that output all the same
    fails("BadArgument", lin, c1=rn.RnsPoly.wrap(Bd, p0.device_ptr()[0], B, owner=p0))
    fails("BadArgument", lin, c0=rn.RnsPoly.wrap(Bd, p1.device_ptr()[0], B, owner=p1))
    # ... and of the rescaling one
    fails("BadArgument", res, out1=q0)
    fails("BasisMismatch", res, out0=p0, out1=p1)  # not drop_last(1) of the inputs'
    fails("BasisMismatch", res, out1=rn.RnsPoly(Bd.drop_last(1), B))  # two basis objects
    fails("BadArgument", res, out0=rn.RnsPoly(low, B + 1), out1=rn.RnsPoly(low, B + 1))
    # a key level view in a ciphertext or plaintext position
    full = DhCase(rn, 8, 4, 2, 2, 2, 31, baby=[0, 1, -3], giant=[4, 0, -8], seed=13, n_special=2)
    view = full.bset.at_level(3)
    for pos in ("out0", "out1", "c0", "c1", "d"):
        fails("Unsupported", lin, zero, **{pos: view.a})
    # plaintexts on another context over the same moduli are E's by value: a valid call, the call's words
    want = b.run()
    dt = rn.RnsPoly.from_channels(b.diagE, rn.RnsBasis(b.emod, n))
    dt.to_ntt_domain()
    w0, w1 = rn.RnsPoly(Bd, B), rn.RnsPoly(Bd, B)
    rn.check(lin(out0=w0, out1=w1, d=dt))
    assert np.array_equal(w0.channels(), want.c0.channels()) and np.array_equal(w1.channels(), want.c1.channels())
    # the valid calls still run after all that
    rn.check(lin())
    assert np.array_equal(p0.channels(), want.c0.channels()) and np.array_equal(p1.channels(), want.c1.channels())
    rn.check(res())
    r = rn.rescale_ciphertext(want)
    assert np.array_equal(q0.channels(), r.c0.channels()) and np.array_equal(q1.channels(), r.c1.channels())


def test_python_layer_guards_the_key_class_and_form(gpu):
    c = DhCase(gpu, 8, 3, 2, 2, 2, 31, baby=[0, 1, -3], giant=[0, 2], seed=14)
    rn = c.rn
    plain_baby = rn.RnsHybridKeySet(_upload(rn, c.ext, c.alpha, c.baby, c.bkeys, False), c.alpha)
    hoisted_giant = rn.RnsHybridKeySet(_upload(rn, c.ext, c.alpha, c.giant, c.gkeys, True), c.alpha)
    rng = np.random.default_rng(69)
    gk = rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.Lv), _rand(rng, c.mod, c.n, c.Lv), c.basis, rotation=1)
    gset = rn.RnsGadgetKeySet([None, gk, None], c.basis)
    for call in (lambda: rn.linear_bsgs_hybrid_dh(c.ct, c.d, plain_baby, c.gset),     # ordinary baby keys
                 lambda: rn.linear_bsgs_hybrid_dh(c.ct, c.d, c.bset, hoisted_giant),  # hoisting-form giants
                 lambda: rn.linear_bsgs_hybrid_dh(c.ct, c.d, gset, c.gset),           # a gadget key set
                 lambda: rn.linear_bsgs_hybrid_dh(c.ct, c.d, c.bset, rn.RnsHybridKeySet([None, None], c.alpha + 1))):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
# tools/dh_bsgs_tolerance.py (profiles/dh_bsgs_tolerance.txt), eight seeds, the
# same ring and parameters on the CPU (oracle/pyoracle, oracle/encoder.py,
# tests/dh_bsgs_ref.py): the largest decode errors.  The tolerances are 4 x
# these, the project's margin for another noise draw (the device's sampler),
# the arithmetic being identical.  rnt_ct_linear_bsgs_hybrid's figures on the
# same draws: 9.210e-5 for the band, 7.477e-5 for the round trip.
BAND_ERR_MEASURED = 1.003e-4
BACK_ERR_MEASURED = 5.652e-5


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


def test_engine_band_end_to_end(gpu):
    """A 16-diagonal band at diagonal scale 2^30 through
    linear_transform_bsgs_hybrid_dh (4 x 4) -> rescale -> decrypt -> decode
    against M x, and through the _dh_rescale form."""
    rn = gpu
    CkksEngine, eng, q = _engine(rn)
    n, slots, alpha, logp = 1024, 512, 2, 30
    rng = rn.DeviceRng(96)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    host = np.random.default_rng(97)
    x = host.uniform(-1, 1, slots)
    M = np.zeros((slots, slots))
    s = np.arange(slots)
    diags = {}
    for d in range(16):
        diags[d] = host.uniform(-1, 1, slots)
        M[s, (s + d) % slots] = diags[d]
    enc = rn.CkksEncoder(n, logp)
    ct = eng.encrypt(enc.encode(x, eng.basis), pk, rng)
    baby, giant = [0, 1, 2, 3], [0, 4, 8, 12]
    bset = eng.generate_hybrid_rotation_key_set(sk, baby, rng, alpha, hoisted=True)
    gset = eng.generate_hybrid_rotation_key_set(sk, giant, rng, alpha)
    assert eng.dh_plain_basis() is eng.ext_basis
    pt = CkksEngine.encode_diagonal_rows_bsgs(diags, baby, giant, enc, eng.dh_plain_basis())
    assert pt.poly.basis is eng.ext_basis and pt.poly.is_ntt_domain()
    out = CkksEngine.linear_transform_bsgs_hybrid_dh(ct, pt, bset, gset)
    assert out.logp == 2 * logp and out.logq == ct.logq
    fused = CkksEngine.linear_transform_bsgs_hybrid_dh_rescale(ct, pt, bset, gset)
    res = CkksEngine.rescale_ciphertext(out)
    assert fused.logp == res.logp and fused.logq == res.logq
    assert np.array_equal(fused.c0.channels(), res.c0.channels()) and np.array_equal(fused.c1.channels(), res.c1.channels())
    got = enc.decode(CkksEngine.decrypt_plaintext(res, CkksEngine.secret_on(sk, res.c0.basis)))
    # logp counts the dropped prime as 31 bits; the true scale is 2^60 / q_last
    y = (M @ x) * (2.0 ** (2 * logp - res.logp) / q[-1])
    err = float(np.max(np.abs(got - y)))
    print(f"double-hoisted band 4 x 4: decode error {err:.3e}, max|y| {np.max(np.abs(y)):.3f}")
    assert err <= 4 * BAND_ERR_MEASURED


def test_engine_coeff_to_slot_then_slot_to_coeff_end_to_end(gpu):
    """CoeffToSlot (one group, 32 x 16) then SlotToCoeff (one group) through
    the _dh path on a fresh 4-limb ciphertext: two levels down -- the second
    group on a level basis of its own and through the key level views -- and
    the slots come back."""
    rn = gpu
    CkksEngine, eng, q = _engine(rn)
    n, slots, alpha, logp = 1024, 512, 2, 30
    rng = rn.DeviceRng(98)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    host = np.random.default_rng(99)
    x = host.uniform(-1, 1, slots) + 1j * host.uniform(-1, 1, slots)
    enc = rn.CkksEncoder(n, logp)
    ct = eng.encrypt(enc.encode_complex(x, eng.basis), pk, rng)
    c2s, s2c = rn.homdft_plan(n, "coeff_to_slot", 1), rn.homdft_plan(n, "slot_to_coeff", 1)
    p1 = eng.prepare_homdft_dh(c2s, eng.basis)
    p2 = eng.prepare_homdft_dh(s2c, p1.bases[-1])
    assert p1.plaintexts[0].poly.basis is eng.ext_basis
    assert p2.plaintexts[0].poly.basis is eng.dh_plain_basis(3)
    assert p2.plaintexts[0].poly.basis.moduli() == rn.hybrid_level_moduli(eng.ext_basis, 2, 3)
    k1 = eng.generate_homdft_key_sets(sk, c2s, rng, alpha)
    k2 = eng.generate_homdft_key_sets(sk, s2c, rng, alpha)
    mid = CkksEngine.coeff_to_slot_hybrid_dh(ct, p1, k1)
    back = CkksEngine.slot_to_coeff_hybrid_dh(mid, p2, k2)
    assert back.c0.basis is p2.bases[-1] and back.c0.basis.channel_count() == 2 and back.logp == ct.logp
    got = enc.decode_complex(CkksEngine.decrypt_plaintext(back, CkksEngine.secret_on(sk, back.c0.basis)))
    err = float(np.max(np.abs(np.asarray(got).reshape(-1) - x)))
    print(f"CoeffToSlot then SlotToCoeff, double-hoisted: decode error {err:.3e}")
    assert err <= 4 * BACK_ERR_MEASURED
