"""The hybrid calls that close a level on the GPU
(rnt_ct_mul_relin_rescale_hybrid, rnt_ct_linear_bsgs_hybrid_rescale): DEFINED
as the un-rescaled hybrid call followed by rnt_ct_rescale, word for word.  The
multiply seeds its key products with the tensor's d0^, d1^ in the NTT domain
(k_hoist_mac_seed: ModDown(A + P d) = ModDown(A) + d) and both calls end in
k_moddown_rescale, so the level-Lv result never reaches memory.  Every case is
compared with the device composition on every poly and with the CPU yardstick
(tests/hybrid_rescale_ref.py, pinned in tests/test_hybrid_rescale_ref.py).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from hybrid_ref import restrict_key
from hybrid_rescale_ref import bsgs_hybrid_rescale_ref, mul_relin_rescale_hybrid_ref
from test_gpu_hybrid import MUL_ERR_MEASURED, Case, _rand
from test_gpu_hybrid_hoist import BsgsCase

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(a.c0.channels(), b.c0.channels()) and np.array_equal(a.c1.channels(), b.c1.channels())


def _composition(rn, c):
    return rn.rescale_ciphertext(rn.mul_ciphertexts_hybrid(c.ct, c.ctp, c.key))


def check_mul(c, key=None, ka=None, kb=None, Be=None):
    """The fused multiply against the device composition on every poly and
    against the yardstick on polys {0, B - 1}."""
    rn = c.rn
    key = key or c.key
    ka, kb, Be = (c.ka if ka is None else ka), (c.kb if kb is None else kb), Be or c.Be
    fused = rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, key)
    comp = rn.rescale_ciphertext(rn.mul_ciphertexts_hybrid(c.ct, c.ctp, key))
    for o in (fused.c0, fused.c1):
        assert not o.is_ntt_domain() and o.n_polys == c.B and o.basis.channel_count() == c.Lv - 1
    assert fused.c0.basis is fused.c1.basis
    assert fused.logp == comp.logp and fused.logq == comp.logq
    assert np.array_equal(fused.c0.channels(), comp.c0.channels()), "out0 differs from the composition"
    assert np.array_equal(fused.c1.channels(), comp.c1.channels()), "out1 differs from the composition"
    for p in sorted({0, c.B - 1}):
        r0, r1 = mul_relin_rescale_hybrid_ref(c.Bc, Be, c.c0[p], c.c1[p], c.c0p[p], c.c1p[p], ka, kb, c.alpha)
        assert np.array_equal(fused.c0.channels_of(p)[0], r0), f"out0 of poly {p} differs from the yardstick"
        assert np.array_equal(fused.c1.channels_of(p)[0], r1), f"out1 of poly {p} differs from the yardstick"
    return fused


def check_bsgs_rescale(c, polys=(0,)):
    """The fused transform of a BsgsCase against the device composition on
    every poly and against the yardstick on ``polys``."""
    rn = c.rn
    fused = rn.linear_transform_bsgs_hybrid_rescale(c.ct, c.d, c.bset, c.gset)
    comp = rn.rescale_ciphertext(c.run())
    for o in (fused.c0, fused.c1):
        assert not o.is_ntt_domain() and o.n_polys == c.B and o.basis.channel_count() == c.Lv - 1
    assert fused.c0.basis is fused.c1.basis and fused.logq == comp.logq
    assert np.array_equal(fused.c0.channels(), comp.c0.channels()), "out0 differs from the composition"
    assert np.array_equal(fused.c1.channels(), comp.c1.channels()), "out1 differs from the composition"
    for p in polys:
        r0, r1 = bsgs_hybrid_rescale_ref(c.Bc, c.Be, c.c0[p], c.c1[p], c.baby, c.giant, c.diag, c.bkeys, c.gkeys,
                                         c.alpha)
        assert np.array_equal(fused.c0.channels_of(p)[0], r0), f"out0 of poly {p} differs from the yardstick"
        assert np.array_equal(fused.c1.channels_of(p)[0], r1), f"out1 of poly {p} differs from the yardstick"
    return fused


# log_n, Lv, K, alpha, B, bits, ws_mb, edge
SHAPES = [
    (8, 3, 2, 2, 3, 31, None, False),    # small four-step grid, partial last digit
    (8, 3, 2, 2, 3, 31, None, True),     # the same with all-(q-1) ciphertexts and an all-(m-1) key
    (8, 2, 1, 1, 2, 31, None, False),    # a single output limb
    (8, 3, 3, 3, 2, 31, None, False),    # a single digit
    (12, 3, 2, 2, 2, 31, None, False),   # whole-plane tensor
    (12, 3, 2, 2, 2, 61, None, False),   # u64
    (14, 3, 2, 2, 3, 31, "1", False),    # several chunks
    (14, 2, 1, 2, 2, 61, None, False),   # u64 four-step
    (16, 4, 2, 2, 2, 31, None, False),   # matrix-core tensor and transforms
    (17, 4, 2, 2, 1, 31, None, False),   # largest ring
    (14, 3, 2, 2, 64, 31, None, False),  # un-split grids
]
PLACED = [s + (place,) for s in SHAPES for place in (("view", "root") if s[0] in (8, 14) else ("view",))]


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb,edge,place", PLACED)
def test_mul_rescale_parity(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb, edge, place):
    """place="root": the ciphertexts on a root context unrelated to the key's,
    so the NTT-domain seeds of one context's transforms enter accumulators the
    other context's transforms invert."""
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    check_mul(Case(gpu, log_n, Lv, K, alpha, B, bits, edge=edge, place=place, seed=B))


@pytest.mark.parametrize("log_n", [12, 16])
def test_mul_rescale_when_the_contexts_transform_differently(gpu, monkeypatch, log_n):
    """A key basis created with RNT_PLANE=0 (four-step kernels everywhere) under
    ciphertexts on a default context: the seeds take the un-fused way inside the
    call and the words are still the composition's."""
    monkeypatch.setenv("RNT_PLANE", "0")  # read at rnt_ctx_create
    c = Case(gpu, log_n, 3, 2, 2, 2, 31, place="root", seed=9)
    monkeypatch.delenv("RNT_PLANE")
    rn = gpu
    c.basis = rn.RnsBasis(c.mod, c.n)
    up = lambda x: rn.RnsPoly.from_channels(x, c.basis)  # noqa: E731
    c.ct, c.ctp = rn.Ciphertext(up(c.c0), up(c.c1)), rn.Ciphertext(up(c.c0p), up(c.c1p))
    check_mul(c)


@pytest.mark.parametrize("log_n", [8, 12, 14])
def test_levelled(gpu, log_n):
    """A 4-limb chain with alpha = 2: a fused multiply at the top level, then
    its OUTPUT (3 limbs, on drop_last(1) of the top context) into a second
    fused multiply with the key restricted to a fresh root over q_0..q_2, p_0,
    p_1.  Both equal the composition and the yardstick."""
    rn = gpu
    top = Case(rn, log_n, 4, 2, 2, 2, 31, seed=2)
    f1 = check_mul(top)
    n, q, p = top.n, top.mod, top.emod[4:]
    low = Case.__new__(Case)
    low.rn, low.n, low.Lv, low.K, low.alpha, low.B = rn, n, 3, 2, 2, 2
    low.mod, low.emod = q[:3], q[:3] + p
    low.c0, low.c1 = f1.c0.channels(), f1.c1.channels()
    low.c0p = np.ascontiguousarray(top.c0p[:, :3, :])
    low.c1p = np.ascontiguousarray(top.c1p[:, :3, :])
    low.ext = rn.RnsBasis(low.emod, n)
    low.key = top.key.restrict(low.ext)
    low.ka, low.kb = restrict_key(top.ka, 4, 2, 3), restrict_key(top.kb, 4, 2, 3)
    low.Bc, low.Be = orc.Basis(low.mod, n), orc.Basis(low.emod, n)
    low.basis = f1.c0.basis
    assert low.basis.channel_count() == 3
    low.ct = f1
    low.ctp = rn.Ciphertext(rn.RnsPoly.from_channels(low.c0p, low.basis), rn.RnsPoly.from_channels(low.c1p, low.basis),
                            logq=f1.logq)
    f2 = check_mul(low)
    assert f2.c0.basis.channel_count() == 2


# baby steps with a zero, a negative and a positive step
BABY = [0, 1, -3]


@pytest.mark.parametrize("giant", [[0, 2], [4, -8], [0]], ids=["zero-and-step", "two-steps", "no-moddown"])
@pytest.mark.parametrize("log_n", [8, 12, 14])
def test_bsgs_rescale_parity(gpu, log_n, giant):
    """[0, g]: the addend Z1 present; [g1, g2]: no step-0 giant (Z1 absent, S0
    from the first automorphism); [0]: no ModDown tail, k_rescale on the sums
    (linear_transform_hybrid's case)."""
    c = BsgsCase(gpu, log_n, 3, 2, 2, 2, 31, baby=BABY, giant=giant, seed=len(giant) + giant[0])
    check_bsgs_rescale(c, polys=(0,) if log_n == 8 else ())


def test_bsgs_rescale_chunked(gpu, monkeypatch):
    """Several chunks: the tails write a chunk's polys at the outputs' own limb
    stride, the k_rescale one included."""
    monkeypatch.setenv("RNT_KS_WS_MB", "1")
    for giant in ([0, 2], [0]):
        c = BsgsCase(gpu, 12, 3, 2, 2, 5, 31, baby=[0, 1], giant=giant, seed=11)
        assert _same(gpu.linear_transform_bsgs_hybrid_rescale(c.ct, c.d, c.bset, c.gset),
                     gpu.rescale_ciphertext(c.run())), giant


def test_unaligned_planes(gpu):
    """The scalar instantiations of both new kernels: inputs, outputs and keys
    wrapped at an offset of one word, so none of their planes is 16-byte
    aligned.  The unaligned outputs select k_moddown_rescale's one-word form,
    the unaligned keys k_hoist_mac_seed's (its seeds and accumulators are in
    the call's own aligned workspace)."""
    import torch

    c = Case(gpu, 8, 3, 2, 2, 3, 31, seed=3)
    rn, lib, Bd = c.rn, c.rn.load(), c.basis
    dev = torch.device("cuda", Bd.device)

    def shifted(basis, n_polys, src=None, ntt=False, n=c.n):
        words = n_polys * basis.channel_count() * n
        t = torch.zeros(words + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(basis, t.data_ptr() + 4, n_polys, in_ntt_domain=ntt, owner=t)
        assert v.device_ptr()[0] % 16 == 4
        if src is not None:
            v.copy_polys(src)
        return v

    want = _composition(rn, c)
    low = want.c0.basis
    g0, g1 = shifted(low, c.B), shifted(low, c.B)
    ins = [shifted(Bd, c.B, x) for x in (c.ct.c0, c.ct.c1, c.ctp.c0, c.ctp.c1)]
    ka, kb = shifted(c.ext, c.beta, c.key.a, ntt=True), shifted(c.ext, c.beta, c.key.b, ntt=True)
    rn.check(lib.rnt_ct_mul_relin_rescale_hybrid(g0.handle, g1.handle, *[x.handle for x in ins], ka.handle, kb.handle,
                                                 c.alpha))
    assert np.array_equal(g0.channels(), want.c0.channels()) and np.array_equal(g1.channels(), want.c1.channels())
    r0, r1 = mul_relin_rescale_hybrid_ref(c.Bc, c.Be, c.c0[1], c.c1[1], c.c0p[1], c.c1p[1], c.ka, c.kb, c.alpha)
    assert np.array_equal(g0.channels_of(1)[0], r0) and np.array_equal(g1.channels_of(1)[0], r1)
    b = BsgsCase(gpu, 8, 3, 2, 2, 3, 31, seed=3)
    wantb = rn.rescale_ciphertext(b.run())
    lowb = wantb.c0.basis
    o0, o1 = shifted(lowb, b.B), shifted(lowb, b.B)
    t0, t1 = shifted(b.basis, b.B, b.ct.c0), shifted(b.basis, b.B, b.ct.c1)
    d = shifted(b.basis, b.d.n_polys, b.d, ntt=True)
    sets = [shifted(b.ext, x.n_polys, x, ntt=True) for x in (b.bset.a, b.bset.b, b.gset.a, b.gset.b)]
    baby, giant = (ctypes.c_int32 * len(b.baby))(*b.baby), (ctypes.c_int32 * len(b.giant))(*b.giant)
    rn.check(lib.rnt_ct_linear_bsgs_hybrid_rescale(o0.handle, o1.handle, t0.handle, t1.handle, baby, len(b.baby),
                                                   giant, len(b.giant), d.handle, *[x.handle for x in sets], b.alpha))
    assert np.array_equal(o0.channels(), wantb.c0.channels()) and np.array_equal(o1.channels(), wantb.c1.channels())


INVERSES = ("whole_inv", "row_inv", "col_inv", "mf_ntt_inv")
NAMES = ("moddown_rescale", "moddown", "rescale", "elementwise", "modup", "hoist_mac") + INVERSES


def _counts(basis, run):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in NAMES}
    basis.profile_enable(False)
    print(counts)
    return counts


def test_launch_counts(gpu):
    """One chunk at 2^14: the fused calls end in two k_moddown_rescale launches
    and no k_moddown or k_rescale; the fused multiply has lost the composition's
    two unscale passes and its two seed inverses."""
    rn = gpu
    c = Case(rn, 14, 3, 2, 2, 2, 31, seed=4)
    fused = _counts(c.basis, lambda: rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key))
    comp = _counts(c.basis, lambda: _composition(rn, c))
    assert (fused["moddown_rescale"], fused["moddown"], fused["rescale"]) == (2, 0, 0)
    assert (comp["moddown_rescale"], comp["moddown"], comp["rescale"]) == (0, 2, 2)
    assert fused["modup"] == 1 and fused["hoist_mac"] == 1
    assert fused["elementwise"] == comp["elementwise"] - 2
    inv_f, inv_c = sum(fused[k] for k in INVERSES), sum(comp[k] for k in INVERSES)
    assert inv_f < inv_c, (inv_f, inv_c)
    b = BsgsCase(rn, 14, 3, 2, 2, 2, 31, seed=4)
    assert sum(g != 0 for g in b.giant) == 2
    fb = _counts(b.basis, lambda: rn.linear_transform_bsgs_hybrid_rescale(b.ct, b.d, b.bset, b.gset))
    assert (fb["moddown_rescale"], fb["moddown"], fb["rescale"]) == (2, 0, 0)
    z = BsgsCase(rn, 14, 3, 2, 2, 2, 31, baby=BABY, giant=[0], seed=4)  # no ModDown tail: no fusion claimed
    fz = _counts(z.basis, lambda: rn.linear_transform_bsgs_hybrid_rescale(z.ct, z.d, z.bset, z.gset))
    assert (fz["moddown_rescale"], fz["moddown"], fz["rescale"]) == (0, 0, 2)


@pytest.mark.parametrize("log_n", [12, 14])
def test_captured(gpu, log_n):
    """Both calls record into a graph after one plain run; two replays on
    refreshed inputs give the words of the plain calls."""
    c = Case(gpu, log_n, 3, 2, 2, 2, 31, seed=5)
    b = BsgsCase(gpu, log_n, 3, 2, 2, 2, 31, seed=5)
    rn, lib = c.rn, c.rn.load()
    low, lowb = c.basis.drop_last(1), b.basis.drop_last(1)
    outs = [rn.RnsPoly(low, c.B) for _ in range(2)]
    bouts = [rn.RnsPoly(lowb, b.B) for _ in range(2)]
    baby, giant = (ctypes.c_int32 * len(b.baby))(*b.baby), (ctypes.c_int32 * len(b.giant))(*b.giant)

    def run_mul():
        rn.check(lib.rnt_ct_mul_relin_rescale_hybrid(outs[0].handle, outs[1].handle, c.ct.c0.handle, c.ct.c1.handle,
                                                     c.ctp.c0.handle, c.ctp.c1.handle, c.key.a.handle,
                                                     c.key.b.handle, c.alpha))

    def run_bsgs():
        rn.check(lib.rnt_ct_linear_bsgs_hybrid_rescale(bouts[0].handle, bouts[1].handle, b.ct.c0.handle,
                                                       b.ct.c1.handle, baby, len(b.baby), giant, len(b.giant),
                                                       b.d.handle, b.bset.a.handle, b.bset.b.handle, b.gset.a.handle,
                                                       b.gset.b.handle, b.alpha))

    run_mul()
    run_bsgs()
    with c.basis.capture() as gm:
        run_mul()
    with b.basis.capture() as gb:
        run_bsgs()
    rng = np.random.default_rng(53 + log_n)
    for _ in range(2):
        for case in (c, b):
            n0, n1 = _rand(rng, case.mod, case.n, case.B), _rand(rng, case.mod, case.n, case.B)
            case.ct.c0.copy_polys(rn.RnsPoly.from_channels(n0, case.basis))
            case.ct.c1.copy_polys(rn.RnsPoly.from_channels(n1, case.basis))
        gm.replay()
        c.basis.sync()
        gb.replay()
        b.basis.sync()
        want = rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key)
        assert np.array_equal(outs[0].channels(), want.c0.channels())
        assert np.array_equal(outs[1].channels(), want.c1.channels())
        assert _same(want, _composition(rn, c))
        wantb = rn.linear_transform_bsgs_hybrid_rescale(b.ct, b.d, b.bset, b.gset)
        assert np.array_equal(bouts[0].channels(), wantb.c0.channels())
        assert np.array_equal(bouts[1].channels(), wantb.c1.channels())
        assert _same(wantb, rn.rescale_ciphertext(b.run()))


def test_errors(gpu):
    """Every row of the header's table, with its status and fields; a refused
    call leaves marked outputs untouched."""
    c = Case(gpu, 8, 3, 2, 2, 2, 31, seed=6)
    rn, lib, Bd, Lv, B, n = c.rn, c.rn.load(), c.basis, c.Lv, c.B, c.n
    low = Bd.drop_last(1)
    rng = np.random.default_rng(58)
    mark0, mark1 = _rand(rng, c.mod[:-1], n, B), _rand(rng, c.mod[:-1], n, B)
    o0, o1 = rn.RnsPoly.from_channels(mark0, low), rn.RnsPoly.from_channels(mark1, low)
    b = BsgsCase(gpu, 8, 3, 2, 2, 2, 31, baby=[0, 1], giant=[0, 2], seed=6)
    blow = b.basis.drop_last(1)
    p0, p1 = rn.RnsPoly.from_channels(mark0, blow), rn.RnsPoly.from_channels(mark1, blow)
    baby, giant = (ctypes.c_int32 * 2)(*b.baby), (ctypes.c_int32 * 2)(*b.giant)

    def mul(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, c0p=c.ctp.c0, c1p=c.ctp.c1, ka=c.key.a, kb=c.key.b,
            alpha=c.alpha):
        return lib.rnt_ct_mul_relin_rescale_hybrid(out0.handle, out1.handle, c0.handle, c1.handle, c0p.handle,
                                                   c1p.handle, ka.handle, kb.handle, alpha)

    def lin(out0=p0, out1=p1, c0=b.ct.c0, c1=b.ct.c1, d=b.d, bka=b.bset.a, bkb=b.bset.b, gka=b.gset.a, gkb=b.gset.b,
            alpha=b.alpha):
        return lib.rnt_ct_linear_bsgs_hybrid_rescale(out0.handle, out1.handle, c0.handle, c1.handle, baby, 2, giant, 2,
                                                     d.handle, bka.handle, bkb.handle, gka.handle, gkb.handle, alpha)

    def fails(kind, fn, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(fn(**kw))
        assert e.value.kind == kind, (kind, fn.__name__, kw.keys(), str(e.value))
        if fields is not None:
            assert e.value.fields == fields, e.value.fields
        for o, m in ((o0, mark0), (o1, mark1), (p0, mark0), (p1, mark1)):
            assert np.array_equal(o.channels(), m), kw.keys()

    def keypoly(count, basis, ntt=True):
        L = basis.channel_count()
        return rn.RnsPoly.from_channels(np.zeros((count, L, n), np.uint64), basis, in_ntt_domain=ntt)

    for fn, case, outs in ((mul, c, (o0, o1)), (lin, b, (p0, p1))):
        Bf = case.basis
        # outputs on the wrong context: the inputs' own, a basis two limbs down, an unrelated root
        for wrong in (Bf, Bf.drop_last(2), rn.RnsBasis(case.mod[:-1], n)):
            fails("BasisMismatch", fn, out0=rn.RnsPoly(wrong, B))
            fails("BasisMismatch", fn, out1=rn.RnsPoly(wrong, B))
        # the right limbs on a context of their own: the outputs do not share one
        fails("BasisMismatch", fn, out1=rn.RnsPoly(Bf.drop_last(1), B))
        fails("BadArgument", fn, out1=outs[0])  # out0 == out1
        fails("BadArgument", fn, out0=rn.RnsPoly(outs[0].basis, B + 1))  # wrong output size
        fails("BadArgument", fn, alpha=0)
        ntt = case.ct.c1.clone()
        ntt.to_ntt_domain()
        fails("DomainMismatch", fn, c1=ntt)
        fails("DomainMismatch", fn, c0=ntt)
    ntt = c.ctp.c0.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", mul, c0p=ntt)
    # a coefficient-domain key, a wrong key count
    fails("DomainMismatch", mul, ka=keypoly(c.beta, c.ext, ntt=False))
    fails("DomainMismatch", mul, kb=keypoly(c.beta, c.ext, ntt=False))
    fails("ChannelCountMismatch", mul, {"expected": c.beta, "actual": c.beta + 1}, ka=keypoly(c.beta + 1, c.ext))
    fails("ChannelCountMismatch", mul, {"expected": c.beta, "actual": 1}, kb=keypoly(1, c.ext))
    fails("ChannelCountMismatch", mul, {"expected": Lv, "actual": c.beta}, alpha=1)
    fails("DomainMismatch", lin, gka=keypoly(b.gset.a.n_polys, b.ext, ntt=False))
    fails("ChannelCountMismatch", lin, {"expected": 2 * b.beta, "actual": 2 * b.beta + 1},
          bka=keypoly(2 * b.beta + 1, b.ext))
    # a key basis without a special limb; inputs on two contexts
    fails("BasisMismatch", mul, ka=keypoly(c.beta, Bd), kb=keypoly(c.beta, Bd))
    fails("BasisMismatch", mul, c1=rn.RnsPoly(rn.RnsBasis(c.mod, n), B))
    fails("BadArgument", mul, c1=rn.RnsPoly(Bd, B + 1))  # inputs of different batch sizes
    # the same primes in another order; a 61-bit special prime makes E a u64 basis
    other = rn.RnsBasis(c.emod[1:] + c.emod[:1], n)
    fails("BasisMismatch", mul, ka=keypoly(c.beta, other), kb=keypoly(c.beta, other))
    wide = rn.RnsBasis(c.mod + rn.generate_primes(61, 1, n), n)
    fails("Unsupported", mul, {"degree": 0, "max_degree": 0}, ka=keypoly(c.beta, wide), kb=keypoly(c.beta, wide))
    # a one-limb ciphertext: nothing to drop
    one = Case(gpu, 8, 1, 1, 1, B, 31, seed=6)
    fails("InvalidModDrop", mul, {"drop_count": 1, "channel_count": 1}, c0=one.ct.c0, c1=one.ct.c1, c0p=one.ctp.c0,
          c1p=one.ctp.c1, ka=one.key.a, kb=one.key.b, alpha=1)
    # two faults at once: the multiply compares the inputs with c0, then checks
    # alpha and the key, then the inputs' domain, and the outputs last
    ntt = c.ct.c0.clone()
    ntt.to_ntt_domain()
    apart = rn.RnsPoly(rn.RnsBasis(c.mod, n), B)  # the right limbs on a root of their own
    fails("BasisMismatch", mul, c1p=apart, alpha=0)
    fails("BadArgument", mul, c0p=rn.RnsPoly(Bd, B + 1), ka=keypoly(c.beta + 1, c.ext))
    fails("BadArgument", mul, out0=rn.RnsPoly(Bd, B), alpha=0)
    fails("DomainMismatch", mul, out0=rn.RnsPoly(Bd, B), c0=ntt)
    fails("DomainMismatch", mul, out1=rn.RnsPoly(low, B + 1), kb=keypoly(c.beta, c.ext, ntt=False))
    fails("ChannelCountMismatch", mul, {"expected": c.beta, "actual": c.beta + 1}, c0=ntt,
          ka=keypoly(c.beta + 1, c.ext))
    fails("ChannelCountMismatch", mul, {"expected": c.beta, "actual": 1}, out0=rn.RnsPoly(low, B + 1),
          kb=keypoly(1, c.ext))
    fails("BasisMismatch", mul, out0=rn.RnsPoly(Bd, B + 1))  # an output's basis before its size
    one_ntt = one.ct.c1.clone()
    one_ntt.to_ntt_domain()
    fails("DomainMismatch", mul, c0=one.ct.c0, c1=one_ntt, c0p=one.ctp.c0, c1p=one.ctp.c1, ka=one.key.a,
          kb=one.key.b, alpha=1)  # a one-limb ciphertext in the NTT domain
    one_b = BsgsCase(gpu, 8, 1, 1, 1, B, 31, baby=[0, 1], giant=[0, 2], seed=6)
    fails("InvalidModDrop", lin, {"drop_count": 1, "channel_count": 1}, c0=one_b.ct.c0, c1=one_b.ct.c1, d=one_b.d,
          bka=one_b.bset.a, bkb=one_b.bset.b, gka=one_b.gset.a, gkb=one_b.gset.b, alpha=1)
    # the valid calls still run after all that
    rn.check(mul())
    want = _composition(rn, c)
    assert np.array_equal(o0.channels(), want.c0.channels()) and np.array_equal(o1.channels(), want.c1.channels())
    rn.check(lin())
    wantb = rn.rescale_ciphertext(b.run())
    assert np.array_equal(p0.channels(), wantb.c0.channels()) and np.array_equal(p1.channels(), wantb.c1.channels())


def test_python_layer_guards(gpu):
    """The wrappers refuse a gadget key and key sets of the wrong form before
    they reach the library, as the un-rescaled wrappers do."""
    c = Case(gpu, 8, 3, 2, 2, 2, 31, seed=7)
    rn = c.rn
    rng = np.random.default_rng(59)
    gk = rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.Lv), _rand(rng, c.mod, c.n, c.Lv), c.basis, rotation=1)
    with pytest.raises(TypeError):
        rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, gk)
    b = BsgsCase(gpu, 8, 3, 2, 2, 2, 31, baby=[0, 1], giant=[0, 2], seed=7)
    with pytest.raises(ValueError):
        rn.linear_transform_bsgs_hybrid_rescale(b.ct, b.d, b.gset, b.gset)  # ordinary keys as baby keys
    with pytest.raises(ValueError):
        rn.linear_transform_bsgs_hybrid_rescale(b.ct, b.d, b.bset, b.bset)  # hoisting-form keys as giant keys


def test_engine_hybrid_multiply_rescale_end_to_end(gpu):
    """tools/hybrid_tolerance.py's parameters (N = 2^10, the four smallest
    31-bit primes + 2 special primes, alpha = 2, scale 2^30): encrypt ->
    mul_ciphertexts_hybrid_rescale -> decrypt -> decode.  The ciphertext words
    are the two-call composition's, so the decode error has its tolerance
    (4 x the tool's measurement, 1.14e-4)."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L, K, alpha, logp = 1024, 512, 4, 2, 2, 30
    q, cand = [], (1 << 30) + 1
    while len(q) < L:
        if rn.is_ntt_friendly_prime(cand, n):
            q.append(cand)
        cand += 2 * n
    eng = CkksEngine(q, n, error_std=3.2, hamming_weight=n // 2, special_moduli=rn.generate_primes(31, K, n))
    rng = rn.DeviceRng(81)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    host = np.random.default_rng(82)
    x, y = host.uniform(-1, 1, slots), host.uniform(-1, 1, slots)
    enc = rn.CkksEncoder(n, logp)
    ctx, cty = eng.encrypt(enc.encode(x, eng.basis), pk, rng), eng.encrypt(enc.encode(y, eng.basis), pk, rng)
    rlk = eng.generate_hybrid_relin_key(sk, rng, alpha)
    prod = CkksEngine.mul_ciphertexts_hybrid_rescale(ctx, cty, rlk)
    comp = CkksEngine.rescale_ciphertext(CkksEngine.mul_ciphertexts_hybrid(ctx, cty, rlk))
    assert prod.logp == comp.logp == 2 * logp - 31 and prod.logq == comp.logq
    assert prod.c0.basis.channel_count() == L - 1
    assert _same(prod, comp)
    got = enc.decode(CkksEngine.decrypt_plaintext(prod, CkksEngine.secret_on(sk, prod.c0.basis)))
    # logp counts the dropped prime as 31 bits; the true scale is 2^60 / q_last
    err = float(np.max(np.abs(got - x * y * (2.0 ** (2 * logp - prod.logp) / q[-1]))))
    print(f"fused hybrid multiply + rescale: decode error {err:.3e}")
    assert err <= 4 * MUL_ERR_MEASURED


def test_engine_bsgs_rescale_bookkeeping(gpu):
    """CkksEngine.linear_transform_bsgs_hybrid_rescale: the composition's words,
    logp grown by the diagonals' scale and dropped, with logq, by the limb."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    b = BsgsCase(rn, 8, 3, 2, 2, 2, 31, baby=[0, 1], giant=[0, 2], seed=12)
    b.ct.logp, b.ct.logq = 30, 93
    pt = rn.Plaintext(b.d, 30, b.n // 2)
    fused = CkksEngine.linear_transform_bsgs_hybrid_rescale(b.ct, pt, b.bset, b.gset)
    comp = CkksEngine.rescale_ciphertext(CkksEngine.linear_transform_bsgs_hybrid(b.ct, pt, b.bset, b.gset))
    assert (fused.logp, fused.logq) == (comp.logp, comp.logq) == (60 - b.mod[-1].bit_length(), 93 - b.mod[-1].bit_length())
    assert _same(fused, comp)
