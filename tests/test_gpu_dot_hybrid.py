"""The hybrid ciphertext inner product on the GPU (rnt_ct_dot_relin_hybrid,
rnt_ct_dot_relin_rescale_hybrid): the tensor components of n_terms products
are summed in the NTT domain (k_dot_tensor, groups of kDotT terms) and ONE
key-switch runs on the summed d2.  Exact arithmetic with canonical outputs, so
both calls must give, on every poly, the words of the device composition of
existing ops (RnsPoly products and sums -> keyswitch_hybrid -> add ->
rescale_ciphertext) and, on polys {0, B - 1}, those of the CPU yardstick
(tests/dot_hybrid_ref.py, pinned in tests/test_dot_hybrid_ref.py).

END-TO-END TOLERANCE: tools/dot_tolerance.py, eight seeds of the CPU yardstick
on the evaluator tests' ring (N = 2^10, 7 ciphertext primes of 30 bits, 2
special primes of 31 bits, alpha = 2, scale 2^30, 8 terms, inputs uniform in
(-1, 1)), largest decode error at the nominal scale against numpy's
sum_i a_i b_i: 2.737e-04 (the looped multiplies on the same runs: 2.725e-04;
both are mostly the scale drift of q_last != 2^30 on a sum of up to 8).  The
test allows 4 x that, the project's standing margin for seed spread.  Measured
on the device (test_engine_dot_end_to_end's seed): 2.703e-04, the loop
2.702e-04.
"""
from __future__ import annotations

import numpy as np
import pytest

import encoder as cpu_encoder
import pyoracle as orc
from dot_hybrid_ref import dot_relin_hybrid_ref
from hybrid_ref import crt_centered, n_digits
from hybrid_rescale_ref import rescale_pair
from test_gpu_hybrid import _rand

pytestmark = pytest.mark.gpu

KDOT_T = 4  # rnt_internal.hpp: the terms one k_dot_tensor launch sums
DOT_ERR_MEASURED = 2.737e-04  # tools/dot_tolerance.py


class DotCase:
    """n_terms packed ciphertext pairs of B ciphertexts over q_0..q_{Lv-1}
    (term i of ciphertext b at poly i B + b) and random key channels over
    q_0..q_{Lv-1}, p_0..p_{K-1}.  edge: all-(q-1) ciphertexts in every term and
    an all-(m-1) key.  place as test_gpu_hybrid.Case's."""

    def __init__(self, rn, log_n, Lv, K, alpha, B, bits, n_terms, edge=False, place="view", seed=0, n_special=None):
        self.rn, self.n, self.Lv, self.K, self.alpha, self.B, self.nt = rn, 1 << log_n, Lv, K, alpha, B, n_terms
        n = self.n
        self.emod = rn.generate_primes(bits, Lv + K, n)
        self.mod = self.emod[:Lv]
        self.beta = n_digits(Lv, alpha)
        rng = np.random.default_rng(7300 + 41 * log_n + 7 * n_terms + seed)
        self.x0, self.x1, self.y0, self.y1 = (_rand(rng, self.mod, n, n_terms * B) for _ in range(4))
        self.ka, self.kb = _rand(rng, self.emod, n, self.beta), _rand(rng, self.emod, n, self.beta)
        if edge:
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            for c in (self.x0, self.x1, self.y0, self.y1):
                c[:] = np.broadcast_to(qm1, c.shape)
            mm1 = np.array(self.emod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.ka[:] = np.broadcast_to(mm1, self.ka.shape)
            self.kb[:] = np.broadcast_to(mm1, self.kb.shape)
        self.ext = rn.RnsBasis(self.emod, n)
        self.basis = self.ext.drop_last(K) if place == "view" else rn.RnsBasis(self.mod, n)
        self.Bc, self.Be = orc.Basis(self.mod, n), orc.Basis(self.emod, n)
        self.key = rn.RnsHybridKey.from_channels(self.ka, self.kb, self.ext, alpha, n_special=n_special)
        self.upload()

    def upload(self, basis=None):
        rn = self.rn
        self.basis = basis or self.basis
        up = lambda x: rn.RnsPoly.from_channels(x, self.basis)  # noqa: E731
        self.ctx = rn.Ciphertext(up(self.x0), up(self.x1))
        self.cty = rn.Ciphertext(up(self.y0), up(self.y1))

    def yardstick(self, p, ka=None, kb=None, Be=None):
        """Un-rescaled and rescaled yardstick words of ciphertext p."""
        ka, kb, Be = (self.ka if ka is None else ka), (self.kb if kb is None else kb), Be or self.Be
        pick = lambda x: x[p::self.B]  # noqa: E731  (term i of ciphertext p at poly i B + p)
        r = dot_relin_hybrid_ref(self.Bc, Be, pick(self.x0), pick(self.x1), pick(self.y0), pick(self.y1), ka, kb,
                                 self.alpha)
        return r, rescale_pair(self.Bc, *r)


def _term_sum(rn, p, n_terms, B):
    acc = None
    for i in range(n_terms):
        t = rn.RnsPoly(p.basis, B)
        t.copy_polys(p, 0, i * B, B)
        acc = t if acc is None else acc + t
    return acc


def composition(rn, ctx, cty, n_terms, key, rescale):
    """The definition on the device, from existing ops alone."""
    B = ctx.c0.n_polys // n_terms
    d0 = _term_sum(rn, ctx.c0 * cty.c0, n_terms, B)
    d1 = _term_sum(rn, ctx.c0 * cty.c1 + ctx.c1 * cty.c0, n_terms, B)
    d2 = _term_sum(rn, ctx.c1 * cty.c1, n_terms, B)
    a0, a1 = rn.keyswitch_hybrid(d2, key)
    out = rn.Ciphertext(d0 + a0, d1 + a1)
    return rn.rescale_ciphertext(out) if rescale else out


def _same(a, b):
    return np.array_equal(a.c0.channels(), b.c0.channels()) and np.array_equal(a.c1.channels(), b.c1.channels())


def check_dot(c, key=None, yard=True, **yk):
    """Both calls against the device composition on every poly and against the
    yardstick on polys {0, B - 1}."""
    rn = c.rn
    key = key or c.key
    outs = {}
    for rescale in (False, True):
        fused = rn.dot_ciphertexts_hybrid(c.ctx, c.cty, c.nt, key, rescale=rescale)
        comp = composition(rn, c.ctx, c.cty, c.nt, key, rescale)
        for o in (fused.c0, fused.c1):
            assert not o.is_ntt_domain() and o.n_polys == c.B and o.basis.channel_count() == c.Lv - int(rescale)
        assert fused.c0.basis is fused.c1.basis
        assert np.array_equal(fused.c0.channels_batch(), comp.c0.channels_batch()), f"out0, rescale={rescale}"
        assert np.array_equal(fused.c1.channels_batch(), comp.c1.channels_batch()), f"out1, rescale={rescale}"
        outs[rescale] = fused
    for p in sorted({0, c.B - 1}) if yard else ():
        refs = c.yardstick(p, **yk)
        for rescale in (False, True):
            r0, r1 = refs[int(rescale)]
            assert np.array_equal(outs[rescale].c0.channels_of(p)[0], r0), f"out0 of poly {p}, rescale={rescale}"
            assert np.array_equal(outs[rescale].c1.channels_of(p)[0], r1), f"out1 of poly {p}, rescale={rescale}"
    # the inputs are const
    assert np.array_equal(c.ctx.c0.channels_batch(), c.x0) and np.array_equal(c.cty.c1.channels_batch(), c.y1)
    return outs


@pytest.mark.parametrize("n_terms", [1, 2, KDOT_T, KDOT_T + 1, 2 * KDOT_T + 1])
def test_group_and_accumulate_boundaries(gpu, n_terms):
    c = DotCase(gpu, 8, 3, 2, 2, 3, 31, n_terms)
    outs = check_dot(c)
    if n_terms == 1:  # the exact words of the hybrid multiplies
        assert _same(outs[False], gpu.mul_ciphertexts_hybrid(c.ctx, c.cty, c.key))
        assert _same(outs[True], gpu.mul_ciphertexts_hybrid_rescale(c.ctx, c.cty, c.key))


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,n_terms", [
    (8, 3, 2, 2, 3, 31, 2 * KDOT_T + 1),
    (12, 3, 2, 2, 2, 61, KDOT_T + 1),
])
def test_accumulator_bounds_on_the_largest_residues(gpu, log_n, Lv, K, alpha, B, bits, n_terms):
    check_dot(DotCase(gpu, log_n, Lv, K, alpha, B, bits, n_terms, edge=True))


# log_n, Lv, K, alpha, B, bits, ws_mb
SHAPES = [
    (8, 2, 1, 1, 2, 31, None),    # a single output limb
    (12, 3, 2, 2, 2, 31, None),   # whole-plane transforms
    (14, 3, 2, 2, 3, 31, "1"),    # several chunks
    (14, 2, 1, 2, 2, 61, None),   # u64 four-step
    (16, 4, 2, 2, 2, 31, None),   # matrix-core transforms
    (17, 4, 2, 2, 1, 31, None),   # largest ring
    (14, 3, 2, 2, 64, 31, None),  # un-split grids
]


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb", SHAPES)
def test_dot_parity(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    check_dot(DotCase(gpu, log_n, Lv, K, alpha, B, bits, 3, seed=B))


@pytest.mark.parametrize("log_n", [8, 14])
def test_ciphertexts_on_an_unrelated_root(gpu, log_n):
    check_dot(DotCase(gpu, log_n, 3, 2, 2, 3, 31, 3, place="root", seed=1))


def test_when_the_contexts_transform_differently(gpu, monkeypatch):
    """A key basis created with RNT_PLANE=0 under ciphertexts on a default
    context: the rescaling call takes the un-seeded route."""
    monkeypatch.setenv("RNT_PLANE", "0")  # read at rnt_ctx_create
    c = DotCase(gpu, 12, 3, 2, 2, 2, 31, 3, place="root", seed=9)
    monkeypatch.delenv("RNT_PLANE")
    c.upload(gpu.RnsBasis(c.mod, c.n))
    check_dot(c)


@pytest.mark.parametrize("log_n,n_terms", [(8, KDOT_T + 1), (14, 3)])
def test_squares(gpu, log_n, n_terms):
    """y is x: equal to the call on copies (and so to the composition)."""
    rn = gpu
    c = DotCase(rn, log_n, 3, 2, 2, 2, 31, n_terms, seed=2)
    copies = rn.Ciphertext(c.ctx.c0.clone(), c.ctx.c1.clone())
    for rescale in (False, True):
        sq = rn.dot_ciphertexts_hybrid(c.ctx, c.ctx, n_terms, c.key, rescale=rescale)
        assert _same(sq, rn.dot_ciphertexts_hybrid(c.ctx, copies, n_terms, c.key, rescale=rescale))
        assert _same(sq, composition(rn, c.ctx, c.ctx, n_terms, c.key, rescale))
    assert np.array_equal(c.ctx.c0.channels_batch(), c.x0) and np.array_equal(c.ctx.c1.channels_batch(), c.x1)


@pytest.mark.parametrize("log_n", [8, 14])
def test_level_view_equals_the_restricted_key(gpu, log_n):
    """One full-level key (4 limbs) under 3-limb ciphertexts: the wrapper takes
    its level view, and the words are those of the restricted key on a fresh
    root."""
    rn = gpu
    n_terms = 3
    c = DotCase(rn, log_n, 4, 2, 2, 2, 31, n_terms, seed=3, n_special=2)
    lv = 3
    for name in ("x0", "x1", "y0", "y1"):
        setattr(c, name, np.ascontiguousarray(getattr(c, name)[:, :lv, :]))
    c.upload(c.ext.drop_last(c.K + c.Lv - lv))
    view = c.key.at_level(lv)
    root = rn.RnsBasis(c.mod[:lv] + c.emod[c.Lv:], c.n)
    restricted = c.key.restrict(root)
    for rescale in (False, True):
        got = rn.dot_ciphertexts_hybrid(c.ctx, c.cty, n_terms, c.key, rescale=rescale)  # picks the view itself
        assert _same(got, rn.dot_ciphertexts_hybrid(c.ctx, c.cty, n_terms, view, rescale=rescale))
        assert _same(got, rn.dot_ciphertexts_hybrid(c.ctx, c.cty, n_terms, restricted, rescale=rescale))
        assert _same(got, composition(rn, c.ctx, c.cty, n_terms, restricted, rescale))
    # a view in any other position is refused
    lib = rn.load()
    o0, o1 = rn.RnsPoly(c.basis, c.B), rn.RnsPoly(c.basis, c.B)
    with pytest.raises(rn.RnsNttError) as e:
        rn.check(lib.rnt_ct_dot_relin_hybrid(o0.handle, o1.handle, view.a.handle, c.ctx.c1.handle, c.cty.c0.handle,
                                             c.cty.c1.handle, n_terms, view.a.handle, view.b.handle, c.alpha))
    assert e.value.kind == "Unsupported"


def test_unaligned_planes(gpu):
    """Inputs, outputs and keys wrapped at an offset of one word, so none of
    their planes is 16-byte aligned: the gather takes its one-word form."""
    import torch

    n_terms = KDOT_T + 1
    c = DotCase(gpu, 8, 3, 2, 2, 3, 31, n_terms, seed=4)
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

    ins = [shifted(Bd, n_terms * c.B, x) for x in (c.ctx.c0, c.ctx.c1, c.cty.c0, c.cty.c1)]
    ka, kb = shifted(c.ext, c.beta, c.key.a, ntt=True), shifted(c.ext, c.beta, c.key.b, ntt=True)
    for rescale, call in ((False, lib.rnt_ct_dot_relin_hybrid), (True, lib.rnt_ct_dot_relin_rescale_hybrid)):
        want = composition(rn, c.ctx, c.cty, n_terms, c.key, rescale)
        g0, g1 = shifted(want.c0.basis, c.B), shifted(want.c0.basis, c.B)
        rn.check(call(g0.handle, g1.handle, *[x.handle for x in ins], n_terms, ka.handle, kb.handle, c.alpha))
        assert np.array_equal(g0.channels(), want.c0.channels()) and np.array_equal(g1.channels(), want.c1.channels())


@pytest.mark.parametrize("log_n", [12, 14])
def test_captured(gpu, log_n):
    """Both calls record into a graph after one plain run; two replays on
    refreshed inputs give the words of the plain calls."""
    n_terms = KDOT_T + 1
    c = DotCase(gpu, log_n, 3, 2, 2, 2, 31, n_terms, seed=5)
    rn, lib = c.rn, c.rn.load()
    low = c.basis.drop_last(1)
    outs = [rn.RnsPoly(c.basis, c.B) for _ in range(2)] + [rn.RnsPoly(low, c.B) for _ in range(2)]

    def run():
        args = (c.ctx.c0.handle, c.ctx.c1.handle, c.cty.c0.handle, c.cty.c1.handle, n_terms, c.key.a.handle,
                c.key.b.handle, c.alpha)
        rn.check(lib.rnt_ct_dot_relin_hybrid(outs[0].handle, outs[1].handle, *args))
        rn.check(lib.rnt_ct_dot_relin_rescale_hybrid(outs[2].handle, outs[3].handle, *args))

    run()
    with c.basis.capture() as g:
        run()
    rng = np.random.default_rng(63 + log_n)
    for _ in range(2):
        n0, n1 = _rand(rng, c.mod, c.n, n_terms * c.B), _rand(rng, c.mod, c.n, n_terms * c.B)
        c.ctx.c0.copy_polys(rn.RnsPoly.from_channels(n0, c.basis))
        c.cty.c1.copy_polys(rn.RnsPoly.from_channels(n1, c.basis))
        g.replay()
        c.basis.sync()
        plain = rn.dot_ciphertexts_hybrid(c.ctx, c.cty, n_terms, c.key, rescale=False)
        assert np.array_equal(outs[0].channels(), plain.c0.channels())
        assert np.array_equal(outs[1].channels(), plain.c1.channels())
        assert _same(plain, composition(rn, c.ctx, c.cty, n_terms, c.key, False))
        resc = rn.dot_ciphertexts_hybrid(c.ctx, c.cty, n_terms, c.key, rescale=True)
        assert np.array_equal(outs[2].channels(), resc.c0.channels())
        assert np.array_equal(outs[3].channels(), resc.c1.channels())


NAMES = ("modup", "hoist_mac", "moddown_rescale", "moddown", "rescale", "dot_tensor")


def _counts(basis, run):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in NAMES}
    basis.profile_enable(False)
    print(counts)
    return counts


def test_launch_counts(gpu):
    """5 terms in one chunk at 2^14: one ModUp, one key-product launch and two
    k_moddown_rescale launches, where the loop of fused multiplies pays each
    five times."""
    rn = gpu
    n_terms = 5
    c = DotCase(rn, 14, 3, 2, 2, 2, 31, n_terms, seed=6)
    fused = _counts(c.basis, lambda: rn.dot_ciphertexts_hybrid(c.ctx, c.cty, n_terms, c.key))
    assert (fused["modup"], fused["hoist_mac"], fused["moddown_rescale"]) == (1, 1, 2)
    assert (fused["moddown"], fused["rescale"]) == (0, 0)
    assert fused["dot_tensor"] == -(-n_terms // KDOT_T) >= 1
    xs = [rn.Ciphertext(_slice(rn, c.ctx.c0, i, c.B), _slice(rn, c.ctx.c1, i, c.B)) for i in range(n_terms)]
    ys = [rn.Ciphertext(_slice(rn, c.cty.c0, i, c.B), _slice(rn, c.cty.c1, i, c.B)) for i in range(n_terms)]

    def loop():
        for a, b in zip(xs, ys):
            rn.mul_ciphertexts_hybrid_rescale(a, b, c.key)

    comp = _counts(c.basis, loop)
    assert (comp["modup"], comp["hoist_mac"], comp["moddown_rescale"]) == (5, 5, 10)
    assert comp["dot_tensor"] == 0
    plain = _counts(c.basis, lambda: rn.dot_ciphertexts_hybrid(c.ctx, c.cty, n_terms, c.key, rescale=False))
    assert (plain["modup"], plain["hoist_mac"], plain["moddown"], plain["moddown_rescale"]) == (1, 1, 2, 0)


def _slice(rn, p, i, B):
    t = rn.RnsPoly(p.basis, B)
    t.copy_polys(p, 0, i * B, B)
    return t


def test_errors(gpu):
    """Every row of the header's table, with its status and fields; a refused
    call leaves marked outputs untouched."""
    n_terms = 3
    c = DotCase(gpu, 8, 3, 2, 2, 2, 31, n_terms, seed=7)
    rn, lib, Bd, Lv, B, n = c.rn, c.rn.load(), c.basis, c.Lv, c.B, c.n
    low = Bd.drop_last(1)
    rng = np.random.default_rng(68)
    marks = {False: (_rand(rng, c.mod, n, B), _rand(rng, c.mod, n, B)),
             True: (_rand(rng, c.mod[:-1], n, B), _rand(rng, c.mod[:-1], n, B))}
    outs = {False: tuple(rn.RnsPoly.from_channels(m, Bd) for m in marks[False]),
            True: tuple(rn.RnsPoly.from_channels(m, low) for m in marks[True])}

    def keypoly(count, basis, ntt=True):
        L = basis.channel_count()
        return rn.RnsPoly.from_channels(np.zeros((count, L, n), np.uint64), basis, in_ntt_domain=ntt)

    for rescale in (False, True):
        o0, o1 = outs[rescale]
        fn = lib.rnt_ct_dot_relin_rescale_hybrid if rescale else lib.rnt_ct_dot_relin_hybrid

        def dot(out0=o0, out1=o1, x0=c.ctx.c0, x1=c.ctx.c1, y0=c.cty.c0, y1=c.cty.c1, nt=n_terms, ka=c.key.a,
                kb=c.key.b, alpha=c.alpha):
            return fn(out0.handle, out1.handle, x0.handle, x1.handle, y0.handle, y1.handle, nt, ka.handle, kb.handle,
                      alpha)

        def fails(kind, fields=None, **kw):
            with pytest.raises(rn.RnsNttError) as e:
                rn.check(dot(**kw))
            assert e.value.kind == kind, (kind, rescale, kw.keys(), str(e.value))
            if fields is not None:
                assert e.value.fields == fields, e.value.fields
            for o, m in zip(outs[rescale], marks[rescale]):
                assert np.array_equal(o.channels(), m), kw.keys()

        ob = o0.basis
        fails("BadArgument", nt=0)
        fails("BadArgument", nt=4)  # 6 polys are no 4 terms
        fails("BadArgument", x1=rn.RnsPoly(Bd, n_terms * B + 1))  # input poly counts differ
        fails("BadArgument", y0=rn.RnsPoly(Bd, B))
        fails("BadArgument", out0=rn.RnsPoly(ob, B + 1))  # outputs of other than B polys
        fails("BadArgument", out1=rn.RnsPoly(ob, n_terms * B))
        fails("BadArgument", out1=o0)  # out0 == out1
        fails("BadArgument", alpha=0)
        if not rescale:  # an output that is an input (the rescaling call's outputs live on another context)
            six = rn.RnsPoly.from_channels(c.x0, Bd)
            with pytest.raises(rn.RnsNttError) as e:
                rn.check(fn(six.handle, o1.handle, six.handle, c.ctx.c1.handle, c.cty.c0.handle, c.cty.c1.handle, 1,
                            c.key.a.handle, c.key.b.handle, c.alpha))
            assert e.value.kind == "BadArgument" and np.array_equal(six.channels(), c.x0)
        # inputs on two contexts; outputs on the wrong context
        fails("BasisMismatch", y1=rn.RnsPoly(rn.RnsBasis(c.mod, n), n_terms * B))
        wrongs = (Bd, Bd.drop_last(2), rn.RnsBasis(c.mod[:-1], n)) if rescale else (low, rn.RnsBasis(c.mod, n))
        for wrong in wrongs:
            fails("BasisMismatch", out0=rn.RnsPoly(wrong, B))
            fails("BasisMismatch", out1=rn.RnsPoly(wrong, B))
        if rescale:  # the right limbs on a context of their own: the outputs do not share one
            fails("BasisMismatch", out1=rn.RnsPoly(Bd.drop_last(1), B))
        for name in ("x0", "x1", "y0", "y1"):
            ntt = getattr(c.ctx if name[0] == "x" else c.cty, "c" + name[1]).clone()
            ntt.to_ntt_domain()
            fails("DomainMismatch", **{name: ntt})
        # rnt_keyswitch_hybrid's rules: key domain, key poly count, key basis, word width
        fails("DomainMismatch", ka=keypoly(c.beta, c.ext, ntt=False))
        fails("DomainMismatch", kb=keypoly(c.beta, c.ext, ntt=False))
        fails("ChannelCountMismatch", {"expected": c.beta, "actual": c.beta + 1}, ka=keypoly(c.beta + 1, c.ext))
        fails("ChannelCountMismatch", {"expected": c.beta, "actual": 1}, kb=keypoly(1, c.ext))
        fails("ChannelCountMismatch", {"expected": Lv, "actual": c.beta}, alpha=1)
        fails("BasisMismatch", ka=keypoly(c.beta, Bd), kb=keypoly(c.beta, Bd))  # no special limb
        other = rn.RnsBasis(c.emod[1:] + c.emod[:1], n)
        fails("BasisMismatch", ka=keypoly(c.beta, other), kb=keypoly(c.beta, other))
        half = rn.RnsBasis(c.emod, n // 2)
        with pytest.raises(rn.RnsNttError) as e:  # another degree
            rn.check(dot(ka=rn.RnsPoly.from_channels(np.zeros((c.beta, Lv + c.K, n // 2), np.uint64), half, True),
                         kb=rn.RnsPoly.from_channels(np.zeros((c.beta, Lv + c.K, n // 2), np.uint64), half, True)))
        assert e.value.kind == "BasisMismatch"
        wide = rn.RnsBasis(c.mod + rn.generate_primes(61, 1, n), n)
        fails("Unsupported", {"degree": 0, "max_degree": 0}, ka=keypoly(c.beta, wide), kb=keypoly(c.beta, wide))
        if rescale:  # a one-limb ciphertext: nothing to drop
            one = DotCase(gpu, 8, 1, 1, 1, B, 31, n_terms, seed=7)
            fails("InvalidModDrop", {"drop_count": 1, "channel_count": 1}, x0=one.ctx.c0, x1=one.ctx.c1,
                  y0=one.cty.c0, y1=one.cty.c1, ka=one.key.a, kb=one.key.b, alpha=1)
        # the valid call still runs after all that
        rn.check(dot())
        want = composition(rn, c.ctx, c.cty, n_terms, c.key, rescale)
        assert np.array_equal(o0.channels(), want.c0.channels()) and np.array_equal(o1.channels(), want.c1.channels())


def test_python_layer_guards(gpu):
    c = DotCase(gpu, 8, 3, 2, 2, 2, 31, 2, seed=8)
    rn = c.rn
    rng = np.random.default_rng(69)
    gk = rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.Lv), _rand(rng, c.mod, c.n, c.Lv), c.basis)
    with pytest.raises(TypeError):
        rn.dot_ciphertexts_hybrid(c.ctx, c.cty, 2, gk)
    with pytest.raises(ValueError):
        rn.dot_ciphertexts_hybrid(c.ctx, c.cty, 3, c.key)  # 4 polys are no 3 terms
    with pytest.raises(ValueError):
        rn.dot_ciphertexts_hybrid(c.ctx, c.cty, 0, c.key)


def test_engine_dot_end_to_end(gpu):
    """The evaluator tests' ring (N = 2^10, 7 x 30-bit primes, K = 2, alpha = 2,
    scale 2^30), 8 terms: encrypt -> dot_ciphertexts_hybrid -> decrypt ->
    decode against numpy's sum_i a_i b_i, within 4 x tools/dot_tolerance.py's
    figure; the looped mul_ciphertexts_hybrid_rescale + add_ciphertexts on the
    same inputs is held to the same tolerance.  Measured on the device:
    2.703e-04 for the new call, 2.702e-04 for the loop (tolerance 1.095e-03)."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L, K, alpha, logp, n_terms = 1024, 512, 7, 2, 2, 30, 8
    q, p = orc.generate_primes(logp, L, n), orc.generate_primes(31, K, n)
    eng = CkksEngine(q, n, error_std=3.2, hamming_weight=n // 2, special_moduli=p)
    rng = rn.DeviceRng(91)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    rlk = eng.generate_hybrid_relin_key(sk, rng, alpha)
    host = np.random.default_rng(92)
    a, b = host.uniform(-1, 1, (n_terms, slots)), host.uniform(-1, 1, (n_terms, slots))
    enc = rn.CkksEncoder(n, logp)
    cas = [eng.encrypt(enc.encode(v, eng.basis), pk, rng, logp=logp) for v in a]
    cbs = [eng.encrypt(enc.encode(v, eng.basis), pk, rng, logp=logp) for v in b]

    def pack(cts):
        c0, c1 = rn.RnsPoly(eng.basis, n_terms), rn.RnsPoly(eng.basis, n_terms)
        for i, ct in enumerate(cts):
            c0.copy_polys(ct.c0, i, 0, 1)
            c1.copy_polys(ct.c1, i, 0, 1)
        return rn.Ciphertext(c0, c1, cts[0].logp, cts[0].logq)

    ctx, cty = pack(cas), pack(cbs)
    low = eng.basis.drop_last(1)
    got = CkksEngine.dot_ciphertexts_hybrid(ctx, cty, n_terms, rlk, out_basis=low)
    assert got.c0.n_polys == 1 and got.c0.basis is low and low.channel_count() == L - 1
    assert got.logp == 2 * logp - q[-1].bit_length() and got.logq == ctx.logq - q[-1].bit_length()
    assert _same(got, composition(rn, ctx, cty, n_terms, rlk, True))
    loop = None
    for ca, cb in zip(cas, cbs):
        t = CkksEngine.mul_ciphertexts_hybrid_rescale(ca, cb, rlk, out_basis=low)
        loop = t if loop is None else CkksEngine.add_ciphertexts(loop, t)
    assert (loop.logp, loop.logq) == (got.logp, got.logq)
    want = np.sum(a * b, axis=0)
    tol = 4 * DOT_ERR_MEASURED
    sk_l = CkksEngine.secret_on(sk, low)
    errs = []
    for ct in (got, loop):
        # decrypted on the device over all L - 1 limbs, lifted with the big-integer centred CRT (180 bits) and
        # decoded at the nominal scale, as tools/dot_tolerance.py does
        dec = CkksEngine.decrypt(rn.Ciphertext(_one(rn, ct.c0), _one(rn, ct.c1)), sk_l).channels()
        coeffs = np.array(crt_centered(dec, q[: L - 1]), dtype=np.int64)
        errs.append(float(np.max(np.abs(cpu_encoder.decode_fft(coeffs, n, got.logp, slots) - want))))
    print(f"dot of {n_terms} terms: decode error {errs[0]:.3e}, looped multiplies {errs[1]:.3e} (tolerance {tol:.3e})")
    assert errs[0] <= tol
    assert errs[1] <= tol


def _one(rn, p):
    """Poly 0 of a batch (or the single polynomial) as a single polynomial."""
    return rn.RnsPoly.from_channels(np.ascontiguousarray(p.channels_batch()[0]), p.basis)
