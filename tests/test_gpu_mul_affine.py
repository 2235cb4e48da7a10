"""rnt_ct_mul_relin_rescale_affine_hybrid on the GPU: the fused multiply-add on
a hybrid key, out = w r + u z + bias with r the result of
rnt_ct_mul_relin_rescale_hybrid, the affine step in the epilogue of the two
k_moddown_rescale launches that close the multiply.

DEFINED as rnt_ct_mul_relin_rescale_hybrid followed by rnt_ct_lincomb on the
packed [r, z] with weights (w, u) and the bias: that device composition is the
yardstick of every case, word for word on every poly; the first case is also
compared with the CPU model (tests/evalmod_ref.py: the multiply's own yardstick,
then the affine step in Python integers) on polys 0 and B - 1.
"""
from __future__ import annotations

import numpy as np
import pytest

from evalmod_ref import affine_ref
from hybrid_rescale_ref import mul_relin_rescale_hybrid_ref
from test_gpu_hybrid import Case, _rand
from test_gpu_hybrid_launch_tables import EXPECTED as PLAIN_TABLES
from test_gpu_unaligned import guards, shifted

pytestmark = pytest.mark.gpu

# (w, u, bias); u None: no addend
AFFINE = [(2, -1, 0), (2, None, -(1 << 30)), (1, 1, 0), (-3, 5, (1 << 61) - 1), (0, 1, -1)]


class AffCase:
    """A Case with the outputs' basis (one object: the addend and both outputs
    share it) and an addend on it whose last poly is all q - 1."""

    def __init__(self, rn, *args, **kw):
        self.around(Case(rn, *args, **kw))

    @classmethod
    def of(cls, c):
        """Around a Case-like object prepared by the test (rn, n, Lv, B, mod, basis, key, ct, ctp)."""
        self = cls.__new__(cls)
        self.around(c)
        return self

    def around(self, c):
        self.c, self.rn = c, c.rn
        rn = c.rn
        self.low = c.basis.drop_last(1)
        self.lmod = c.mod[:-1]
        rng = np.random.default_rng(6100 + c.n + c.B)
        self.z0, self.z1 = _rand(rng, self.lmod, c.n, c.B), _rand(rng, self.lmod, c.n, c.B)
        qm1 = np.array(self.lmod, dtype=np.uint64)[:, None] - np.uint64(1)
        self.z0[c.B - 1] = self.z1[c.B - 1] = np.broadcast_to(qm1, (c.Lv - 1, c.n))
        self.plain = rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key, out_basis=self.low)
        self.z = rn.Ciphertext(rn.RnsPoly.from_channels(self.z0, self.low), rn.RnsPoly.from_channels(self.z1, self.low),
                               self.plain.logp, self.plain.logq)

    def fused(self, w, u, bias, key=None):
        c = self.c
        return self.rn.mul_ciphertexts_hybrid_rescale_affine(c.ct, c.ctp, key or c.key, w, None if u is None else self.z,
                                                             0 if u is None else u, bias, out_basis=self.low)

    def composition(self, w, u, bias, key=None):
        """mul_ciphertexts_hybrid_rescale, then ct_lincomb(rescale=False) on the packed [r, z]."""
        rn, c, B = self.rn, self.c, self.c.B
        r = rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, key or c.key, out_basis=self.low)
        if u is None:
            return rn.ct_lincomb(r, 1, [[w]], [bias], rescale=False, out_basis=self.low)
        p0, p1 = rn.RnsPoly(self.low, 2 * B, _uninit=True), rn.RnsPoly(self.low, 2 * B, _uninit=True)
        for p, rr, zz in ((p0, r.c0, self.z.c0), (p1, r.c1, self.z.c1)):
            p.copy_polys(rr, 0, 0, B)
            p.copy_polys(zz, B, 0, B)
        return rn.ct_lincomb(rn.Ciphertext(p0, p1, r.logp, r.logq), 2, [[w, u]], [bias], rescale=False,
                             out_basis=self.low)

    def check(self, w, u, bias, key=None):
        got, want = self.fused(w, u, bias, key), self.composition(w, u, bias, key)
        for o in (got.c0, got.c1):
            assert not o.is_ntt_domain() and o.n_polys == self.c.B and o.basis is self.low
        assert (got.logp, got.logq) == (self.plain.logp, self.plain.logq)
        assert np.array_equal(got.c0.channels(), want.c0.channels()), f"out0 differs from the composition {(w, u, bias)}"
        assert np.array_equal(got.c1.channels(), want.c1.channels()), f"out1 differs from the composition {(w, u, bias)}"
        return got


def _counts(basis, run, names):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in names}
    basis.profile_enable(False)
    return counts


# ---------------------------------------------------------------------------
# 1. words against the device composition and the CPU model
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring10(gpu):
    """N = 2^10, 7 x 30-bit limbs, K = 2, alpha = 2, B = 2; poly B - 1 of every
    input and of the addend is all q - 1, the key all m - 1.  The CPU model's
    multiply is computed once for polys 0 and B - 1."""
    a = AffCase(gpu, 10, 7, 2, 2, 2, 30, edge=True, seed=21)
    c = a.c
    a.ref = {p: mul_relin_rescale_hybrid_ref(c.Bc, c.Be, c.c0[p], c.c1[p], c.c0p[p], c.c1p[p], c.ka, c.kb, c.alpha)
             for p in (0, c.B - 1)}
    return a


@pytest.mark.parametrize("w,u,bias", AFFINE)
def test_words_against_composition_and_cpu_model(ring10, w, u, bias):
    a = ring10
    got = a.check(w, u, bias)
    for p, (r0, r1) in a.ref.items():  # B = 2: the bias lane of poly 1 is not lane 0
        z = None if u is None else (a.z0[p], a.z1[p])
        m0, m1 = affine_ref(a.lmod, r0, r1, w, z, u or 0, bias)
        assert np.array_equal(got.c0.channels_of(p)[0], m0), f"out0 of poly {p} differs from the CPU model"
        assert np.array_equal(got.c1.channels_of(p)[0], m1), f"out1 of poly {p} differs from the CPU model"


# ---------------------------------------------------------------------------
# 2. every register tier: KMAX 4 / 8 / 16 / generic, u32 and u64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [31, 61], ids=["u32", "u64"])
@pytest.mark.parametrize("K", [2, 5, 9, 17])
def test_every_register_tier(gpu, K, bits):
    a = AffCase(gpu, 8, K + 1, K, K, 2, bits, edge=True, seed=K)
    a.check(-3, 5, (1 << 61) - 1)
    a.check(2, None, -(1 << 30))
    counts = _counts(a.c.basis, lambda: a.fused(2, -1, 7), ("moddown_rescale_affine", "moddown_rescale", "modup"))
    assert counts == {"moddown_rescale_affine": 2, "moddown_rescale": 0, "modup": 1}, counts


# ---------------------------------------------------------------------------
# 3. the ragged split grid of moddown_rescale_t
# ---------------------------------------------------------------------------
def test_ragged_last_run(gpu):
    """Lv = 4, K = 2, alpha = 2, B = 24 at N = 2^14, 31-bit: bx = 384 workgroups
    of vectors, runs = min(3, 1024 / 384) = 2 over the 3 output limbs, jper = 2:
    {0, 1} and {2}, the second run clamped (the derivation of
    test_gpu_hybrid_tiers.py::test_ragged_last_run_moddown_rescale).  One chunk."""
    a = AffCase(gpu, 14, 4, 2, 2, 24, 31, seed=13)
    a.check(2, -1, -(1 << 30))
    counts = _counts(a.c.basis, lambda: a.fused(2, -1, -(1 << 30)),
                     ("moddown_rescale_affine", "moddown_rescale", "moddown", "modup", "lincomb"))
    assert counts == {"moddown_rescale_affine": 2, "moddown_rescale": 0, "moddown": 0, "modup": 1, "lincomb": 0}, counts


# ---------------------------------------------------------------------------
# 4. the scalar instantiation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits,which", [(31, "all"), (61, "all"), (31, "z"), (31, "out")])
def test_word_aligned_buffers(gpu, bits, which):
    """The addend and / or the outputs on wrapped buffers one word past a
    16-byte boundary, between guard words: the launcher's alignment test
    includes z, so either alone selects the one-word kernel."""
    a = AffCase(gpu, 8, 3, 2, 2, 3, bits, seed=3)
    rn, lib, c = a.rn, a.rn.load(), a.c
    want = a.composition(-3, 5, 12345)
    z0 = shifted(rn, a.low, a.z0) if which in ("all", "z") else a.z.c0
    z1 = shifted(rn, a.low, a.z1) if which in ("all", "z") else a.z.c1
    o0 = shifted(rn, a.low, c.B) if which in ("all", "out") else rn.RnsPoly(a.low, c.B)
    o1 = shifted(rn, a.low, c.B) if which in ("all", "out") else rn.RnsPoly(a.low, c.B)
    rn.check(lib.rnt_ct_mul_relin_rescale_affine_hybrid(o0.handle, o1.handle, c.ct.c0.handle, c.ct.c1.handle,
                                                        c.ctp.c0.handle, c.ctp.c1.handle, c.key.a.handle,
                                                        c.key.b.handle, c.alpha, -3, z0.handle, z1.handle, 5, 12345))
    assert np.array_equal(o0.channels(), want.c0.channels()) and np.array_equal(o1.channels(), want.c1.channels())
    guards(*[v for v in (z0, z1, o0, o1) if hasattr(v, "check_guards")])
    if which in ("all", "z"):  # the addend is an input: unchanged
        assert np.array_equal(z0.channels(), a.z0) and np.array_equal(z1.channels(), a.z1)


# ---------------------------------------------------------------------------
# 5. mixed cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,B,ws_mb", [(8, 3, None), (12, 5, "1"), (16, 2, None)])
def test_in_place_accumulation(gpu, monkeypatch, log_n, B, ws_mb):
    """z is out: every lane reads its addend word before it stores there.  The
    2^12 case runs in several chunks (1 MiB of workspace)."""
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    a = AffCase(gpu, log_n, 3, 2, 2, B, 31, seed=31)
    rn, lib, c = a.rn, a.rn.load(), a.c
    want = a.composition(2, -1, 99)
    acc0, acc1 = a.z.c0.clone(), a.z.c1.clone()
    rn.check(lib.rnt_ct_mul_relin_rescale_affine_hybrid(acc0.handle, acc1.handle, c.ct.c0.handle, c.ct.c1.handle,
                                                        c.ctp.c0.handle, c.ctp.c1.handle, c.key.a.handle,
                                                        c.key.b.handle, c.alpha, 2, acc0.handle, acc1.handle, -1, 99))
    assert np.array_equal(acc0.channels(), want.c0.channels()) and np.array_equal(acc1.channels(), want.c1.channels())
    if ws_mb is not None:
        n = _counts(c.basis, lambda: a.fused(2, -1, 99), ("modup", "moddown_rescale_affine"))
        assert n["modup"] > 1 and n["moddown_rescale_affine"] == 2 * n["modup"], n


@pytest.mark.parametrize("log_n", [8, 12])
def test_drop_last_input_and_level_view_key(gpu, log_n):
    """The inputs one level below the key's: ciphertexts on a drop_last view of
    a 4-limb basis, ONE full-level key with n_special, whose level view the
    wrapper picks (rnt_key_level_view) -- the composition picks the same."""
    rn = gpu
    top = Case(rn, log_n, 4, 2, 2, 2, 31, seed=17)
    c = Case.__new__(Case)
    c.rn, c.n, c.Lv, c.K, c.alpha, c.B, c.mod = rn, top.n, 3, 2, 2, 2, top.mod[:3]
    c.key = key = rn.RnsHybridKey.from_channels(top.ka, top.kb, top.ext, top.alpha, n_special=top.K)
    c.basis = top.basis.drop_last(1)  # a view of a view of the key's root
    up = lambda x: rn.RnsPoly.from_channels(np.ascontiguousarray(x[:, :3, :]), c.basis)  # noqa: E731
    c.ct, c.ctp = rn.Ciphertext(up(top.c0), up(top.c1)), rn.Ciphertext(up(top.c0p), up(top.c1p))
    a = AffCase.of(c)
    assert key.at_level(3).level == 3
    a.check(2, -1, -(1 << 30))
    a.check(1, None, 5)


@pytest.mark.parametrize("log_n", [12, 16])
def test_when_the_contexts_transform_differently(gpu, monkeypatch, log_n):
    """The un-seeded path (test_gpu_hybrid_rescale.py's means): a key basis
    created with RNT_PLANE=0 under ciphertexts on a default context, so the
    tensor's d0, d1 are ModDown's addends and the affine addend comes on top."""
    monkeypatch.setenv("RNT_PLANE", "0")  # read at rnt_ctx_create
    rn = gpu
    c = Case(rn, log_n, 3, 2, 2, 2, 31, place="root", seed=9)
    monkeypatch.delenv("RNT_PLANE")
    c.basis = rn.RnsBasis(c.mod, c.n)
    up = lambda x: rn.RnsPoly.from_channels(x, c.basis)  # noqa: E731
    c.ct, c.ctp = rn.Ciphertext(up(c.c0), up(c.c1)), rn.Ciphertext(up(c.c0p), up(c.c1p))
    a = AffCase.of(c)
    got = a.check(-3, 5, (1 << 61) - 1)
    r0, r1 = mul_relin_rescale_hybrid_ref(c.Bc, c.Be, c.c0[1], c.c1[1], c.c0p[1], c.c1p[1], c.ka, c.kb, c.alpha)
    m0, m1 = affine_ref(a.lmod, r0, r1, -3, (a.z0[1], a.z1[1]), 5, (1 << 61) - 1)
    assert np.array_equal(got.c0.channels_of(1)[0], m0) and np.array_equal(got.c1.channels_of(1)[0], m1)


# ---------------------------------------------------------------------------
# 6. launch table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [9, 12, 16])
def test_launch_table(gpu, log_n):
    """The plain fused multiply's table (tests/test_gpu_hybrid_launch_tables.py)
    with moddown_rescale: 2 replaced by moddown_rescale_affine: 2 and no
    lincomb; the plain multiply still profiles moddown_rescale: 2."""
    from rns_ntt import _lib

    a = AffCase(gpu, log_n, 3, 2, 2, 2, 31, seed=11)
    c, rn = a.c, a.rn
    want = dict(PLAIN_TABLES[f"ct_mul_relin_rescale_hybrid-2^{log_n}-B2"])
    assert want.pop("moddown_rescale") == 2
    want["moddown_rescale_affine"] = 2
    got = {k: v for k, v in _counts(c.basis, lambda: a.fused(2, -1, 3), _lib.PROFILE_NAMES).items() if v}
    assert got == want
    assert "lincomb" not in got
    plain = _counts(c.basis, lambda: rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key, out_basis=a.low),
                    ("moddown_rescale", "moddown_rescale_affine"))
    assert plain == {"moddown_rescale": 2, "moddown_rescale_affine": 0}


# ---------------------------------------------------------------------------
# 7. recording
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [12, 16])
def test_captured(gpu, log_n):
    """After one plain run the call records (nothing is copied from the host,
    unlike rnt_ct_lincomb); two replays on refreshed inputs give the eager
    call's words.  The graph is one chain of launches on one stream."""
    a = AffCase(gpu, log_n, 3, 2, 2, 2, 31, seed=5)
    rn, lib, c = a.rn, a.rn.load(), a.c
    outs = [rn.RnsPoly(a.low, c.B) for _ in range(2)]

    def run():
        rn.check(lib.rnt_ct_mul_relin_rescale_affine_hybrid(outs[0].handle, outs[1].handle, c.ct.c0.handle,
                                                            c.ct.c1.handle, c.ctp.c0.handle, c.ctp.c1.handle,
                                                            c.key.a.handle, c.key.b.handle, c.alpha, 2, a.z.c0.handle,
                                                            a.z.c1.handle, -1, -(1 << 30)))

    run()
    with c.basis.capture() as g:
        run()
    rng = np.random.default_rng(57 + log_n)
    for _ in range(2):
        c.ct.c0.copy_polys(rn.RnsPoly.from_channels(_rand(rng, c.mod, c.n, c.B), c.basis))
        a.z.c1.copy_polys(rn.RnsPoly.from_channels(_rand(rng, a.lmod, c.n, c.B), a.low))
        g.replay()
        c.basis.sync()
        want = a.fused(2, -1, -(1 << 30))
        assert np.array_equal(outs[0].channels(), want.c0.channels())
        assert np.array_equal(outs[1].channels(), want.c1.channels())
        comp = a.composition(2, -1, -(1 << 30))
        assert np.array_equal(want.c0.channels(), comp.c0.channels())
        assert np.array_equal(want.c1.channels(), comp.c1.channels())


# ---------------------------------------------------------------------------
# 8. every status of the header; a refused call leaves its outputs untouched
# ---------------------------------------------------------------------------
def test_errors(gpu):
    a = AffCase(gpu, 8, 3, 2, 2, 2, 31, seed=6)
    rn, lib, c, low, B, n = a.rn, a.rn.load(), a.c, a.low, a.c.B, a.c.n
    rng = np.random.default_rng(58)
    mark0, mark1 = _rand(rng, a.lmod, n, B), _rand(rng, a.lmod, n, B)
    o0, o1 = rn.RnsPoly.from_channels(mark0, low), rn.RnsPoly.from_channels(mark1, low)
    NONE = type("none", (), {"handle": None})()

    def call(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, c0p=c.ctp.c0, c1p=c.ctp.c1, ka=c.key.a, kb=c.key.b,
             alpha=c.alpha, w=2, z0=a.z.c0, z1=a.z.c1, u=-1, bias=1):
        return lib.rnt_ct_mul_relin_rescale_affine_hybrid(out0.handle, out1.handle, c0.handle, c1.handle, c0p.handle,
                                                          c1p.handle, ka.handle, kb.handle, alpha, w, z0.handle,
                                                          z1.handle, u, bias)

    def fails(kind, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(call(**kw))
        assert e.value.kind == kind, (kind, kw.keys(), str(e.value))
        if fields is not None:
            assert e.value.fields == fields, e.value.fields
        assert np.array_equal(o0.channels(), mark0) and np.array_equal(o1.channels(), mark1), kw.keys()

    def keypoly(count, basis, ntt=True):
        return rn.RnsPoly.from_channels(np.zeros((count, basis.channel_count(), n), np.uint64), basis,
                                        in_ntt_domain=ntt)

    # --- the affine arguments
    for bad in (1 << 31, -(1 << 31), (1 << 40)):
        fails("BadArgument", w=bad)
        fails("BadArgument", u=bad)
    rn.check(call(w=(1 << 31) - 1, u=-(1 << 31) + 1, bias=(1 << 62) - 1))  # the largest magnitudes allowed
    o0.copy_polys(rn.RnsPoly.from_channels(mark0, low))
    o1.copy_polys(rn.RnsPoly.from_channels(mark1, low))
    for bad in (1 << 62, -(1 << 62)):
        fails("BadArgument", bias=bad)
    rn.check(call(z0=NONE, z1=NONE, u=1 << 40))  # without addends u is ignored
    o0.copy_polys(rn.RnsPoly.from_channels(mark0, low))
    o1.copy_polys(rn.RnsPoly.from_channels(mark1, low))
    fails("BadArgument", z0=NONE)
    fails("BadArgument", z1=NONE)
    apart = c.basis.drop_last(1)  # the right limbs on a context of their own
    fails("BasisMismatch", z0=rn.RnsPoly(apart, B))
    fails("BasisMismatch", z1=rn.RnsPoly(apart, B))
    fails("BasisMismatch", z0=rn.RnsPoly(c.basis, B), z1=rn.RnsPoly(c.basis, B))  # the inputs' level
    fails("BadArgument", z0=rn.RnsPoly(low, B + 1))
    ntt = a.z.c1.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", z1=ntt)
    fails("DomainMismatch", z0=ntt)
    # a key level view in an addend position
    full = rn.RnsHybridKey.from_channels(c.ka, c.kb, c.ext, c.alpha, n_special=c.K)
    view = full.at_level(2)
    fails("Unsupported", {"degree": 0, "max_degree": 0}, z0=view.a)
    fails("Unsupported", {"degree": 0, "max_degree": 0}, z1=view.b)
    # aliasing: z0 == out0 needs z1 == out1; crossed, or an addend on the other output
    fails("BadArgument", z0=o0)
    fails("BadArgument", z1=o1)
    fails("BadArgument", z0=o1, z1=o0)
    fails("BadArgument", z1=o0)
    fails("BadArgument", out1=o0)  # out0 == out1, the multiply's rule
    # --- the multiply's own rules and statuses
    for wrong in (c.basis, c.basis.drop_last(2), rn.RnsBasis(c.mod[:-1], n)):
        fails("BasisMismatch", out0=rn.RnsPoly(wrong, B))
        fails("BasisMismatch", out1=rn.RnsPoly(wrong, B))
    fails("BasisMismatch", out1=rn.RnsPoly(c.basis.drop_last(1), B))  # the outputs do not share one context
    fails("BadArgument", out0=rn.RnsPoly(low, B + 1))
    fails("BadArgument", alpha=0)
    nin = c.ct.c1.clone()
    nin.to_ntt_domain()
    fails("DomainMismatch", c1=nin)
    fails("DomainMismatch", c0p=nin)
    fails("DomainMismatch", ka=keypoly(c.beta, c.ext, ntt=False))
    fails("ChannelCountMismatch", {"expected": c.beta, "actual": c.beta + 1}, ka=keypoly(c.beta + 1, c.ext))
    fails("ChannelCountMismatch", {"expected": c.Lv, "actual": c.beta}, alpha=1)
    fails("BasisMismatch", ka=keypoly(c.beta, c.basis), kb=keypoly(c.beta, c.basis))  # no special limb
    fails("BasisMismatch", c1=rn.RnsPoly(rn.RnsBasis(c.mod, n), B))
    fails("BadArgument", c1=rn.RnsPoly(c.basis, B + 1))
    wide = rn.RnsBasis(c.mod + rn.generate_primes(61, 1, n), n)
    fails("Unsupported", {"degree": 0, "max_degree": 0}, ka=keypoly(c.beta, wide), kb=keypoly(c.beta, wide))
    fails("Unsupported", {"degree": 0, "max_degree": 0}, c0=view.a)  # a view anywhere but the key positions
    one = Case(gpu, 8, 1, 1, 1, B, 31, seed=6)
    fails("InvalidModDrop", {"drop_count": 1, "channel_count": 1}, c0=one.ct.c0, c1=one.ct.c1, c0p=one.ctp.c0,
          c1p=one.ctp.c1, ka=one.key.a, kb=one.key.b, alpha=1)
    # --- the valid call still runs after all that, with a level-view key in the key positions too
    rn.check(call())
    want = a.composition(2, -1, 1)
    assert np.array_equal(o0.channels(), want.c0.channels()) and np.array_equal(o1.channels(), want.c1.channels())
    rn.check(call(ka=full.a, kb=full.b))  # another key object of the same words
    assert np.array_equal(o0.channels(), want.c0.channels()) and np.array_equal(o1.channels(), want.c1.channels())


def test_python_layer(gpu):
    """The wrapper: a gadget key is refused, and so is an addend whose logp or
    logq is not the result's."""
    a = AffCase(gpu, 8, 3, 2, 2, 2, 31, seed=7)
    rn, c = a.rn, a.c
    rng = np.random.default_rng(59)
    gk = rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.Lv), _rand(rng, c.mod, c.n, c.Lv), c.basis, rotation=1)
    with pytest.raises(TypeError):
        rn.mul_ciphertexts_hybrid_rescale_affine(c.ct, c.ctp, gk)
    for dp, dq in ((1, 0), (0, 1)):
        z = rn.Ciphertext(a.z.c0, a.z.c1, a.z.logp + dp, a.z.logq + dq)
        with pytest.raises(ValueError):
            rn.mul_ciphertexts_hybrid_rescale_affine(c.ct, c.ctp, c.key, 2, z, -1)
    out = rn.mul_ciphertexts_hybrid_rescale_affine(c.ct, c.ctp, c.key)  # the defaults: the plain multiply's words
    assert out.c0.basis is out.c1.basis and out.c0.basis.channel_count() == c.Lv - 1
    assert np.array_equal(out.c0.channels(), a.plain.c0.channels())
    assert np.array_equal(out.c1.channels(), a.plain.c1.channels())
