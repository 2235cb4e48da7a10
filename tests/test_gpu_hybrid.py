"""Hybrid key-switching on the GPU (rnt_keyswitch_hybrid, rnt_ct_rotate_hybrid,
rnt_ct_mul_relin_hybrid): digits of alpha limbs raised to Q u P (k_modup), one
multiply-accumulate against a key over Q u P, division by P (k_moddown).  Exact
arithmetic with canonical outputs, so the calls must reproduce the CPU
yardstick (tests/hybrid_ref.py, itself checked in tests/test_hybrid_ref.py)
word for word, on every kind of ring the transforms treat differently.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from hybrid_ref import keyswitch_hybrid_ref, mul_relin_hybrid_ref, n_digits, restrict_key, rotate_hybrid_ref

pytestmark = pytest.mark.gpu

STEP = -3


def _rand(rng, mod, n, batch):
    return orc.uniform_poly(mod, n, rng, batch=batch)


class Case:
    """Random ciphertexts over q_0..q_{Lv-1} and random key channels over
    q_0..q_{Lv-1}, p_0..p_{K-1}.  `place`: "view" puts the ciphertexts on the
    drop_last(K) view of the key's root, "root" on an unrelated root basis."""

    def __init__(self, rn, log_n, Lv, K, alpha, B, bits, edge=False, place="view", seed=0):
        self.rn, self.n, self.Lv, self.K, self.alpha, self.B = rn, 1 << log_n, Lv, K, alpha, B
        n = self.n
        self.emod = rn.generate_primes(bits, Lv + K, n)
        self.mod = self.emod[:Lv]
        self.beta = n_digits(Lv, alpha)
        rng = np.random.default_rng(5200 + 41 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.c0p, self.c1p = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.ka, self.kb = _rand(rng, self.emod, n, self.beta), _rand(rng, self.emod, n, self.beta)
        if edge:  # an all-(q-1) ciphertext and an all-(m-1) key
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            for c in (self.c0, self.c1, self.c0p, self.c1p):
                c[B - 1] = np.broadcast_to(qm1, (Lv, n))
            mm1 = np.array(self.emod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.ka[:] = np.broadcast_to(mm1, self.ka.shape)
            self.kb[:] = np.broadcast_to(mm1, self.kb.shape)
        self.ext = rn.RnsBasis(self.emod, n)
        self.basis = self.ext.drop_last(K) if place == "view" else rn.RnsBasis(self.mod, n)
        self.Bc, self.Be = orc.Basis(self.mod, n), orc.Basis(self.emod, n)
        self.key = rn.RnsHybridKey.from_channels(self.ka, self.kb, self.ext, alpha, rotation=STEP)
        up = lambda x: rn.RnsPoly.from_channels(x, self.basis)  # noqa: E731
        self.ct = rn.Ciphertext(up(self.c0), up(self.c1))
        self.ctp = rn.Ciphertext(up(self.c0p), up(self.c1p))

    def check_all(self, key=None, ka=None, kb=None, Be=None):
        """The three calls against the yardstick on polys {0, B - 1}."""
        rn = self.rn
        key = key or self.key
        ka, kb, Be = (self.ka if ka is None else ka), (self.kb if kb is None else kb), Be or self.Be
        a0, a1 = rn.keyswitch_hybrid(self.ct.c1, key)
        rot = rn.rotate_ciphertext_hybrid(self.ct, key)
        mul = rn.mul_ciphertexts_hybrid(self.ct, self.ctp, key)
        for o in (a0, a1, rot.c0, rot.c1, mul.c0, mul.c1):
            assert not o.is_ntt_domain()
        for p in sorted({0, self.B - 1}):
            r0, r1 = keyswitch_hybrid_ref(Be, self.Lv, self.c1[p], ka, kb, self.alpha)
            assert np.array_equal(a0.channels_of(p)[0], r0), f"keyswitch acc0, poly {p}"
            assert np.array_equal(a1.channels_of(p)[0], r1), f"keyswitch acc1, poly {p}"
            r0, r1 = rotate_hybrid_ref(self.Bc, Be, self.c0[p], self.c1[p], STEP, ka, kb, self.alpha)
            assert np.array_equal(rot.c0.channels_of(p)[0], r0), f"rotation out0, poly {p}"
            assert np.array_equal(rot.c1.channels_of(p)[0], r1), f"rotation out1, poly {p}"
            r0, r1 = mul_relin_hybrid_ref(self.Bc, Be, self.c0[p], self.c1[p], self.c0p[p], self.c1p[p], ka, kb,
                                          self.alpha)
            assert np.array_equal(mul.c0.channels_of(p)[0], r0), f"multiply out0, poly {p}"
            assert np.array_equal(mul.c1.channels_of(p)[0], r1), f"multiply out1, poly {p}"


@pytest.mark.parametrize("log_n,Lv,K,alpha,B,bits,ws_mb,edge", [
    (8, 3, 2, 2, 3, 31, None, False),   # small four-step grid, partial last digit
    (8, 3, 2, 2, 3, 31, None, True),    # the same with an all-(q-1) ciphertext and an all-(m-1) key
    (8, 3, 1, 1, 2, 31, None, False),   # one-limb digits
    (8, 3, 3, 3, 2, 31, None, False),   # a single digit
    (12, 3, 2, 2, 2, 31, None, False),  # whole-plane ring
    (12, 3, 2, 2, 2, 61, None, False),  # u64 kernels
    (14, 3, 2, 2, 3, 31, "1", False),   # several chunks
    (14, 2, 1, 2, 2, 61, None, False),  # u64 four-step
    (16, 4, 2, 2, 2, 31, None, False),  # matrix-core transforms
    (17, 4, 2, 2, 1, 31, None, False),  # largest ring
])
def test_hybrid_parity(gpu, monkeypatch, log_n, Lv, K, alpha, B, bits, ws_mb, edge):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    Case(gpu, log_n, Lv, K, alpha, B, bits, edge=edge).check_all()


def test_large_batch_grids(gpu):
    """k_modup and k_moddown split their target-limb loops over the grid while
    the vectors alone give fewer than 1024 workgroups; 64 ciphertexts at 2^14
    (1024 workgroups of vectors) take the un-split grids of both."""
    Case(gpu, 14, 3, 2, 2, 64, 31, seed=8).check_all()


def test_rotation_by_zero_copies_and_ignores_the_key(gpu):
    c = Case(gpu, 8, 3, 2, 2, 2, 31, seed=1)
    key0 = gpu.RnsHybridKey.from_channels(c.ka, c.kb, c.ext, c.alpha, rotation=0)
    out = gpu.rotate_ciphertext_hybrid(c.ct, key0)
    assert np.array_equal(out.c0.channels(), c.c0) and np.array_equal(out.c1.channels(), c.c1)


@pytest.mark.parametrize("log_n", [8, 12, 14])
def test_levelled(gpu, log_n):
    """A 4-limb chain with alpha = 2: at the top level the ciphertext is a
    view of the key's own root; one level down it is drop_last(1) of an
    unrelated 4-limb root and the key is the full key restricted to a fresh
    root over q_0..q_2, p_0, p_1."""
    rn = gpu
    top = Case(rn, log_n, 4, 2, 2, 2, 31, seed=2)
    top.check_all()
    n, q, p = top.n, top.mod, top.emod[4:]
    low = Case.__new__(Case)
    low.rn, low.n, low.Lv, low.K, low.alpha, low.B = rn, n, 3, 2, 2, 2
    low.mod, low.emod = q[:3], q[:3] + p
    for name in ("c0", "c1", "c0p", "c1p"):
        setattr(low, name, np.ascontiguousarray(getattr(top, name)[:, :3, :]))
    low.ext = rn.RnsBasis(low.emod, n)
    low.key = top.key.restrict(low.ext)
    assert low.key.a.n_polys == 2 and low.key.a.basis is low.ext and low.key.rotation == STEP
    low.ka, low.kb = restrict_key(top.ka, 4, 2, 3), restrict_key(top.kb, 4, 2, 3)
    low.Bc, low.Be = orc.Basis(low.mod, n), orc.Basis(low.emod, n)
    low.basis = rn.RnsBasis(q, n).drop_last(1)
    up = lambda x: rn.RnsPoly.from_channels(x, low.basis)  # noqa: E731
    low.ct, low.ctp = rn.Ciphertext(up(low.c0), up(low.c1)), rn.Ciphertext(up(low.c0p), up(low.c1p))
    low.check_all()
    # the same level with the ciphertext a view of the restricted key's root
    low.basis = low.ext.drop_last(2)
    low.ct, low.ctp = rn.Ciphertext(up(low.c0), up(low.c1)), rn.Ciphertext(up(low.c0p), up(low.c1p))
    low.check_all()


def test_unaligned_planes(gpu):
    """The scalar instantiations: the inputs and the outputs wrapped at an
    offset of one word, so none of their planes is 16-byte aligned."""
    import torch

    c = Case(gpu, 8, 3, 2, 2, 3, 31, seed=3)
    rn, lib, Bd = c.rn, c.rn.load(), c.basis
    dev = torch.device("cuda", Bd.device)

    def shifted(src=None):
        words = c.B * c.Lv * c.n
        t = torch.zeros(words + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(Bd, t.data_ptr() + 4, c.B, owner=t)
        assert v.device_ptr()[0] % 16 == 4
        if src is not None:
            v.copy_polys(src)
        return v

    w0, w1 = rn.keyswitch_hybrid(c.ct.c1, c.key)
    g0, g1 = shifted(), shifted()
    s0, s1 = shifted(c.ct.c0), shifted(c.ct.c1)
    rn.check(lib.rnt_keyswitch_hybrid(g0.handle, g1.handle, s1.handle, c.key.a.handle, c.key.b.handle, c.alpha))
    assert np.array_equal(g0.channels(), w0.channels()) and np.array_equal(g1.channels(), w1.channels())
    want = rn.rotate_ciphertext_hybrid(c.ct, c.key)
    rn.check(lib.rnt_ct_rotate_hybrid(g0.handle, g1.handle, s0.handle, s1.handle, STEP, c.key.a.handle,
                                      c.key.b.handle, c.alpha))
    assert np.array_equal(g0.channels(), want.c0.channels()) and np.array_equal(g1.channels(), want.c1.channels())
    r0, r1 = rotate_hybrid_ref(c.Bc, c.Be, c.c0[1], c.c1[1], STEP, c.ka, c.kb, c.alpha)
    assert np.array_equal(g0.channels_of(1)[0], r0) and np.array_equal(g1.channels_of(1)[0], r1)


NAMES = ("modup", "moddown", "hoist_mac", "ks_decompose", "ks_rows", "ks_whole", "hoist_digits")


def _counts(basis, run):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in NAMES}
    basis.profile_enable(False)
    print(counts)
    return counts


def test_launch_counts(gpu):
    """One chunk: one ModUp, one multiply-accumulate, a ModDown per output,
    and none of the gadget key-switch's kernels."""
    c = Case(gpu, 14, 3, 2, 2, 2, 31, seed=4)
    counts = _counts(c.basis, lambda: gpu.rotate_ciphertext_hybrid(c.ct, c.key))
    assert counts["modup"] == 1 and counts["hoist_mac"] == 1 and counts["moddown"] >= 1
    for k in ("ks_decompose", "ks_rows", "ks_whole", "hoist_digits"):
        assert counts[k] == 0, k


def test_launch_counts_chunked(gpu, monkeypatch):
    monkeypatch.setenv("RNT_KS_WS_MB", "1")
    c = Case(gpu, 14, 3, 2, 2, 3, 31, seed=4)
    counts = _counts(c.basis, lambda: gpu.rotate_ciphertext_hybrid(c.ct, c.key))
    assert counts["modup"] == 3 and counts["hoist_mac"] == 3


@pytest.mark.parametrize("log_n", [12, 14])
def test_captured(gpu, log_n):
    """The three calls record into a graph after one plain run; two replays on
    refreshed inputs give the words of the plain calls."""
    c = Case(gpu, log_n, 3, 2, 2, 2, 31, seed=5)
    rn, lib, Bd = c.rn, c.rn.load(), c.basis
    outs = [rn.RnsPoly(Bd, c.B) for _ in range(6)]
    h = [o.handle for o in outs]
    ka, kb = c.key.a.handle, c.key.b.handle

    def run():
        rn.check(lib.rnt_keyswitch_hybrid(h[0], h[1], c.ct.c1.handle, ka, kb, c.alpha))
        rn.check(lib.rnt_ct_rotate_hybrid(h[2], h[3], c.ct.c0.handle, c.ct.c1.handle, STEP, ka, kb, c.alpha))
        rn.check(lib.rnt_ct_mul_relin_hybrid(h[4], h[5], c.ct.c0.handle, c.ct.c1.handle, c.ctp.c0.handle,
                                             c.ctp.c1.handle, ka, kb, c.alpha))

    run()
    with Bd.capture() as g:
        run()
    rng = np.random.default_rng(47 + log_n)
    for _ in range(2):
        n0, n1 = _rand(rng, c.mod, c.n, c.B), _rand(rng, c.mod, c.n, c.B)
        c.ct.c0.copy_polys(rn.RnsPoly.from_channels(n0, Bd))
        c.ct.c1.copy_polys(rn.RnsPoly.from_channels(n1, Bd))
        g.replay()
        Bd.sync()
        got = [o.channels() for o in outs]
        a0, a1 = rn.keyswitch_hybrid(c.ct.c1, c.key)
        rot = rn.rotate_ciphertext_hybrid(c.ct, c.key)
        mul = rn.mul_ciphertexts_hybrid(c.ct, c.ctp, c.key)
        want = [x.channels() for x in (a0, a1, rot.c0, rot.c1, mul.c0, mul.c1)]
        for i in range(6):
            assert np.array_equal(got[i], want[i]), i
        r0, r1 = rotate_hybrid_ref(c.Bc, c.Be, n0[0], n1[0], STEP, c.ka, c.kb, c.alpha)
        assert np.array_equal(got[2][0], r0) and np.array_equal(got[3][0], r1)


def test_errors(gpu):
    """Every row of the error table, with its status and fields; a refused
    call leaves the outputs untouched."""
    c = Case(gpu, 8, 3, 2, 2, 2, 31, seed=6)
    rn, lib, Bd, Lv, B, n = c.rn, c.rn.load(), c.basis, c.Lv, c.B, c.n
    rng = np.random.default_rng(48)
    mark0, mark1 = _rand(rng, c.mod, n, B), _rand(rng, c.mod, n, B)
    o0, o1 = rn.RnsPoly.from_channels(mark0, Bd), rn.RnsPoly.from_channels(mark1, Bd)

    def ks(acc0=o0, acc1=o1, d=c.ct.c1, ka=c.key.a, kb=c.key.b, alpha=c.alpha):
        return lib.rnt_keyswitch_hybrid(acc0.handle, acc1.handle, d.handle, ka.handle, kb.handle, alpha)

    def rot(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, ka=c.key.a, kb=c.key.b, alpha=c.alpha, k=STEP):
        return lib.rnt_ct_rotate_hybrid(out0.handle, out1.handle, c0.handle, c1.handle, k, ka.handle, kb.handle, alpha)

    def mul(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, c0p=c.ctp.c0, c1p=c.ctp.c1, ka=c.key.a, kb=c.key.b,
            alpha=c.alpha):
        return lib.rnt_ct_mul_relin_hybrid(out0.handle, out1.handle, c0.handle, c1.handle, c0p.handle, c1p.handle,
                                           ka.handle, kb.handle, alpha)

    def fails(kind, fn, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(fn(**kw))
        assert e.value.kind == kind, (kind, fn.__name__, kw.keys(), str(e.value))
        if fields is not None:
            assert e.value.fields == fields, e.value.fields
        assert np.array_equal(o0.channels(), mark0) and np.array_equal(o1.channels(), mark1), kw.keys()

    def keypoly(count, basis=c.ext, ntt=True):
        L = basis.channel_count()
        return rn.RnsPoly.from_channels(np.zeros((count, L, n), np.uint64), basis, in_ntt_domain=ntt)

    for fn in (ks, rot, mul):
        fails("BadArgument", fn, alpha=0)
    fails("BadArgument", ks, acc1=o0)
    fails("BadArgument", rot, out1=o0)
    fails("BadArgument", mul, out1=o0)
    fails("BadArgument", ks, acc0=c.ct.c1, acc1=rn.RnsPoly(Bd, B))  # an accumulator aliasing d
    fails("BadArgument", ks, acc1=c.ct.c1, acc0=rn.RnsPoly(Bd, B))
    for fn, name in ((ks, "acc0"), (rot, "out0"), (mul, "out1")):  # wrong output size
        fails("BadArgument", fn, **{name: rn.RnsPoly(Bd, B + 1)})
    # degree, device or moduli-prefix mismatch
    half = rn.RnsBasis(rn.generate_primes(31, Lv + c.K, n // 2), n // 2)
    hk = rn.RnsPoly.from_channels(np.zeros((c.beta, Lv + c.K, n // 2), np.uint64), half, in_ntt_domain=True)
    other = rn.RnsBasis(c.emod[1:] + c.emod[:1], n)  # the same primes in another order
    for fn in (ks, rot, mul):
        fails("BasisMismatch", fn, ka=hk, kb=hk)
        fails("BasisMismatch", fn, ka=keypoly(c.beta, other), kb=keypoly(c.beta, other))
        # E without a special limb: the ciphertext's own basis, and a shorter one
        fails("BasisMismatch", fn, ka=keypoly(c.beta, Bd), kb=keypoly(c.beta, Bd))
        fails("BasisMismatch", fn, ka=keypoly(c.beta, c.ext.drop_last(c.K + 1)), kb=keypoly(c.beta, c.ext.drop_last(c.K + 1)))
    # different device word widths: a 61-bit special prime makes E a u64 basis
    wide = rn.RnsBasis(c.mod + rn.generate_primes(61, 1, n), n)
    for fn in (ks, rot, mul):
        fails("Unsupported", fn, {"degree": 0, "max_degree": 0}, ka=keypoly(c.beta, wide), kb=keypoly(c.beta, wide))
    for fn in (ks, rot, mul):
        fails("ChannelCountMismatch", fn, {"expected": c.beta, "actual": c.beta + 1}, ka=keypoly(c.beta + 1))
        fails("ChannelCountMismatch", fn, {"expected": c.beta, "actual": 1}, kb=keypoly(1))
        fails("ChannelCountMismatch", fn, {"expected": Lv, "actual": c.beta}, alpha=1)
        fails("DomainMismatch", fn, ka=keypoly(c.beta, ntt=False))
        fails("DomainMismatch", fn, kb=keypoly(c.beta, ntt=False))
    ntt = c.ct.c1.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", ks, d=ntt)
    fails("DomainMismatch", rot, c0=ntt)
    fails("DomainMismatch", rot, c1=ntt)
    fails("DomainMismatch", mul, c1=ntt)
    fails("DomainMismatch", mul, c0p=ntt)
    # two faults at once: the multiply compares all six operands with out0,
    # then checks alpha and the key, then the inputs' domain
    apart = rn.RnsPoly(rn.RnsBasis(c.mod, n), B)  # the right limbs on a root of their own
    fails("BasisMismatch", mul, c1p=apart, alpha=0)
    fails("BasisMismatch", mul, c0=apart, ka=keypoly(c.beta + 1))
    fails("BadArgument", mul, c1=rn.RnsPoly(Bd, B + 1), kb=keypoly(c.beta, ntt=False))
    fails("BadArgument", mul, c1=ntt, alpha=0)
    fails("ChannelCountMismatch", mul, {"expected": c.beta, "actual": c.beta + 1}, c0=ntt, ka=keypoly(c.beta + 1))
    fails("BasisMismatch", mul, c0p=ntt, ka=keypoly(c.beta, Bd), kb=keypoly(c.beta, Bd))
    # the valid calls still run after all that
    v0, v1 = rn.RnsPoly(Bd, B), rn.RnsPoly(Bd, B)
    rn.check(rot(out0=v0, out1=v1))
    r0, r1 = rotate_hybrid_ref(c.Bc, c.Be, c.c0[0], c.c1[0], STEP, c.ka, c.kb, c.alpha)
    assert np.array_equal(v0.channels_of(0)[0], r0) and np.array_equal(v1.channels_of(0)[0], r1)
    # in place, as rnt_ct_rotate allows
    ct = rn.Ciphertext(c.ct.c0.clone(), c.ct.c1.clone())
    rn.check(rot(out0=ct.c0, out1=ct.c1, c0=ct.c0, c1=ct.c1))
    assert np.array_equal(ct.c0.channels(), v0.channels()) and np.array_equal(ct.c1.channels(), v1.channels())


def test_python_layer_guards_the_key_class(gpu):
    """A gadget key given to a hybrid wrapper and a hybrid key given to a
    gadget wrapper are refused before they reach the library."""
    c = Case(gpu, 8, 3, 2, 2, 2, 31, seed=7)
    rn = c.rn
    rng = np.random.default_rng(49)
    gk = rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.Lv), _rand(rng, c.mod, c.n, c.Lv), c.basis, rotation=1)
    for call in (lambda: rn.keyswitch_hybrid(c.ct.c1, gk), lambda: rn.rotate_ciphertext_hybrid(c.ct, gk),
                 lambda: rn.mul_ciphertexts_hybrid(c.ct, c.ctp, gk), lambda: rn.keyswitch(c.ct.c1, c.key),
                 lambda: rn.rotate_ciphertext(c.ct, c.key), lambda: rn.mul_ciphertexts_gadget(c.ct, c.ctp, c.key)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        rn.RnsHybridKey.from_channels(c.ka, c.kb, c.ext, 0)
    with pytest.raises(ValueError):
        c.key.restrict(rn.RnsBasis(c.emod[1:], c.n))


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _rolled(x, k):
    r = np.roll(x, -abs(int(k)))
    return np.conj(r) if k < 0 else r


# tools/hybrid_tolerance.py, eight seeds, the same ring and parameters on the
# CPU (oracle/pyoracle, oracle/encoder.py, tests/hybrid_ref.py): largest decode
# error of the hybrid rotation and of the hybrid multiply + rescale.  The
# tolerances are 4 x these: 1.67e-4 and 1.14e-4.  (The gadget rotation of the
# same ciphertext at this scale decodes with an error of 1.6e+5: its noise,
# about 2^36, is above the 2^30 message.)
ROT_ERR_MEASURED = 4.172e-5
MUL_ERR_MEASURED = 2.859e-5


def test_engine_hybrid_end_to_end(gpu):
    """N = 2^10, 4 x 31-bit + 2 special primes, alpha = 2, a DeviceRng, scale
    2^30 (one prime per level): encrypt -> rotate_ciphertext_hybrid by 1 and by
    -3 -> decrypt -> decode against the rolled slots, and multiply two
    ciphertexts with mul_ciphertexts_hybrid -> rescale -> decrypt -> decode
    against the slot products."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L, K, alpha, logp = 1024, 512, 4, 2, 2, 30
    # the L smallest 31-bit primes (a rescale keeps the scale near 2^30) and
    # the K largest as special primes (P >= alpha max Q_d): tools/hybrid_tolerance.py's ring
    q, c = [], (1 << 30) + 1
    while len(q) < L:
        if rn.is_ntt_friendly_prime(c, n):
            q.append(c)
        c += 2 * n
    eng = CkksEngine(q, n, error_std=3.2, hamming_weight=n // 2, special_moduli=rn.generate_primes(31, K, n))
    assert eng.ext_basis.channel_count() == L + K and eng.basis.channel_count() == L
    rng = rn.DeviceRng(81)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    host = np.random.default_rng(82)
    x, y = host.uniform(-1, 1, slots), host.uniform(-1, 1, slots)
    enc = rn.CkksEncoder(n, logp)
    ctx, cty = eng.encrypt(enc.encode(x, eng.basis), pk, rng), eng.encrypt(enc.encode(y, eng.basis), pk, rng)
    worst = 0.0
    for k in (1, -3):
        rk = eng.generate_hybrid_rotation_key(sk, k, rng, alpha)
        assert rk.a.n_polys == 2 and rk.rotation == k
        out = CkksEngine.rotate_ciphertext_hybrid(ctx, rk)
        assert out.logp == logp and out.logq == ctx.logq
        got = enc.decode(CkksEngine.decrypt_plaintext(out, sk))
        err = float(np.max(np.abs(got - _rolled(x, k))))
        print(f"hybrid rotation by {k}: decode error {err:.3e}")
        worst = max(worst, err)
    rlk = eng.generate_hybrid_relin_key(sk, rng, alpha)
    prod = CkksEngine.rescale_ciphertext(CkksEngine.mul_ciphertexts_hybrid(ctx, cty, rlk))
    assert prod.logp == 2 * logp - 31
    got = enc.decode(CkksEngine.decrypt_plaintext(prod, CkksEngine.secret_on(sk, prod.c0.basis)))
    # logp counts the dropped prime as 31 bits; the true scale is 2^60 / q_last
    err_mul = float(np.max(np.abs(got - x * y * (2.0 ** (2 * logp - prod.logp) / q[-1]))))
    print(f"hybrid multiply + rescale: decode error {err_mul:.3e}")
    with pytest.raises(ValueError):
        eng.generate_hybrid_relin_key(sk, rng, 3)  # P (62 bits) < alpha max Q_d (three 31-bit limbs)
    assert worst <= 4 * ROT_ERR_MEASURED
    assert err_mul <= 4 * MUL_ERR_MEASURED
