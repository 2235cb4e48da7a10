"""Key level views: one full-level hybrid key (or packed key set), resident on
the device once, as the key of every lower level (rnt_ctx_hybrid_level,
rnt_key_level_view; RnsBasis.hybrid_level, RnsHybridKey.at_level,
RnsHybridKeySet.at_level).

A hybrid call with level views is DEFINED as the same call with the restricted
key on a root context over the view's moduli, so every comparison is equality
of words: with the restricted-key device path (RnsHybridKey.restrict on a fresh
root, every poly) and, at the levels L - 1 and 1, with the CPU yardsticks
(tests/hybrid_ref.py, hybrid_hoist_ref.py, hybrid_rescale_ref.py on
restrict_key'd channels, polys {0, B - 1}).  At level 1 a ciphertext has no limb
to rescale away, so the two rescaling calls run from level 2 on.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from hybrid_hoist_ref import bsgs_hybrid_ref, rotate_hybrid_hoisted_ref
from hybrid_ref import keyswitch_hybrid_ref, mul_relin_hybrid_ref, n_digits, restrict_key, rotate_hybrid_ref
from hybrid_rescale_ref import rescale_pair

pytestmark = pytest.mark.gpu

STEP = -3
HOIST_STEPS = [1, -3, 0]
BABY, GIANT = [0, 1, 2], [0, 4]
TRANSFORMS = ("col_fwd", "row_fwd", "row_inv", "col_inv", "whole_fwd", "whole_inv", "mf_ntt_fwd", "mf_ntt_inv")
KERNELS = TRANSFORMS + ("elementwise", "rescale", "automorphism", "copy", "tensor_rows", "tensor_whole", "mf_tensor",
                        "bsgs_mac", "hoist_mac", "modup", "moddown", "moddown_auto", "moddown_rescale",
                        "ks_decompose", "ks_rows", "ks_whole", "hoist_digits")


def _rand(rng, mod, n, batch):
    return orc.uniform_poly(mod, n, rng, batch=batch)


class Ring:
    """A root key basis q_0..q_{L-1}, p_0..p_{K-1} with random full-level keys
    on it -- one ordinary key for STEP (also the multiply's), a hoisting-form
    set for HOIST_STEPS, a hoisting-form baby set and an ordinary giant set --
    and random level-L ciphertexts, whose first lv limbs are the level-lv ones."""

    def __init__(self, rn, log_n, L, K, alpha, B, bits, seed=0):
        self.rn, self.n, self.L, self.K, self.alpha, self.B = rn, 1 << log_n, L, K, alpha, B
        n = self.n
        self.emod = rn.generate_primes(bits, L + K, n)
        self.q, self.p = self.emod[:L], self.emod[L:]
        beta = n_digits(L, alpha)
        rng = np.random.default_rng(9100 + 53 * log_n + seed)
        self.ct_ch = [_rand(rng, self.q, n, B) for _ in range(4)]  # c0, c1, c0', c1'
        self.diag = _rand(rng, self.q, n, len(BABY) * len(GIANT))
        self.key_ch = (_rand(rng, self.emod, n, beta), _rand(rng, self.emod, n, beta))

        def keys(steps):
            return [None if k == 0 else (_rand(rng, self.emod, n, beta), _rand(rng, self.emod, n, beta)) for k in steps]

        self.hoist_ch, self.baby_ch, self.giant_ch = keys(HOIST_STEPS), keys(BABY), keys(GIANT)
        self.ext = rn.RnsBasis(self.emod, n)
        self.key = rn.RnsHybridKey.from_channels(*self.key_ch, self.ext, alpha, rotation=STEP, n_special=K)

        def upload(steps, chans, hoisted):
            out = []
            for k, kk in zip(steps, chans):
                hk = None if kk is None else rn.RnsHybridKey.from_channels(kk[0], kk[1], self.ext, alpha, rotation=k,
                                                                           n_special=K)
                if hk is not None and hoisted:
                    hk.prepare_hoisted()
                out.append(hk)
            return out

        self.hoist_keys = upload(HOIST_STEPS, self.hoist_ch, True)
        self.baby_keys = upload(BABY, self.baby_ch, True)
        self.giant_keys = upload(GIANT, self.giant_ch, False)
        self.hset = rn.RnsHybridKeySet(self.hoist_keys, alpha)
        self.bset = rn.RnsHybridKeySet(self.baby_keys, alpha)
        self.gset = rn.RnsHybridKeySet(self.giant_keys, alpha)

    def operands(self, basis, lv):
        """The level-lv ciphertexts and plaintexts on `basis` (lv limbs)."""
        rn = self.rn
        up = lambda x: rn.RnsPoly.from_channels(np.ascontiguousarray(x[:, :lv, :]), basis)  # noqa: E731
        c = [up(x) for x in self.ct_ch]
        d = up(self.diag)
        d.to_ntt_domain()
        return rn.Ciphertext(c[0], c[1]), rn.Ciphertext(c[2], c[3]), d

    def view_side(self, lv):
        """(ciphertext basis, keys) of the view path: a prefix of the root and
        views of the resident keys."""
        basis = self.ext.drop_last(self.K + self.L - lv)
        return basis, (self.key.at_level(lv), self.hset.at_level(lv), self.bset.at_level(lv), self.gset.at_level(lv))

    def restricted_side(self, lv):
        """The same on a fresh root over q_0..q_{lv-1}, p: restricted copies."""
        rn = self.rn
        root = rn.RnsBasis(self.q[:lv] + self.p, self.n)
        r = lambda ks: rn.RnsHybridKeySet([None if k is None else k.restrict(root) for k in ks], self.alpha)  # noqa: E731
        return root.drop_last(self.K), (self.key.restrict(root), r(self.hoist_keys), r(self.baby_keys),
                                        r(self.giant_keys))

    def run(self, basis, keys, lv, calls=None):
        """name -> [polys][lv][N] words of every call's outputs."""
        rn = self.rn
        key, hset, bset, gset = keys
        ct, ctp, d = self.operands(basis, lv)
        out = {}

        def put(name, c0, c1):
            assert not c0.is_ntt_domain() and not c1.is_ntt_domain()
            out[name + ".0"], out[name + ".1"] = c0.channels_batch(), c1.channels_batch()

        want = lambda name: calls is None or name in calls  # noqa: E731
        if want("keyswitch"):
            put("keyswitch", *rn.keyswitch_hybrid(ct.c1, key))
        if want("rotate"):
            o = rn.rotate_ciphertext_hybrid(ct, key)
            put("rotate", o.c0, o.c1)
        if want("mul"):
            o = rn.mul_ciphertexts_hybrid(ct, ctp, key)
            put("mul", o.c0, o.c1)
        if want("hoisted"):
            o = rn.rotate_ciphertext_hybrid_hoisted(ct, hset)
            put("hoisted", o.c0, o.c1)
        if want("bsgs"):
            o = rn.linear_transform_bsgs_hybrid(ct, d, bset, gset)
            put("bsgs", o.c0, o.c1)
        if lv >= 2 and want("mul_rescale"):
            o = rn.mul_ciphertexts_hybrid_rescale(ct, ctp, key)
            put("mul_rescale", o.c0, o.c1)
        if lv >= 2 and want("bsgs_rescale"):
            o = rn.linear_transform_bsgs_hybrid_rescale(ct, d, bset, gset)
            put("bsgs_rescale", o.c0, o.c1)
        return out

    def yardstick(self, got, lv):
        """Polys {0, B - 1} of `got` against the CPU definitions on the
        restricted channels."""
        L, al, n = self.L, self.alpha, self.n
        Bc, Be = orc.Basis(self.q[:lv], n), orc.Basis(self.q[:lv] + self.p, n)
        rk = lambda kk: None if kk is None else (restrict_key(kk[0], L, al, lv), restrict_key(kk[1], L, al, lv))  # noqa: E731
        ka, kb = rk(self.key_ch)
        hk, bk, gk = ([rk(x) for x in s] for s in (self.hoist_ch, self.baby_ch, self.giant_ch))
        diag = np.ascontiguousarray(self.diag[:, :lv, :])
        for p in sorted({0, self.B - 1}):
            c0, c1, c0p, c1p = (np.ascontiguousarray(x[p, :lv, :]) for x in self.ct_ch)
            ref = {}
            ref["keyswitch"] = keyswitch_hybrid_ref(Be, lv, c1, ka, kb, al)
            ref["rotate"] = rotate_hybrid_ref(Bc, Be, c0, c1, STEP, ka, kb, al)
            ref["mul"] = mul_relin_hybrid_ref(Bc, Be, c0, c1, c0p, c1p, ka, kb, al)
            ref["bsgs"] = bsgs_hybrid_ref(Bc, Be, c0, c1, BABY, GIANT, diag, bk, gk, al)
            if lv >= 2:
                ref["mul_rescale"] = rescale_pair(Bc, *ref["mul"])
                ref["bsgs_rescale"] = rescale_pair(Bc, *ref["bsgs"])
            for name, (r0, r1) in ref.items():
                assert np.array_equal(got[name + ".0"][p], r0), f"{name} out0, poly {p}, level {lv}"
                assert np.array_equal(got[name + ".1"][p], r1), f"{name} out1, poly {p}, level {lv}"
            for t, k in enumerate(HOIST_STEPS):
                r0, r1 = rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, k, *(hk[t] or (None, None)), al)
                assert np.array_equal(got["hoisted.0"][t * self.B + p], r0), f"hoisted out0, step {k}, poly {p}"
                assert np.array_equal(got["hoisted.1"][t * self.B + p], r1), f"hoisted out1, step {k}, poly {p}"

    def check_level(self, lv, yardstick):
        got = self.run(*self.view_side(lv), lv)
        want = self.run(*self.restricted_side(lv), lv)
        assert got.keys() == want.keys() and len(got) == (14 if lv >= 2 else 10)
        for name in want:
            assert np.array_equal(got[name], want[name]), f"{name} at level {lv}: view differs from the restricted key"
        if yardstick:
            self.yardstick(got, lv)


# ---------------------------------------------------------------------------
# parity of all seven calls
# ---------------------------------------------------------------------------
# log_n, L, K, alpha, B, bits, ws_mb, every level
SHAPES = [
    (8, 4, 2, 2, 3, 31, None, True),    # small four-step grid
    (8, 5, 2, 2, 2, 31, None, True),    # beta = 3: at beta' = 2 and 1 a set's step stride is not its digit count
    (12, 4, 2, 2, 2, 31, None, False),  # whole-plane ring
    (12, 4, 2, 2, 2, 61, None, False),  # u64 kernels
    (14, 4, 2, 2, 3, 31, "1", False),   # several chunks
    (14, 3, 1, 2, 2, 61, None, False),  # u64 four-step
    (16, 4, 2, 2, 2, 31, None, False),  # matrix-core transforms
    (17, 4, 2, 2, 1, 31, None, False),  # largest ring
]


@pytest.mark.parametrize("log_n,L,K,alpha,B,bits,ws_mb,every", SHAPES)
def test_level_view_parity(gpu, monkeypatch, log_n, L, K, alpha, B, bits, ws_mb, every):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    r = Ring(gpu, log_n, L, K, alpha, B, bits)
    for lv in (range(1, L + 1) if every else sorted({1, L - 1})):
        r.check_level(lv, yardstick=lv in (1, L - 1))


def test_view_shapes_and_sharing(gpu):
    """What the handles report; one level-basis object and one view per level."""
    rn = gpu
    r = Ring(rn, 8, 5, 2, 2, 2, 31, seed=1)
    for lv in range(1, 6):
        lb = r.ext.hybrid_level(2, lv)
        assert lb is r.ext.hybrid_level(2, lv)
        assert lb.channel_count() == lv + 2 and lb.moduli() == r.q[:lv] + r.p and lb.degree == r.n
        assert lb.total_bits() == sum(m.bit_length() - 1 for m in r.q[:lv] + r.p)
        assert [lb.psi(t) for t in range(lv + 2)] == [rn.find_psi(m, r.n) for m in r.q[:lv] + r.p]
        assert lb.stream() == r.ext.stream()
        v = r.key.at_level(lv)
        assert v is r.key.at_level(lv) and v.a.basis is lb and v.b.basis is lb
        assert v.a.n_polys == n_digits(lv, 2) and v.a.is_ntt_domain()
        assert (v.alpha, v.rotation, v.hoisted, v.level) == (2, STEP, False, lv)
        s = r.hset.at_level(lv)
        assert s is r.hset.at_level(lv) and s.a.basis is lb and s.hoisted and s.steps == HOIST_STEPS
        assert s.a.n_polys == len(HOIST_STEPS) * n_digits(lv, 2)


def test_wrappers_pick_the_level(gpu):
    """Keys that carry n_special serve a lower-level ciphertext as they are;
    without n_special the call is today's (the full key does not fit)."""
    rn = gpu
    r = Ring(rn, 8, 4, 2, 2, 2, 31, seed=2)
    lv = 2
    basis, views = r.view_side(lv)
    want = r.run(basis, views, lv)
    got = r.run(basis, (r.key, r.hset, r.bset, r.gset), lv)
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    plain = rn.RnsHybridKey.from_channels(*r.key_ch, r.ext, 2, rotation=STEP)
    assert plain.n_special is None
    ct, _, _ = r.operands(basis, lv)
    with pytest.raises(rn.RnsNttError) as e:
        rn.rotate_ciphertext_hybrid(ct, plain)
    assert e.value.code == rn._lib.CHANNEL_COUNT


# ---------------------------------------------------------------------------
# register tiers, scalar forms, split grids
# ---------------------------------------------------------------------------
TIERS = [4, 5, 8, 9, 16, 17]


def _tier_ring(gpu, a, bits):
    return Ring(gpu, 8, a + 2, a, a, 1, bits, seed=a)


@pytest.mark.parametrize("bits", [31, 61], ids=["u32", "u64"])
@pytest.mark.parametrize("a", TIERS)
def test_tier_level_views(gpu, a, bits):
    """alpha = K = a, L = a + 2, level a + 1: two digits (a limbs and one) and
    a gap of 1 at every AMAX / KMAX tier of k_modup and the three ModDowns.
    B = 1 at N = 2^8 is one workgroup of vectors, so every split grid runs one
    target limb a run (tper = jper = 1) and the map is applied per run."""
    r = _tier_ring(gpu, a, bits)
    r.check_level(a + 1, yardstick=False)


@pytest.mark.parametrize("bits", [31, 61], ids=["u32", "u64"])
@pytest.mark.parametrize("a", TIERS)
def test_tier_level_views_unaligned(gpu, a, bits):
    """The scalar (one-word) forms: ciphertext and outputs wrapped at an offset
    of one word, as test_gpu_hybrid.test_unaligned_planes does."""
    import torch

    rn, lib = gpu, gpu.load()
    r = _tier_ring(gpu, a, bits)
    lv = a + 1
    basis, (key, _, _, _) = r.view_side(lv)
    ct, _, _ = r.operands(basis, lv)
    want = rn.rotate_ciphertext_hybrid(ct, key)  # the aligned view path, checked by test_tier_level_views
    dev = torch.device("cuda", basis.device)
    wb = 4 if bits == 31 else 8

    def shifted(src=None):
        t = torch.zeros(r.B * lv * r.n * wb // 4 + 4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(basis, t.data_ptr() + wb, r.B, owner=t)
        assert v.device_ptr()[0] % 16 == wb
        if src is not None:
            v.copy_polys(src)
        return v

    g0, g1, s0, s1 = shifted(), shifted(), shifted(ct.c0), shifted(ct.c1)
    rn.check(lib.rnt_ct_rotate_hybrid(g0.handle, g1.handle, s0.handle, s1.handle, STEP, key.a.handle, key.b.handle,
                                      key.alpha))
    assert np.array_equal(g0.channels_batch(), want.c0.channels_batch())
    assert np.array_equal(g1.channels_batch(), want.c1.channels_batch())


def test_split_run_straddles_the_level(gpu):
    """N = 2^14, B = 16, L = 5, K = 2, alpha = 2 at level 4 (gap 1): a chunk is
    bx = 16 B = 256 workgroups of vectors, beta' = 2, so modup_t splits the
    LE = 6 target limbs into min(6, 1024 / (256 x 2)) = 2 runs of tper = 3 --
    {0, 1, 2} and {3, 4, 5} -- and the second run crosses level = 4 inside its
    loop: working limb 3 is root limb 3, working limbs 4 and 5 root limbs 5, 6."""
    r = Ring(gpu, 14, 5, 2, 2, 16, 31, seed=3)
    lv = 4
    calls = {"rotate", "mul_rescale"}
    got = r.run(*r.view_side(lv), lv, calls)
    want = r.run(*r.restricted_side(lv), lv, calls)
    assert len(got) == 4
    for name in want:
        assert np.array_equal(got[name], want[name]), name


# ---------------------------------------------------------------------------
# the constants' cache
# ---------------------------------------------------------------------------
def test_cache_key_holds_the_gap(gpu):
    """Root q_0..q_3, p_0, p_1.  The prefix form -- key basis drop_last(1) =
    q_0..q_3, p_0 with a ciphertext of 3 limbs, so that q_3 and p_0 are its
    special primes -- and the level-3 view q_0..q_2, p_0, p_1 are both (LE, Lv,
    alpha) = (5, 3, 2) on the same tables, with different special primes.  Run
    alternately, each must keep matching its own yardstick."""
    rn = gpu
    n, alpha, B = 256, 2, 2
    emod = rn.generate_primes(31, 6, n)
    q, p = emod[:4], emod[4:]
    ext = rn.RnsBasis(emod, n)
    rng = np.random.default_rng(9901)
    c0, c1 = _rand(rng, q[:3], n, B), _rand(rng, q[:3], n, B)
    cb = ext.drop_last(3)
    ct = rn.Ciphertext(rn.RnsPoly.from_channels(c0, cb), rn.RnsPoly.from_channels(c1, cb))
    # the view form: a full key (beta = 2) at level 3
    ka, kb = _rand(rng, emod, n, 2), _rand(rng, emod, n, 2)
    full = rn.RnsHybridKey.from_channels(ka, kb, ext, alpha, rotation=STEP, n_special=2)
    view = full.at_level(3)
    v_mod = q[:3] + p
    va, vb = restrict_key(ka, 4, alpha, 3), restrict_key(kb, 4, alpha, 3)
    # the prefix form: a key of 2 polys on q_0..q_3, p_0, read with Lv = 3
    pref = ext.drop_last(1)
    p_mod = emod[:5]
    pa, pb = _rand(rng, p_mod, n, 2), _rand(rng, p_mod, n, 2)
    pkey = rn.RnsHybridKey.from_channels(pa, pb, pref, alpha, rotation=STEP)
    Bc = orc.Basis(q[:3], n)
    refs = {}
    for name, mod, a_, b_ in (("view", v_mod, va, vb), ("prefix", p_mod, pa, pb)):
        refs[name] = [rotate_hybrid_ref(Bc, orc.Basis(mod, n), c0[i], c1[i], STEP, a_, b_, alpha) for i in range(B)]
    assert not np.array_equal(refs["view"][0][1], refs["prefix"][0][1])
    for name, key in (("prefix", pkey), ("view", view), ("prefix", pkey), ("view", view)):
        out = rn.rotate_ciphertext_hybrid(ct, key)
        for i in range(B):
            assert np.array_equal(out.c0.channels_of(i)[0], refs[name][i][0]), (name, i)
            assert np.array_equal(out.c1.channels_of(i)[0], refs[name][i][1]), (name, i)


# ---------------------------------------------------------------------------
# launch counts
# ---------------------------------------------------------------------------
def _counts(basis, run):
    run()  # warm: workspaces and constants cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in KERNELS}
    basis.profile_enable(False)
    return counts


@pytest.mark.parametrize("log_n", [8, 12, 16])
def test_launch_counts(gpu, log_n):
    """At level == L a view gives the key's own outputs with the same launches
    of every kernel.  Below (gap > 0) the transforms over the key basis run
    once per contiguous run of root limbs, two launches instead of one, and
    nothing else changes.  rotate_ciphertext_hybrid, one chunk: a forward
    transform of D and an inverse of A0 and of A1 over the key basis -- with
    the four-step kernels (2^8) col_fwd, row_fwd 1 -> 2 and row_inv, col_inv
    2 -> 4; with the whole-plane (2^12) and matrix-core (2^16) transforms the
    forward kernel 1 -> 2 and the inverse 2 -> 4."""
    rn = gpu
    r = Ring(rn, log_n, 4, 2, 2, 2, 31, seed=4)
    basis, (view, _, _, _) = r.view_side(4)
    ct, _, _ = r.operands(basis, 4)
    direct = rn.rotate_ciphertext_hybrid(ct, rn.RnsHybridKey.from_channels(*r.key_ch, r.ext, 2, rotation=STEP))
    top = rn.rotate_ciphertext_hybrid(ct, view)
    assert np.array_equal(top.c0.channels_batch(), direct.c0.channels_batch())
    assert np.array_equal(top.c1.channels_batch(), direct.c1.channels_batch())
    plain = rn.RnsHybridKey.from_channels(*r.key_ch, r.ext, 2, rotation=STEP)
    assert _counts(basis, lambda: rn.rotate_ciphertext_hybrid(ct, view)) == \
        _counts(basis, lambda: rn.rotate_ciphertext_hybrid(ct, plain))
    lv = 3
    vb, (v3, _, _, _) = r.view_side(lv)
    rb, (k3, _, _, _) = r.restricted_side(lv)
    cv, _, _ = r.operands(vb, lv)
    cr, _, _ = r.operands(rb, lv)
    got = _counts(vb, lambda: rn.rotate_ciphertext_hybrid(cv, v3))
    want = _counts(rb, lambda: rn.rotate_ciphertext_hybrid(cr, k3))
    for k in KERNELS:
        if k not in TRANSFORMS:
            assert got[k] == want[k], (k, got, want)
    fwd, inv = {8: (("col_fwd", "row_fwd"), ("row_inv", "col_inv")), 12: (("whole_fwd",), ("whole_inv",)),
                16: (("mf_ntt_fwd",), ("mf_ntt_inv",))}[log_n]
    for k in TRANSFORMS:
        exp_r = 1 if k in fwd else 2 if k in inv else 0
        assert (want[k], got[k]) == (exp_r, 2 * exp_r), (k, got, want)
    assert (got["modup"], got["hoist_mac"], got["moddown"]) == (1, 1, 2)


# ---------------------------------------------------------------------------
# capture
# ---------------------------------------------------------------------------
def test_capture_with_a_view(gpu):
    """One plain run (constants and workspaces), then the multiply + rescale
    with a view recorded and replayed on other inputs."""
    rn = gpu
    r = Ring(rn, 8, 4, 2, 2, 2, 31, seed=5)
    lv = 3
    basis, (key, _, _, _) = r.view_side(lv)
    ct, ctp, _ = r.operands(basis, lv)
    lib = rn.load()
    low = basis.drop_last(1)
    o0, o1 = rn.RnsPoly(low, r.B), rn.RnsPoly(low, r.B)

    def call():
        rn.check(lib.rnt_ct_mul_relin_rescale_hybrid(o0.handle, o1.handle, ct.c0.handle, ct.c1.handle, ctp.c0.handle,
                                                     ctp.c1.handle, key.a.handle, key.b.handle, key.alpha))

    call()
    want0, want1 = o0.channels_batch(), o1.channels_batch()
    with basis.capture() as g:
        call()
    zero = rn.RnsPoly(low, r.B)
    o0.copy_polys(zero)
    o1.copy_polys(zero)
    g.replay()
    basis.sync()
    assert np.array_equal(o0.channels_batch(), want0) and np.array_equal(o1.channels_batch(), want1)
    assert want0.any()


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
def _status(rn, rc):
    with pytest.raises(rn.RnsNttError) as e:
        rn.check(rc)
    return e.value.code


def test_level_context_errors(gpu):
    rn, lib, S = gpu, gpu.load(), gpu._lib
    n = 256
    ext = rn.RnsBasis(rn.generate_primes(31, 6, n), n)
    h = ctypes.c_void_p()
    mk = lambda ctx, ns, lv, out=None: lib.rnt_ctx_hybrid_level(ctx, ns, lv, ctypes.byref(h) if out is None else out)  # noqa: E731
    assert _status(rn, mk(None, 2, 1)) == S.BAD_ARGUMENT
    assert _status(rn, mk(ext.handle, 2, 1, out=ctypes.cast(None, ctypes.POINTER(ctypes.c_void_p)))) == S.BAD_ARGUMENT
    assert _status(rn, mk(ext.handle, 0, 1)) == S.BAD_ARGUMENT
    assert _status(rn, mk(ext.handle, 6, 1)) == S.BAD_ARGUMENT
    assert _status(rn, mk(ext.handle, 2, 0)) == S.BAD_ARGUMENT
    assert _status(rn, mk(ext.handle, 2, 5)) == S.BAD_ARGUMENT
    lb = ext.hybrid_level(2, 3)
    assert _status(rn, mk(lb.handle, 2, 1)) == S.BAD_ARGUMENT  # a level context of a level context
    b = ctypes.c_void_p()
    for rc in (lib.rnt_ctx_drop_last(lb.handle, 1, ctypes.byref(h)), lib.rnt_buf_alloc(lb.handle, 1, ctypes.byref(b)),
               lib.rnt_buf_alloc_uninit(lb.handle, 1, ctypes.byref(b)),
               lib.rnt_buf_wrap(lb.handle, ctypes.c_void_p(4096), 1, 0, ctypes.byref(b))):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(rc)
        assert e.value.code == S.UNSUPPORTED and (e.value.degree, e.value.max_degree) == (0, 0)
    # a level-L context is a level context too (gap 0)
    assert _status(rn, lib.rnt_buf_alloc(ext.hybrid_level(2, 4).handle, 1, ctypes.byref(b))) == S.UNSUPPORTED


def test_key_view_errors(gpu):
    rn, lib, S = gpu, gpu.load(), gpu._lib
    r = Ring(rn, 8, 4, 2, 2, 2, 31, seed=6)
    lb = r.ext.hybrid_level(2, 3)
    h = ctypes.c_void_p()
    view = lambda key, ctx, alpha: lib.rnt_key_level_view(key, ctx, alpha, ctypes.byref(h))  # noqa: E731
    ka = r.key.a
    assert _status(rn, view(None, lb.handle, 2)) == S.BAD_ARGUMENT
    assert _status(rn, view(ka.handle, None, 2)) == S.BAD_ARGUMENT
    assert _status(rn, view(ka.handle, lb.handle, 0)) == S.BAD_ARGUMENT
    assert _status(rn, view(ka.handle, r.ext.handle, 2)) == S.BAD_ARGUMENT  # not a level context
    other = rn.RnsBasis(r.emod, r.n)
    assert _status(rn, view(ka.handle, other.hybrid_level(2, 3).handle, 2)) == S.BASIS_MISMATCH
    coeff = rn.RnsPoly.from_channels(r.key_ch[0], r.ext)
    assert _status(rn, view(coeff.handle, lb.handle, 2)) == S.DOMAIN_MISMATCH
    three = rn.RnsPoly(r.ext, 3)
    three.to_ntt_domain()
    with pytest.raises(rn.RnsNttError) as e:
        rn.check(view(three.handle, lb.handle, 2))  # beta = 2
    assert e.value.code == S.CHANNEL_COUNT and (e.value.expected, e.value.actual) == (2, 3)
    v = r.key.at_level(3)
    assert _status(rn, view(v.a.handle, lb.handle, 2)) == S.BAD_ARGUMENT  # a view of a view
    # a view anywhere but a key position: refused, nothing touched
    basis, _ = r.view_side(3)
    ct, _, _ = r.operands(basis, 3)
    o0, o1 = ct.c0.clone(), ct.c1.clone()
    keep0, keep1 = o0.channels_batch(), o1.channels_batch()
    for rc in (lib.rnt_keyswitch_hybrid(o0.handle, o1.handle, v.a.handle, v.a.handle, v.b.handle, 2),   # as d
               lib.rnt_keyswitch_hybrid(v.a.handle, o1.handle, ct.c1.handle, v.a.handle, v.b.handle, 2),  # as an output
               lib.rnt_add(o0.handle, v.a.handle, o1.handle), lib.rnt_add(o0.handle, o1.handle, v.a.handle),
               lib.rnt_add(v.a.handle, o0.handle, o1.handle)):
        assert _status(rn, rc) == S.UNSUPPORTED
    assert np.array_equal(o0.channels_batch(), keep0) and np.array_equal(o1.channels_batch(), keep1)
    assert np.array_equal(v.a._view_of.channels_batch(), r.key.a.channels_batch())
    # the halves on two distinct handles of the same level
    lb2 = ctypes.c_void_p()
    rn.check(lib.rnt_ctx_hybrid_level(r.ext.handle, 2, 3, ctypes.byref(lb2)))
    rn.check(view(r.key.b.handle, lb2, 2))
    try:
        assert _status(rn, lib.rnt_keyswitch_hybrid(o0.handle, o1.handle, ct.c1.handle, v.a.handle, h, 2)) == \
            S.BASIS_MISMATCH
    finally:
        lib.rnt_buf_free(h)
        lib.rnt_ctx_destroy(lb2)
    assert np.array_equal(o0.channels_batch(), keep0)


# ---------------------------------------------------------------------------
# engine, end to end
# ---------------------------------------------------------------------------
# tools/hybrid_levels_tolerance.py, eight seeds, the same ring, parameters and
# circuit on the CPU (oracle/pyoracle, oracle/encoder.py, tests/hybrid_ref.py
# with restrict_key'd keys): the largest decode error.  The tolerance is 4 x
# this, the margin of test_gpu_hybrid.py's end-to-end test: 1.61e-4.
CIRCUIT_ERR_MEASURED = 4.026e-5


def test_engine_levels_end_to_end(gpu):
    """test_engine_hybrid_end_to_end's ring: N = 2^10, 4 x 31-bit + 2 special
    primes, alpha = 2, scale 2^30, a DeviceRng.  rot_1(((x y) rescaled w)
    rescaled) with ONE relinearisation key and ONE rotation key and no restrict
    call: the wrappers take the keys' views at levels 3 and 2.  Word for word
    the circuit with restricted keys, and the slots of roll(x y w, -1)."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L, K, alpha, logp = 1024, 512, 4, 2, 2, 30
    q, c = [], (1 << 30) + 1
    while len(q) < L:
        if rn.is_ntt_friendly_prime(c, n):
            q.append(c)
        c += 2 * n
    p = rn.generate_primes(31, K, n)
    eng = CkksEngine(q, n, error_std=3.2, hamming_weight=n // 2, special_moduli=p)
    rng = rn.DeviceRng(91)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    host = np.random.default_rng(92)
    x, y, w = (host.uniform(-1, 1, slots) for _ in range(3))
    enc = rn.CkksEncoder(n, logp)
    cx, cy, cw = (eng.encrypt(enc.encode(v, eng.basis), pk, rng) for v in (x, y, w))
    rlk = eng.generate_hybrid_relin_key(sk, rng, alpha)
    rotk = eng.generate_hybrid_rotation_key(sk, 1, rng, alpha)
    assert rlk.n_special == K and rotk.n_special == K

    def circuit(key_at):
        t = CkksEngine.mul_ciphertexts_hybrid_rescale(cx, cy, key_at(rlk, 4))
        b3 = t.c0.basis
        assert b3.channel_count() == 3
        w3 = rn.Ciphertext(cw.c0.mod_drop_last(1), cw.c1.mod_drop_last(1), cw.logp, t.logq)
        w3 = rn.Ciphertext(_on(rn, w3.c0, b3), _on(rn, w3.c1, b3), cw.logp, t.logq)
        t = CkksEngine.mul_ciphertexts_hybrid_rescale(t, w3, key_at(rlk, 3))
        assert t.c0.basis.channel_count() == 2
        return CkksEngine.rotate_ciphertext_hybrid(t, key_at(rotk, 2))

    got = circuit(lambda key, lv: key)  # the engine's keys as they are
    roots = {lv: rn.RnsBasis(q[:lv] + p, n) for lv in (3, 2)}
    want = circuit(lambda key, lv: key if lv == 4 else key.restrict(roots[lv]))
    assert np.array_equal(got.c0.channels(), want.c0.channels())
    assert np.array_equal(got.c1.channels(), want.c1.channels())
    dec = enc.decode(rn.Plaintext(CkksEngine.decrypt(got, CkksEngine.secret_on(sk, got.c0.basis)), logp, slots))
    err = float(np.max(np.abs(dec - np.roll(x * y * w, -1) * (2.0 ** (2 * logp) / (q[3] * q[2])))))
    print(f"rot_1(((x y) rescaled w) rescaled): decode error {err:.3e}")
    assert err <= 4 * CIRCUIT_ERR_MEASURED


def _on(rn, poly, basis):
    """`poly` (coefficient domain) on `basis`, a context with the same moduli."""
    assert poly.basis.moduli() == basis.moduli()
    return rn.RnsPoly.from_channels(poly.channels_batch() if poly.batched else poly.channels(), basis)
