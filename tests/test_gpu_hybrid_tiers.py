"""Every register tier of the four element-wise kernels of the hybrid
key-switch (k_modup, k_moddown, k_moddown_auto, k_moddown_rescale), the last,
partly empty run of their split grids, the scalar forms of the higher tiers,
alpha above the level, and one key basis serving several plans.

The launchers (modup_t, moddown_t, moddown_auto_t, moddown_rescale_t in
rnt_kernels.hip) choose a template instantiation from alpha (k_modup, clamped
to Lv) or K (the three ModDowns): AMAX / KMAX = 4, 8, 16 keep the y_i / z_k in
registers, 0 is the generic form that recomputes them per target limb
(k_moddown_auto has no 16 tier).  The tier matrix runs N = 2^8, B = 2,
Lv = alpha + 1 (a full digit and a one-limb last digit: the unrolled tiers'
`a < cnt` guard with cnt = alpha and cnt = 1), at 31 bits (u32 kernels) and at
61 bits (u64 kernels); every buffer is 16-byte aligned, so these rows take the
16-byte (VEC) forms:

    (alpha, K)  k_modup   k_moddown   k_moddown_rescale   k_moddown_auto
    ( 4,  4)    AMAX 4    KMAX 4      KMAX 4              KMAX 4     upper edge
    ( 5,  5)    AMAX 8    KMAX 8      KMAX 8              KMAX 8     lower edge (+ an edge-values row)
    ( 8,  8)    AMAX 8    KMAX 8      KMAX 8              KMAX 8     upper edge
    ( 9,  9)    AMAX 16   KMAX 16     KMAX 16             KMAX 0     lower edge
    (16, 16)    AMAX 16   KMAX 16     KMAX 16             KMAX 0     upper edge
    (17, 17)    AMAX 0    KMAX 0      KMAX 0              KMAX 0     generic (+ an edge-values row)

    test                          kernels it runs at the row's tier
    test_tier_three_calls         k_modup, k_moddown (keyswitch, rotation, multiply + relin)
    test_tier_hoisted_rotation    k_modup, k_moddown_auto (asserted by the launch counts)
    test_tier_hoisted_unfused     k_modup, k_moddown + the automorphism (RNT_MODDOWN_AUTO=0)
    test_tier_bsgs                k_modup, k_moddown_auto (baby steps), k_moddown (the two sums)
    test_tier_mul_rescale         k_modup, k_hoist_mac_seed, k_moddown_rescale; k_moddown (composition)
    test_tier_bsgs_rescale        k_modup, k_moddown_auto, k_moddown_rescale; k_moddown (composition)
    test_tier_plain_key_identity  k_modup, k_moddown, without the yardstick

So each of the 4 tiers x {u32, u64} of k_modup, k_moddown and
k_moddown_rescale and each of the 3 tiers x {u32, u64} of k_moddown_auto runs
at both of its edges.  The scalar (one-word, VEC = false) forms run in
test_tier_unaligned: k_modup and k_moddown at AMAX / KMAX 8 and 0 for u32 and
at 8 for u64 (the 4-limb tier's are in test_gpu_hybrid.test_unaligned_planes).

All of it is exact integer arithmetic with canonical outputs: every assertion
is equality of words with the CPU yardsticks (tests/hybrid_ref.py,
hybrid_hoist_ref.py, hybrid_rescale_ref.py; pinned at these tiers by
tests/test_hybrid_ref.py), with the device composition, or with the input.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from hybrid_ref import hybrid_key_plain, keyswitch_hybrid_ref, n_digits, rotate_hybrid_ref
from test_gpu_hybrid import STEP, Case, _rand
from test_gpu_hybrid_hoist import BsgsCase, _check_rotations, _counts
from test_gpu_hybrid_hoist import Case as HoistCase
from test_gpu_hybrid_rescale import _counts as _rescale_counts
from test_gpu_hybrid_rescale import check_bsgs_rescale, check_mul

pytestmark = pytest.mark.gpu

LOG_N, B = 8, 2
TIERS = [(4, 4), (5, 5), (8, 8), (9, 9), (16, 16), (17, 17)]
# alpha, K, bits, edge (an all-(q-1) ciphertext and all-(m-1) keys)
MATRIX = [(a, k, bits, False) for a, k in TIERS for bits in (31, 61)]
MATRIX += [(a, k, bits, True) for a, k in ((5, 5), (17, 17)) for bits in (31, 61)]
STEPS = [0, 1, -3]


def _row_id(row):
    a, k, bits, edge = row
    return f"a{a}-K{k}-u{32 if bits == 31 else 64}" + ("-edge" if edge else "")


tier_matrix = pytest.mark.parametrize("alpha,K,bits,edge", MATRIX, ids=[_row_id(r) for r in MATRIX])


# ---------------------------------------------------------------------------
# a. the tier matrix
# ---------------------------------------------------------------------------
@tier_matrix
def test_tier_three_calls(gpu, alpha, K, bits, edge):
    Case(gpu, LOG_N, alpha + 1, K, alpha, B, bits, edge=edge, seed=alpha).check_all()


def _hoisted(gpu, alpha, K, bits, edge, fused, log_n=LOG_N, Lv=None, batch=B):
    """The hoisted rotation by STEPS against the yardstick; the launch counts
    say which tail ran (two nonzero steps, two components)."""
    c = HoistCase(gpu, log_n, alpha + 1 if Lv is None else Lv, K, alpha, batch, bits, steps=STEPS, edge=edge,
                  seed=alpha)
    out = c.run()
    _check_rotations(c, out.c0.channels(), out.c1.channels())
    counts = _counts(c.basis, c.run)
    assert counts["modup"] == 1, counts  # one chunk
    assert (counts["moddown_auto"], counts["moddown"]) == ((4, 0) if fused else (0, 4)), counts


@tier_matrix
def test_tier_hoisted_rotation(gpu, alpha, K, bits, edge):
    """The default tail: k_moddown_auto below 16 MiB a component."""
    _hoisted(gpu, alpha, K, bits, edge, fused=True)


@tier_matrix
def test_tier_hoisted_unfused(gpu, monkeypatch, alpha, K, bits, edge):
    monkeypatch.setenv("RNT_MODDOWN_AUTO", "0")  # read at rnt_ctx_create
    _hoisted(gpu, alpha, K, bits, edge, fused=False)


@tier_matrix
def test_tier_bsgs(gpu, alpha, K, bits, edge):
    c = BsgsCase(gpu, LOG_N, alpha + 1, K, alpha, B, bits, edge=edge, seed=alpha)
    out = c.run()
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    g0, g1 = out.c0.channels(), out.c1.channels()
    for p in sorted({0, B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0), f"out0 of ciphertext {p} differs from bsgs_hybrid_ref"
        assert np.array_equal(g1[p], r1), f"out1 of ciphertext {p} differs from bsgs_hybrid_ref"


@tier_matrix
def test_tier_mul_rescale(gpu, alpha, K, bits, edge):
    c = Case(gpu, LOG_N, alpha + 1, K, alpha, B, bits, edge=edge, seed=alpha)
    check_mul(c)
    counts = _rescale_counts(c.basis, lambda: gpu.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key))
    assert (counts["moddown_rescale"], counts["moddown"], counts["modup"]) == (2, 0, 1), counts


@tier_matrix
def test_tier_bsgs_rescale(gpu, alpha, K, bits, edge):
    """Baby steps with a zero, giants [0, 2]: the addend of the step-0 giant and
    one key-switched giant in front of the two k_moddown_rescale launches."""
    c = BsgsCase(gpu, LOG_N, alpha + 1, K, alpha, B, bits, baby=STEPS, giant=[0, 2], edge=edge, seed=alpha)
    check_bsgs_rescale(c, polys=sorted({0, B - 1}))
    counts = _rescale_counts(c.basis, lambda: gpu.linear_transform_bsgs_hybrid_rescale(c.ct, c.d, c.bset, c.gset))
    assert (counts["moddown_rescale"], counts["moddown"]) == (2, 0), counts


# ---------------------------------------------------------------------------
# e. an identity that needs no yardstick
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,K,bits", [r[:3] for r in MATRIX if not r[3]],
                         ids=[_row_id(r) for r in MATRIX if not r[3]])
def test_tier_plain_key_identity(gpu, alpha, K, bits):
    """key_b = the plaintexts G_d of the target 1 -- limb t of G_d is [P]_{q_t}
    on the digit's own limbs and zero elsewhere -- and key_a = 0.  Then A0 =
    P x on the ciphertext limbs and 0 on the special ones, so z = 0 and
    ModDown gives (P x_t) P^-1 = x_t: rnt_keyswitch_hybrid returns (x, 0) word
    for word, for a random x (poly 0) and the all-(q - 1) one (poly 1).  This
    pins k_modup's one-hot rows and k_moddown's P^-1 constants at every tier
    without hybrid_ref.py's conversions (tests/test_hybrid_ref.py states the
    same identity of the yardstick)."""
    rn, n, Lv = gpu, 1 << LOG_N, alpha + 1
    emod = rn.generate_primes(bits, Lv + K, n)
    mod = emod[:Lv]
    one = np.zeros((Lv, n), dtype=np.uint64)
    one[:, 0] = 1
    kb = hybrid_key_plain(emod, Lv, alpha, one)
    ext = rn.RnsBasis(emod, n)
    key = rn.RnsHybridKey.from_channels(np.zeros_like(kb), kb, ext, alpha)
    x = _rand(np.random.default_rng(7700 + alpha + bits), mod, n, 2)
    x[1] = np.broadcast_to(np.array(mod, dtype=np.uint64)[:, None] - np.uint64(1), (Lv, n))
    a0, a1 = rn.keyswitch_hybrid(rn.RnsPoly.from_channels(x, ext.drop_last(K)), key)
    assert np.array_equal(a0.channels(), x), "acc0 is not the input"
    assert not a1.channels().any(), "acc1 is not zero"


# ---------------------------------------------------------------------------
# b. split grids whose last run is partly past the end
#
# N = 2^14, 31-bit words, every buffer aligned: a lane takes V = 4 words, so a
# chunk of B polys is bx = ceil(B N / 4 / 256) = 16 B workgroups along x, and
# the default workspace holds the whole batch in one chunk (asserted: one
# ModUp launch per call), so the launchers see k.B = B.
# ---------------------------------------------------------------------------
def _one_chunk_rotation(gpu, c):
    counts = _counts(c.basis, lambda: gpu.rotate_ciphertext_hybrid(c.ct, c.key))
    assert counts["modup"] == 1 and counts["hoist_mac"] == 1 and counts["moddown"] == 2, counts


def test_ragged_last_run_modup(gpu):
    """modup_t, Lv = 3, K = 2 (LE = 5), alpha = 2 (beta = 2), B = 16: bx = 256,
    runs = min(LE, max(1024 / (bx beta), 1)) = min(5, 2) = 2, tper = ceil(5 / 2)
    = 3, grid.z = ceil(5 / 3) = 2: target limbs {0, 1, 2} and {3, 4}; the second
    run's t0 + tper = 6 is clamped to LE = 5.  (moddown_t at this B: bx = 256,
    runs = min(3, 4) = 3, jper = 1, no ragged run.)"""
    c = Case(gpu, 14, 3, 2, 2, 16, 31, seed=11)
    c.check_all()
    _one_chunk_rotation(gpu, c)


def test_ragged_last_run_moddown(gpu):
    """moddown_t, Lv = 3, K = 2, alpha = 2, B = 24: bx = 384, runs = min(Lv,
    max(1024 / 384, 1)) = min(3, 2) = 2, jper = ceil(3 / 2) = 2, grid.y = 2:
    output limbs {0, 1} and {2}; the second run's j0 + jper = 4 is clamped to
    Lv = 3.  (modup_t at this B: 1024 / (384 x 2) = 1 run, un-split.)"""
    c = Case(gpu, 14, 3, 2, 2, 24, 31, seed=12)
    c.check_all()
    _one_chunk_rotation(gpu, c)


@pytest.mark.parametrize("fused", [True, False], ids=["moddown_auto", "unfused"])
def test_ragged_last_run_hoisted_tails(gpu, monkeypatch, fused):
    """moddown_auto_t at the same shape: bx = (384 + 7) & ~7 = 384, so the same
    2 runs {0, 1} and {2} (a component is 24 x 3 x 64 KiB = 4.5 MiB, below the
    16 MiB from which the default tail is the un-fused one); with
    RNT_MODDOWN_AUTO=0 the tail is k_moddown on the chunk's 24 polys, the grid
    of test_ragged_last_run_moddown, followed by the automorphism."""
    if not fused:
        monkeypatch.setenv("RNT_MODDOWN_AUTO", "0")
    _hoisted(gpu, 2, 2, 31, False, fused, log_n=14, Lv=3, batch=24)


def test_ragged_last_run_moddown_rescale(gpu):
    """moddown_rescale_t, Lv = 4, K = 2, alpha = 2, B = 24: the runs are over the
    lo = Lv - 1 = 3 output limbs, bx = 384, runs = min(3, 2) = 2, jper = 2,
    grid.y = 2: {0, 1} and {2}; the second run's j0 + jper = 4 is clamped to
    lo = 3.  check_mul compares every poly with the device composition (whose
    k_moddown, Lv = 4: runs = 2, jper = 2, divides exactly) and polys {0, 23}
    with the yardstick."""
    c = Case(gpu, 14, 4, 2, 2, 24, 31, seed=13)
    check_mul(c)
    counts = _rescale_counts(c.basis, lambda: gpu.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key))
    assert (counts["moddown_rescale"], counts["moddown"], counts["modup"]) == (2, 0, 1), counts


# ---------------------------------------------------------------------------
# c. the scalar instantiations of the higher tiers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,K,bits", [(5, 5, 31), (17, 17, 31), (5, 5, 61)],
                         ids=["a5-K5-u32", "a17-K17-u32", "a5-K5-u64"])
def test_tier_unaligned(gpu, alpha, K, bits):
    """Inputs and outputs wrapped one word off 16-byte alignment (+4 bytes for
    u32 words, +8 for u64: 8- but not 16-byte aligned planes), so k_modup and
    k_moddown take their one-word forms at the 8-limb tier and in the generic
    form: the words of the aligned calls, and the yardstick's on poly 1."""
    import torch

    c = Case(gpu, LOG_N, alpha + 1, K, alpha, 3, bits, seed=20 + alpha)
    rn, lib, Bd = c.rn, c.rn.load(), c.basis
    dev = torch.device("cuda", Bd.device)
    wb = 4 if bits == 31 else 8
    assert c.ct.c0.device_ptr()[1] == wb

    def shifted(src=None):
        words = c.B * c.Lv * c.n
        t = torch.zeros(words + 16 // wb, dtype=torch.int32 if wb == 4 else torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(Bd, t.data_ptr() + wb, c.B, owner=t)
        assert v.device_ptr()[0] % 16 == wb
        if src is not None:
            v.copy_polys(src)
        return v

    w0, w1 = rn.keyswitch_hybrid(c.ct.c1, c.key)
    g0, g1 = shifted(), shifted()
    s0, s1 = shifted(c.ct.c0), shifted(c.ct.c1)
    rn.check(lib.rnt_keyswitch_hybrid(g0.handle, g1.handle, s1.handle, c.key.a.handle, c.key.b.handle, c.alpha))
    assert np.array_equal(g0.channels(), w0.channels()) and np.array_equal(g1.channels(), w1.channels())
    r0, r1 = keyswitch_hybrid_ref(c.Be, c.Lv, c.c1[1], c.ka, c.kb, c.alpha)
    assert np.array_equal(g0.channels_of(1)[0], r0) and np.array_equal(g1.channels_of(1)[0], r1)
    want = rn.rotate_ciphertext_hybrid(c.ct, c.key)
    rn.check(lib.rnt_ct_rotate_hybrid(g0.handle, g1.handle, s0.handle, s1.handle, STEP, c.key.a.handle,
                                      c.key.b.handle, c.alpha))
    assert np.array_equal(g0.channels(), want.c0.channels()) and np.array_equal(g1.channels(), want.c1.channels())
    r0, r1 = rotate_hybrid_ref(c.Bc, c.Be, c.c0[1], c.c1[1], STEP, c.ka, c.kb, c.alpha)
    assert np.array_equal(g0.channels_of(1)[0], r0) and np.array_equal(g1.channels_of(1)[0], r1)


# ---------------------------------------------------------------------------
# d. alpha above the level; one key basis serving several plans
# ---------------------------------------------------------------------------
def test_alpha_above_the_level(gpu):
    """Lv = 3, K = 2, alpha = 5 with a key of beta = ceil(3 / 5) = 1 poly: the
    library clamps alpha to Lv (one digit of every limb), which is what the
    yardstick's digit_limbs(3, 5, 0) = [0, 3) says, and what a key restricted to
    a low level looks like.  The Python wrappers pass alpha through.  Every
    family, and the words of the same channels declared as alpha = 3."""
    rn = gpu
    c = Case(rn, LOG_N, 3, 2, 5, B, 31, seed=30)
    assert c.beta == 1 and c.key.a.n_polys == 1
    c.check_all()
    check_mul(c)
    _hoisted(rn, 5, 2, 31, False, fused=True, Lv=3)
    b = BsgsCase(rn, LOG_N, 3, 2, 5, B, 31, seed=30)
    o = b.run()
    r0, r1 = b.reference(1)
    assert np.array_equal(o.c0.channels_of(1)[0], r0) and np.array_equal(o.c1.channels_of(1)[0], r1)
    key3 = rn.RnsHybridKey.from_channels(c.ka, c.kb, c.ext, 3, rotation=STEP)
    for a, w in zip(rn.keyswitch_hybrid(c.ct.c1, c.key), rn.keyswitch_hybrid(c.ct.c1, key3)):
        assert np.array_equal(a.channels(), w.channels())


@pytest.mark.parametrize("bits", [31, 61])
def test_two_alphas_on_one_key_basis(gpu, bits):
    """One key basis (Lv = 6, K = 5), one ciphertext, keys of alpha = 2 (three
    digits, the 4-limb tier of k_modup) and alpha = 5 (two digits, the 8-limb
    tier) called in the order 2, 5, 2, 5: hybrid_prepare's cache on the basis
    holds a constants block per (key limbs, Lv, alpha), and each call must get
    its own whichever was built or used last."""
    rn = gpu
    c = Case(rn, LOG_N, 6, 5, 2, B, bits, seed=31)
    rng = np.random.default_rng(7731)
    ka5, kb5 = _rand(rng, c.emod, c.n, n_digits(6, 5)), _rand(rng, c.emod, c.n, n_digits(6, 5))
    key5 = rn.RnsHybridKey.from_channels(ka5, kb5, c.ext, 5)
    plans = {2: (c.key, c.ka, c.kb), 5: (key5, ka5, kb5)}
    want = {a: [keyswitch_hybrid_ref(c.Be, c.Lv, c.c1[p], ka, kb, a) for p in range(B)]
            for a, (_, ka, kb) in plans.items()}
    for turn, a in enumerate((2, 5, 2, 5)):
        a0, a1 = rn.keyswitch_hybrid(c.ct.c1, plans[a][0])
        for p in range(B):
            assert np.array_equal(a0.channels_of(p)[0], want[a][p][0]), f"call {turn} (alpha {a}): acc0, poly {p}"
            assert np.array_equal(a1.channels_of(p)[0], want[a][p][1]), f"call {turn} (alpha {a}): acc1, poly {p}"


@pytest.mark.parametrize("bits", [31, 61])
def test_two_levels_on_one_key_basis(gpu, bits):
    """One five-limb key basis m_0..m_4 under a ciphertext on drop_last(2)
    (Lv = 3, K = 2: m_3, m_4 are the special primes; two digits of alpha = 2)
    and one on drop_last(3) (Lv = 2, K = 3: m_2 is a special prime now; one
    digit), alternated.  Each against the yardstick over the same five moduli
    with its own Lv."""
    rn, n, alpha = gpu, 1 << LOG_N, 2
    emod = rn.generate_primes(bits, 5, n)
    ext, Be = rn.RnsBasis(emod, n), orc.Basis(emod, n)
    rng = np.random.default_rng(7732 + bits)
    plans = {}
    for Lv in (3, 2):
        beta = n_digits(Lv, alpha)
        x = _rand(rng, emod[:Lv], n, B)
        ka, kb = _rand(rng, emod, n, beta), _rand(rng, emod, n, beta)
        d = rn.RnsPoly.from_channels(x, ext.drop_last(5 - Lv))
        key = rn.RnsHybridKey.from_channels(ka, kb, ext, alpha)
        want = [keyswitch_hybrid_ref(Be, Lv, x[p], ka, kb, alpha) for p in range(B)]
        plans[Lv] = (d, key, want)
    for turn, Lv in enumerate((3, 2, 3, 2)):
        d, key, want = plans[Lv]
        a0, a1 = rn.keyswitch_hybrid(d, key)
        assert a0.basis.channel_count() == Lv
        for p in range(B):
            assert np.array_equal(a0.channels_of(p)[0], want[p][0]), f"call {turn} (Lv {Lv}): acc0, poly {p}"
            assert np.array_equal(a1.channels_of(p)[0], want[p][1]), f"call {turn} (Lv {Lv}): acc1, poly {p}"
