"""The ciphertext x plaintext multiply-accumulate on the GPU (rnt_ct_plain_mac,
rnt_ct_plain_mac_rescale): the terms are transformed forward in groups of
kPlainT, k_plain_mac sums them against the NTT-domain plaintexts where they lie,
and two inverse transforms close the call whatever n_terms is.  Exact
arithmetic with canonical outputs, so both calls must give, on every poly, the
words of the device composition of existing ops (RnsPoly products of each term
with the plaintext taken back to coefficients, sums over the terms and the
bias, rescale_ciphertext) and, on polys {0, B - 1}, those of the CPU model
(tests/plain_mac_ref.py, pinned in tests/test_plain_mac_ref.py).

END-TO-END TOLERANCE: tools/plain_mac_tolerance.py, eight seeds of the CPU model
on the evaluator tests' ring (N = 2^10, 7 primes of 30 bits, scale 2^30, 8
terms, a bias, every value uniform in (-1, 1)), largest decode error at the
nominal scale against numpy's sum_i w_i a_i + b: profiles/plain_mac_tolerance.txt
(3.255e-04, mostly the scale drift of q_last != 2^30 on a sum of up to 9).  The
tests allow 4 x that (1.302e-03), the project's standing margin for seed spread.
Measured on the device: 2.478e-04 (plain_mac, 8 terms and a bias), 8.153e-05
(mul_plaintext), 9.444e-06 (add_plaintext), 1.685e-04 (four hoisted rotations,
then plain_mac with four diagonals).
"""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import encoder as cpu_encoder
import pyoracle as orc
from hybrid_ref import crt_centered
from plain_mac_ref import pick_plain, pick_terms, plain_mac_ref
from test_gpu_hybrid import _rand

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPLAIN_T = 16  # rnt_internal.hpp: the terms one k_plain_mac launch sums


def _tolerance():
    """4 x the figure tools/plain_mac_tolerance.py wrote."""
    line = open(os.path.join(REPO, "profiles", "plain_mac_tolerance.txt")).read()
    return 4 * float(re.search(r"seeds ([0-9.e+-]+);", line).group(1))


class MacCase:
    """n_terms packed ciphertexts of B over q_0..q_{Lv-1} (term i of ciphertext b
    at poly i B + b), NTT-domain plaintexts (n_terms of them with `shared`, else
    n_terms B) and a bias (None, "shared": 1 poly, "each": B polys).  edge: every
    word q - 1.  place: "root" a basis of its own, "view" the drop_last(2) of a
    longer root, "other" inputs made on one root and the case on another of the
    same moduli (only the moduli are shared)."""

    def __init__(self, rn, log_n, Lv, B, bits, n_terms, shared=True, bias=None, edge=False, place="root", seed=0):
        self.rn, self.n, self.Lv, self.B, self.nt = rn, 1 << log_n, Lv, B, n_terms
        n = self.n
        extra = 2 if place == "view" else 0
        root_mod = rn.generate_primes(bits, Lv + extra, n)
        self.mod = root_mod[:Lv]
        rng = np.random.default_rng(9100 + 37 * log_n + 5 * n_terms + seed)
        self.x0, self.x1 = _rand(rng, self.mod, n, n_terms * B), _rand(rng, self.mod, n, n_terms * B)
        self.m = _rand(rng, self.mod, n, n_terms if shared else n_terms * B)
        self.b = None if bias is None else _rand(rng, self.mod, n, 1 if bias == "shared" else B)
        if edge:
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            for c in (self.x0, self.x1, self.m) + (() if self.b is None else (self.b,)):
                c[:] = np.broadcast_to(qm1, c.shape)
        root = rn.RnsBasis(root_mod, n)
        self.root = root  # (kept alive)
        self.basis = root.drop_last(extra) if extra else root
        self.Bo = orc.Basis(self.mod, n)
        self.upload()

    def upload(self):
        rn, Bd = self.rn, self.basis
        self.ct = rn.Ciphertext(rn.RnsPoly.from_channels(self.x0, Bd), rn.RnsPoly.from_channels(self.x1, Bd))
        self.pt = rn.RnsPoly.from_channels(self.m, Bd, in_ntt_domain=True)
        self.bias = None if self.b is None else rn.RnsPoly.from_channels(self.b, Bd, in_ntt_domain=True)

    def model(self, p, rescale):
        bias = None if self.b is None else self.b[p if self.b.shape[0] > 1 else 0]
        return plain_mac_ref(self.Bo, pick_terms(self.x0, p, self.B), pick_terms(self.x1, p, self.B),
                             pick_plain(self.m, p, self.B, self.nt), bias, rescale=rescale)


def _slice(rn, p, first, count):
    t = rn.RnsPoly(p.basis, count)
    t.copy_polys(p, 0, first, count)
    return t


def _coeff(p):
    c = p.clone()
    c.to_coeff_domain()
    return c


def composition(rn, ct, n_terms, pt, bias, rescale):
    """The definition on the device, from existing ops alone: one product and
    one add per term and component, the bias, then rescale_ciphertext."""
    B = ct.c0.n_polys // n_terms
    mc = _coeff(pt)
    acc = [None, None]
    for i in range(n_terms):
        if pt.n_polys == n_terms:  # plaintext i for every ciphertext of the batch
            mi = rn.RnsPoly(pt.basis, B)
            for b in range(B):
                mi.copy_polys(mc, b, i, 1)
        else:
            mi = _slice(rn, mc, i * B, B)
        for j, comp in enumerate((ct.c0, ct.c1)):
            t = _slice(rn, comp, i * B, B) * mi
            acc[j] = t if acc[j] is None else acc[j] + t
    if bias is not None:
        bc = _coeff(bias)
        if bias.n_polys != B:
            one, bc = bc, rn.RnsPoly(bias.basis, B)
            for b in range(B):
                bc.copy_polys(one, b, 0, 1)
        acc[0] = acc[0] + bc
    out = rn.Ciphertext(acc[0], acc[1])
    return rn.rescale_ciphertext(out) if rescale else out


def _same(a, b):
    return (np.array_equal(a.c0.channels_batch(), b.c0.channels_batch()) and
            np.array_equal(a.c1.channels_batch(), b.c1.channels_batch()))


def check_mac(c, model=True):
    """Both calls against the device composition on every poly and against the
    CPU model on polys {0, B - 1}; the inputs are const."""
    rn = c.rn
    outs = {}
    for rescale in (False, True):
        fused = rn.ct_plain_mac(c.ct, c.nt, c.pt, c.bias, rescale=rescale)
        comp = composition(rn, c.ct, c.nt, c.pt, c.bias, rescale)
        for o in (fused.c0, fused.c1):
            assert not o.is_ntt_domain() and o.n_polys == c.B and o.basis.channel_count() == c.Lv - int(rescale)
        assert fused.c0.basis is fused.c1.basis
        assert np.array_equal(fused.c0.channels_batch(), comp.c0.channels_batch()), f"out0, rescale={rescale}"
        assert np.array_equal(fused.c1.channels_batch(), comp.c1.channels_batch()), f"out1, rescale={rescale}"
        outs[rescale] = fused
        for p in sorted({0, c.B - 1}) if model else ():
            r0, r1 = c.model(p, rescale)
            assert np.array_equal(fused.c0.channels_of(p)[0], r0), f"out0 of poly {p}, rescale={rescale}"
            assert np.array_equal(fused.c1.channels_of(p)[0], r1), f"out1 of poly {p}, rescale={rescale}"
    assert np.array_equal(c.ct.c0.channels_batch(), c.x0) and np.array_equal(c.ct.c1.channels_batch(), c.x1)
    assert np.array_equal(c.pt.channels_batch(), c.m) and c.pt.is_ntt_domain()
    if c.bias is not None:
        assert np.array_equal(c.bias.channels_batch(), c.b) and c.bias.is_ntt_domain()
    return outs


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "each"])
@pytest.mark.parametrize("bias", [None, "shared", "each"])
@pytest.mark.parametrize("n_terms", [1, 2, KPLAIN_T - 1, KPLAIN_T, KPLAIN_T + 1, 2 * KPLAIN_T + 1])
def test_group_and_accumulate_boundaries(gpu, n_terms, bias, shared):
    c = MacCase(gpu, 8, 3, 3, 31, n_terms, shared=shared, bias=bias)
    outs = check_mac(c)
    if n_terms == 1 and bias is None and not shared:  # the words of RnsPoly c * m, then rescale_ciphertext
        mc = _coeff(c.pt)
        prod = gpu.Ciphertext(c.ct.c0 * mc, c.ct.c1 * mc)
        assert _same(outs[False], prod) and _same(outs[True], gpu.rescale_ciphertext(prod))
        assert _same(outs[True], gpu.mul_plain(c.ct, c.pt))


@pytest.mark.parametrize("log_n,Lv,B,bits", [(8, 3, 3, 31), (12, 3, 2, 61)])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "each"])
def test_largest_residues(gpu, log_n, Lv, B, bits, shared):
    check_mac(MacCase(gpu, log_n, Lv, B, bits, 2 * KPLAIN_T + 1, shared=shared, bias="each", edge=True))


# log_n, Lv, B, bits, ws_mb
SHAPES = [
    (8, 2, 2, 31, None),    # a single output limb
    (12, 3, 2, 31, None),   # whole-plane transforms
    (14, 3, 3, 31, "1"),    # several chunks of one ciphertext
    (14, 3, 3, 31, "4"),    # chunks of two: a ragged last chunk
    (14, 2, 2, 61, None),   # u64 words
    (15, 2, 2, 31, None),   # the four-step kernels: the column pass reads the inputs
    (16, 4, 2, 31, None),   # matrix-core transforms
    (17, 4, 1, 31, None),   # largest ring
    (14, 3, 64, 31, None),  # un-split grids
]


@pytest.mark.parametrize("log_n,Lv,B,bits,ws_mb", SHAPES)
def test_parity_over_the_transform_paths(gpu, monkeypatch, log_n, Lv, B, bits, ws_mb):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    check_mac(MacCase(gpu, log_n, Lv, B, bits, 3, shared=B % 2 == 0, bias="shared" if B % 2 else "each", seed=B))


@pytest.mark.parametrize("log_n", [12, 14])
def test_four_step_kernels_everywhere(gpu, monkeypatch, log_n):
    """RNT_PLANE=0: the column pass reads the inputs and writes the workspace,
    for the whole batch and per term of a chunk."""
    monkeypatch.setenv("RNT_PLANE", "0")  # read at rnt_ctx_create
    monkeypatch.setenv("RNT_KS_WS_MB", "1")
    check_mac(MacCase(gpu, log_n, 3, 3, 31, 3, shared=False, bias="each", seed=11))


@pytest.mark.parametrize("place", ["view", "other"])
@pytest.mark.parametrize("log_n", [8, 14])
def test_levelled_contexts(gpu, log_n, place):
    c = MacCase(gpu, log_n, 3, 3, 31, 3, shared=False, bias="shared", place="view" if place == "view" else "root",
                seed=1)
    if place == "other":  # the same moduli on an unrelated root
        c.root = c.basis = gpu.RnsBasis(c.mod, c.n)
        c.upload()
    else:
        assert c.root.channel_count() == c.Lv + 2 and c.basis.channel_count() == c.Lv
    check_mac(c)


@pytest.mark.parametrize("only_plaintext", [False, True], ids=["all", "plaintext-only"])
@pytest.mark.parametrize("bits", [31, 61])
def test_unaligned_planes(gpu, bits, only_plaintext):
    """Every buffer wrapped one word off a 16-byte boundary between guard words
    -- or the plaintext alone, so that the launcher's choice of form is seen to
    include it."""
    from test_gpu_unaligned import guards, shifted

    n_terms = KPLAIN_T + 1
    c = MacCase(gpu, 8, 3, 3, bits, n_terms, shared=False, bias="each", seed=4)
    rn, lib, Bd = c.rn, c.rn.load(), c.basis
    pt = shifted(rn, Bd, c.pt)
    assert pt.is_ntt_domain()
    if only_plaintext:
        x0, x1, bias, views = c.ct.c0, c.ct.c1, c.bias, [pt]
    else:
        x0, x1, bias = shifted(rn, Bd, c.ct.c0), shifted(rn, Bd, c.ct.c1), shifted(rn, Bd, c.bias)
        views = [pt, x0, x1, bias]
    for rescale, call in ((False, lib.rnt_ct_plain_mac), (True, lib.rnt_ct_plain_mac_rescale)):
        want = composition(rn, c.ct, n_terms, c.pt, c.bias, rescale)
        ob = want.c0.basis
        if only_plaintext:
            g0, g1 = rn.RnsPoly(ob, c.B), rn.RnsPoly(ob, c.B)
        else:
            g0, g1 = shifted(rn, ob, c.B), shifted(rn, ob, c.B)
            views += [g0, g1]
        rn.check(call(g0.handle, g1.handle, x0.handle, x1.handle, pt.handle, bias.handle, n_terms))
        assert np.array_equal(g0.channels_batch(), want.c0.channels_batch())
        assert np.array_equal(g1.channels_batch(), want.c1.channels_batch())
        guards(*views)
    assert np.array_equal(pt.channels_batch(), c.m)


@pytest.mark.parametrize("log_n", [12, 14])
def test_captured(gpu, log_n):
    """Both calls record into a graph after one plain run; two replays on
    refreshed inputs and refreshed plaintexts give the words of the plain calls."""
    n_terms = KPLAIN_T + 1
    c = MacCase(gpu, log_n, 3, 2, 31, n_terms, shared=True, bias="each", seed=5)
    rn, lib = c.rn, c.rn.load()
    low = c.basis.drop_last(1)
    outs = [rn.RnsPoly(c.basis, c.B) for _ in range(2)] + [rn.RnsPoly(low, c.B) for _ in range(2)]

    def run():
        args = (c.ct.c0.handle, c.ct.c1.handle, c.pt.handle, c.bias.handle, n_terms)
        rn.check(lib.rnt_ct_plain_mac(outs[0].handle, outs[1].handle, *args))
        rn.check(lib.rnt_ct_plain_mac_rescale(outs[2].handle, outs[3].handle, *args))

    run()
    with c.basis.capture() as g:
        run()
    rng = np.random.default_rng(73 + log_n)
    for _ in range(2):
        c.ct.c0.copy_polys(rn.RnsPoly.from_channels(_rand(rng, c.mod, c.n, n_terms * c.B), c.basis))
        c.pt.copy_polys(rn.RnsPoly.from_channels(_rand(rng, c.mod, c.n, n_terms), c.basis, in_ntt_domain=True))
        g.replay()
        c.basis.sync()
        plain = rn.ct_plain_mac(c.ct, n_terms, c.pt, c.bias, rescale=False)
        assert np.array_equal(outs[0].channels_batch(), plain.c0.channels_batch())
        assert np.array_equal(outs[1].channels_batch(), plain.c1.channels_batch())
        assert _same(plain, composition(rn, c.ct, n_terms, c.pt, c.bias, False))
        resc = rn.ct_plain_mac(c.ct, n_terms, c.pt, c.bias, rescale=True)
        assert np.array_equal(outs[2].channels_batch(), resc.c0.channels_batch())
        assert np.array_equal(outs[3].channels_batch(), resc.c1.channels_batch())


NAMES = ("plain_mac", "whole_fwd", "whole_inv", "whole_mul", "rescale", "copy", "elementwise")


def _counts(basis, run):
    run()  # warm: workspaces cached
    basis.profile_enable(True)
    run()
    counts = {k: basis.profile_read(k)[0] for k in NAMES}
    basis.profile_enable(False)
    print(counts)
    return counts


def test_launch_counts(gpu):
    """At 2^14 x 3 limbs x 2 ciphertexts (whole-plane transforms, one chunk):
    ceil(n_terms / kPlainT) k_plain_mac launches and as many forward transforms,
    one inverse over both sums when rescaling (two un-rescaled) and two rescale
    launches whatever n_terms is; the composition's counts grow with n_terms."""
    rn = gpu
    seen = {}
    for n_terms in (1, KPLAIN_T, 2 * KPLAIN_T + 1):
        c = MacCase(rn, 14, 3, 2, 31, n_terms, shared=True, bias="shared", seed=6)
        groups = -(-n_terms // KPLAIN_T)
        fused = _counts(c.basis, lambda: rn.ct_plain_mac(c.ct, n_terms, c.pt, c.bias, rescale=True))
        assert fused["plain_mac"] == groups and fused["whole_fwd"] == groups
        assert (fused["whole_inv"], fused["rescale"], fused["whole_mul"]) == (1, 2, 0)
        plain = _counts(c.basis, lambda: rn.ct_plain_mac(c.ct, n_terms, c.pt, c.bias, rescale=False))
        assert plain["plain_mac"] == groups and (plain["whole_inv"], plain["rescale"]) == (2, 0)
        seen[n_terms] = fused
    mc = _coeff(c.pt)
    terms = [(_slice(rn, c.ct.c0, i * c.B, c.B), _slice(rn, c.ct.c1, i * c.B, c.B)) for i in range(n_terms)]
    ms = [_slice(rn, mc, i, 1) for i in range(n_terms)]

    def loop():  # one product per term, component and ciphertext, one add per term, one rescale
        a0 = a1 = None
        for (t0, t1), m in zip(terms, ms):
            mm = rn.RnsPoly(m.basis, c.B)
            for b in range(c.B):
                mm.copy_polys(m, b, 0, 1)
            p0, p1 = t0 * mm, t1 * mm
            a0, a1 = (p0, p1) if a0 is None else (a0 + p0, a1 + p1)
        rn.rescale_ciphertext(rn.Ciphertext(a0, a1))

    comp = _counts(c.basis, loop)
    assert comp["plain_mac"] == 0 and comp["whole_mul"] >= 2 * n_terms and comp["rescale"] == 2
    assert seen[1]["rescale"] == seen[2 * KPLAIN_T + 1]["rescale"] == 2


def test_launch_counts_over_chunks(gpu, monkeypatch):
    """RNT_KS_WS_MB=1 at 2^14 x 3 limbs: one ciphertext a chunk, so every count is per chunk."""
    monkeypatch.setenv("RNT_KS_WS_MB", "1")
    n_terms, B = 3, 3
    c = MacCase(gpu, 14, 3, B, 31, n_terms, shared=False, seed=7)
    fused = _counts(c.basis, lambda: gpu.ct_plain_mac(c.ct, n_terms, c.pt, None, rescale=True))
    assert (fused["plain_mac"], fused["whole_inv"], fused["rescale"]) == (B, B, 2 * B)


def test_errors(gpu):
    """Every row of the header's table, with its status and fields; a refused
    call leaves marked outputs untouched."""
    n_terms = 3
    c = MacCase(gpu, 8, 3, 2, 31, n_terms, shared=True, bias="each", seed=8)
    rn, lib, Bd, B, n = c.rn, c.rn.load(), c.basis, c.B, c.n
    low = Bd.drop_last(1)
    rng = np.random.default_rng(78)
    marks = {False: (_rand(rng, c.mod, n, B), _rand(rng, c.mod, n, B)),
             True: (_rand(rng, c.mod[:-1], n, B), _rand(rng, c.mod[:-1], n, B))}
    outs = {False: tuple(rn.RnsPoly.from_channels(m, Bd) for m in marks[False]),
            True: tuple(rn.RnsPoly.from_channels(m, low) for m in marks[True])}
    other = rn.RnsBasis(c.mod, n)

    def ntt(count, basis=Bd, in_ntt=True):
        return rn.RnsPoly.from_channels(np.zeros((count, basis.channel_count(), n), np.uint64), basis,
                                        in_ntt_domain=in_ntt)

    # a key level view: a hybrid key over q_0..q_2, p_0 seen at level 2
    emod = c.mod + rn.generate_primes(31, 4, n)[3:]
    ext = rn.RnsBasis(emod, n)
    key = rn.RnsHybridKey.from_channels(_rand(rng, emod, n, 3), _rand(rng, emod, n, 3), ext, 1, n_special=1)
    view = key.at_level(2).a
    for rescale in (False, True):
        o0, o1 = outs[rescale]
        fn = lib.rnt_ct_plain_mac_rescale if rescale else lib.rnt_ct_plain_mac

        def mac(out0=o0, out1=o1, x0=c.ct.c0, x1=c.ct.c1, m=c.pt, bias=c.bias, nt=n_terms):
            return fn(out0.handle, out1.handle, x0.handle, x1.handle, m.handle, None if bias is None else bias.handle,
                      nt)

        def fails(kind, fields=None, **kw):
            with pytest.raises(rn.RnsNttError) as e:
                rn.check(mac(**kw))
            assert e.value.kind == kind, (kind, rescale, kw.keys(), str(e.value))
            if fields is not None:
                assert e.value.fields == fields, e.value.fields
            for o, m in zip(outs[rescale], marks[rescale]):
                assert np.array_equal(o.channels_batch(), m), kw.keys()

        ob = o0.basis
        fails("BadArgument", nt=0)
        fails("BadArgument", nt=4)  # 6 polys are no 4 terms
        fails("BadArgument", x1=rn.RnsPoly(Bd, n_terms * B + 1))  # input poly counts differ
        fails("BadArgument", m=ntt(n_terms + 1))  # neither n_terms nor n_terms B plaintexts
        fails("BadArgument", m=ntt(n_terms * B + 1))
        fails("BadArgument", bias=ntt(B + 1))  # neither 1 nor B
        fails("BadArgument", out0=rn.RnsPoly(ob, B + 1))  # outputs of other than B polys
        fails("BadArgument", out1=rn.RnsPoly(ob, n_terms * B))
        fails("BadArgument", out1=o0)  # out0 == out1
        if not rescale:  # an output that is an input (the rescaling call's outputs live on another context)
            two = rn.RnsPoly.from_channels(c.x0[:B], Bd)
            for kw in ({"x0": two, "x1": c.ct.c1}, {"x0": c.ct.c0, "x1": two}):
                with pytest.raises(rn.RnsNttError) as e:
                    rn.check(fn(two.handle, o1.handle, kw["x0"].handle, kw["x1"].handle, ntt(1).handle, None, 1))
                assert e.value.kind == "BadArgument" and np.array_equal(two.channels_batch(), c.x0[:B])
            pm = ntt(B)
            with pytest.raises(rn.RnsNttError) as e:  # the plaintext or the bias as an output
                rn.check(fn(pm.handle, o1.handle, c.ct.c0.handle, c.ct.c1.handle, pm.handle, None, n_terms))
            assert e.value.kind == "BadArgument"
            with pytest.raises(rn.RnsNttError) as e:
                rn.check(fn(o0.handle, pm.handle, c.ct.c0.handle, c.ct.c1.handle, c.pt.handle, pm.handle, n_terms))
            assert e.value.kind == "BadArgument"
        # inputs, plaintexts or bias on different contexts; outputs on the wrong context
        fails("BasisMismatch", x1=rn.RnsPoly(other, n_terms * B))
        fails("BasisMismatch", m=ntt(n_terms, other))
        fails("BasisMismatch", bias=ntt(B, other))
        wrongs = (Bd, Bd.drop_last(2), rn.RnsBasis(c.mod[:-1], n)) if rescale else (low, other)
        for wrong in wrongs:
            fails("BasisMismatch", out0=rn.RnsPoly(wrong, B))
            fails("BasisMismatch", out1=rn.RnsPoly(wrong, B))
        if rescale:  # the right limbs on a context of their own: the outputs do not share one
            fails("BasisMismatch", out1=rn.RnsPoly(Bd.drop_last(1), B))
        for name in ("x0", "x1"):
            t = getattr(c.ct, "c" + name[1]).clone()
            t.to_ntt_domain()
            fails("DomainMismatch", **{name: t})
        fails("DomainMismatch", m=ntt(n_terms, in_ntt=False))
        fails("DomainMismatch", bias=ntt(B, in_ntt=False))
        # a key level view in each position
        for pos in ("out0", "out1", "x0", "x1", "m", "bias"):
            fails("Unsupported", {"degree": 0, "max_degree": 0}, **{pos: view})
        if rescale:  # a one-limb ciphertext: nothing to drop
            one = MacCase(gpu, 8, 1, B, 31, n_terms, shared=True, bias="each", seed=8)
            fails("InvalidModDrop", {"drop_count": 1, "channel_count": 1}, x0=one.ct.c0, x1=one.ct.c1, m=one.pt,
                  bias=one.bias)
        # the valid call still runs after all that, and without a bias
        rn.check(mac())
        want = composition(rn, c.ct, n_terms, c.pt, c.bias, rescale)
        assert np.array_equal(o0.channels_batch(), want.c0.channels_batch())
        assert np.array_equal(o1.channels_batch(), want.c1.channels_batch())
        rn.check(mac(bias=None))
        want = composition(rn, c.ct, n_terms, c.pt, None, rescale)
        assert np.array_equal(o0.channels_batch(), want.c0.channels_batch())
        # both calls are recordable
        with Bd.capture():
            rn.check(mac())


def test_python_layer_guards(gpu):
    from rns_ntt.engine import CkksEngine

    c = MacCase(gpu, 8, 3, 2, 31, 2, shared=True, bias="shared", seed=9)
    rn = c.rn
    ct = rn.Ciphertext(c.ct.c0, c.ct.c1, 30, 90)
    with pytest.raises(ValueError):
        rn.ct_plain_mac(ct, 3, c.pt)  # 4 polys are no 3 terms
    with pytest.raises(ValueError):
        rn.ct_plain_mac(ct, 0, c.pt)
    with pytest.raises(ValueError):
        rn.ct_plain_mac(ct, 2, _slice(rn, c.pt, 0, 1))  # one plaintext for two terms
    with pytest.raises(ValueError):
        rn.ct_plain_mac(ct, 2, c.pt, rn.RnsPoly(c.basis, 3))  # a bias of 3 for a batch of 2
    with pytest.raises(ValueError):
        rn.ct_plain_mac(ct, 2, _coeff(c.pt))  # a coefficient-domain plaintext
    with pytest.raises(ValueError):
        rn.ct_plain_mac(ct, 2, c.pt, _coeff(c.bias))
    with pytest.raises(ValueError):
        rn.ct_plain_mac(ct, 2, c.m)  # not an RnsPoly
    bits = c.mod[-1].bit_length()
    out = rn.ct_plain_mac(ct, 2, c.pt, c.bias)
    assert (out.logp, out.logq) == (30 - bits, 90 - bits) and out.c0.n_polys == 2
    out = rn.ct_plain_mac(ct, 2, c.pt, c.bias, rescale=False)
    assert (out.logp, out.logq) == (30, 90) and out.c0.basis is c.basis
    low = c.basis.drop_last(1)
    assert rn.ct_plain_mac(ct, 2, c.pt, out_basis=low).c0.basis is low
    four = rn.RnsPoly.from_channels(np.concatenate([c.m, c.m]), c.basis, in_ntt_domain=True)
    out = rn.mul_plain(ct, four)  # one term of four ciphertexts, a plaintext each
    assert out.c0.n_polys == 4 and (out.logp, out.logq) == (30 - bits, 90 - bits)
    assert _same(out, rn.ct_plain_mac(ct, 1, four))
    assert _same(rn.mul_plain(ct, four, rescale=False), rn.ct_plain_mac(ct, 1, four, rescale=False))
    # the engine: Plaintexts in either domain, logp = ct.logp + scale_bits - bits dropped, the bias at the products' scale
    pt, pc = rn.Plaintext(c.pt, 25, c.n // 2), rn.Plaintext(_coeff(c.pt), 25, c.n // 2)
    bias = rn.Plaintext(c.bias, 55, c.n // 2)
    prepared = CkksEngine.prepare_plaintext(pc)
    assert prepared.poly.is_ntt_domain() and not pc.poly.is_ntt_domain() and prepared.scale_bits == 25
    assert np.array_equal(prepared.poly.channels_batch(), c.m)
    a = CkksEngine.plain_mac(ct, 2, pt, bias)
    assert (a.logp, a.logq) == (55 - bits, 90 - bits)
    assert _same(a, CkksEngine.plain_mac(ct, 2, pc, rn.Plaintext(_coeff(c.bias), 55, c.n // 2)))
    assert _same(a, rn.ct_plain_mac(ct, 2, c.pt, c.bias))
    assert CkksEngine.plain_mac(ct, 2, pt, rescale=False).logp == 55
    with pytest.raises(ValueError):
        CkksEngine.plain_mac(ct, 2, pt, rn.Plaintext(c.bias, 30, c.n // 2))
    e = CkksEngine.mul_plaintext(ct, rn.Plaintext(four, 25, c.n // 2))
    assert (e.logp, e.logq) == (55 - bits, 90 - bits) and _same(e, out)
    with pytest.raises(AssertionError):
        CkksEngine.add_plaintext(ct, pt)  # logp 30 against scale 25
    s = CkksEngine.add_plaintext(ct, rn.Plaintext(four, 30, c.n // 2))
    assert (s.logp, s.logq) == (30, 90)
    assert np.array_equal(s.c0.channels_batch(), (c.ct.c0 + _coeff(four)).channels_batch())
    assert np.array_equal(s.c1.channels_batch(), c.x1)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _one(rn, p, i=0):
    return rn.RnsPoly.from_channels(np.ascontiguousarray(p.channels_batch()[i]), p.basis)


def _decode(rn, eng, ct, sk, q, logp, slots):
    """Decrypted on the device over all the limbs, lifted with the big-integer
    centred CRT and decoded at the nominal scale, as tools/plain_mac_tolerance.py
    does."""
    from rns_ntt.engine import CkksEngine

    lv = ct.c0.basis.channel_count()
    sk_l = CkksEngine.secret_on(sk, ct.c0.basis)
    dec = CkksEngine.decrypt(rn.Ciphertext(_one(rn, ct.c0), _one(rn, ct.c1)), sk_l).channels()
    coeffs = np.array(crt_centered(dec, q[:lv]), dtype=np.int64)
    return cpu_encoder.decode_fft(coeffs, eng.basis.degree, logp, slots)


@pytest.fixture(scope="module")
def ring(gpu):
    """The evaluator tests' ring: N = 2^10, 7 x 30-bit primes, 2 special primes,
    scale 2^30; eight encrypted vectors, packed."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L, K, logp, n_terms = 1024, 512, 7, 2, 30, 8
    q, p = orc.generate_primes(logp, L, n), orc.generate_primes(31, K, n)
    eng = CkksEngine(q, n, error_std=3.2, hamming_weight=n // 2, special_moduli=p)
    rng = rn.DeviceRng(191)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    host = np.random.default_rng(192)
    a = host.uniform(-1, 1, (n_terms, slots))
    enc = rn.CkksEncoder(n, logp)
    cts = [eng.encrypt(enc.encode(v, eng.basis), pk, rng, logp=logp) for v in a]
    c0, c1 = rn.RnsPoly(eng.basis, n_terms), rn.RnsPoly(eng.basis, n_terms)
    for i, ct in enumerate(cts):
        c0.copy_polys(ct.c0, i, 0, 1)
        c1.copy_polys(ct.c1, i, 0, 1)
    packed = rn.Ciphertext(c0, c1, logp, cts[0].logq)
    return dict(rn=rn, eng=eng, q=q, sk=sk, pk=pk, rng=rng, host=host, a=a, enc=enc, cts=cts, packed=packed,
                slots=slots, logp=logp, n=n)


def _encode_batch(r, values, scale_bits):
    rn = r["rn"]
    enc = rn.CkksEncoder(r["n"], scale_bits)
    out = rn.RnsPoly(r["eng"].basis, len(values))
    for i, v in enumerate(values):
        out.copy_polys(enc.encode(v, r["eng"].basis).poly, i, 0, 1)
    return rn.Plaintext(out, scale_bits, r["slots"])


def test_engine_plain_mac_end_to_end(ring):
    """encrypt 8 vectors -> plain_mac with 8 encoded weight vectors and a bias,
    rescaled -> decrypt -> decode against numpy's sum_i w_i a_i + b, within
    4 x tools/plain_mac_tolerance.py's figure."""
    from rns_ntt.engine import CkksEngine

    r = ring
    rn, q, logp, slots = r["rn"], r["q"], r["logp"], r["slots"]
    w, b = r["host"].uniform(-1, 1, (8, slots)), r["host"].uniform(-1, 1, slots)
    pt = CkksEngine.prepare_plaintext(_encode_batch(r, w, logp))
    bias = _encode_batch(r, [b], 2 * logp)
    got = CkksEngine.plain_mac(r["packed"], 8, pt, bias)
    assert got.c0.n_polys == 1 and got.c0.basis.channel_count() == 6
    assert got.logp == 2 * logp - q[-1].bit_length() and got.logq == r["packed"].logq - q[-1].bit_length()
    assert _same(got, composition(rn, r["packed"], 8, pt.poly, CkksEngine.prepare_plaintext(bias).poly, True))
    err = float(np.max(np.abs(_decode(rn, r["eng"], got, r["sk"], q, got.logp, slots) - (np.sum(w * r["a"], 0) + b))))
    tol = _tolerance()
    print(f"plain_mac of 8 terms + bias: decode error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


def test_engine_mul_and_add_plaintext_end_to_end(ring):
    from rns_ntt.engine import CkksEngine

    r = ring
    rn, q, logp, slots = r["rn"], r["q"], r["logp"], r["slots"]
    w = r["host"].uniform(-1, 1, slots)
    tol = _tolerance()
    ct = r["cts"][0]
    got = CkksEngine.mul_plaintext(ct, r["enc"].encode(w, r["eng"].basis))
    assert got.logp == 2 * logp - q[-1].bit_length()
    err = float(np.max(np.abs(_decode(rn, r["eng"], got, r["sk"], q, got.logp, slots) - w * r["a"][0])))
    print(f"mul_plaintext: decode error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    s = CkksEngine.add_plaintext(ct, r["enc"].encode(w, r["eng"].basis))
    assert (s.logp, s.logq) == (ct.logp, ct.logq)
    err = float(np.max(np.abs(_decode(rn, r["eng"], s, r["sk"], q, s.logp, slots) - (w + r["a"][0]))))
    print(f"add_plaintext: decode error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


def test_hoisted_rotations_then_plain_mac_end_to_end(ring):
    """The diagonal method by hand: rotate_hoisted_hybrid over 4 steps writes
    the packed layout plain_mac reads; with 4 diagonals the result decodes to
    the matrix-vector product."""
    from rns_ntt.engine import CkksEngine

    r = ring
    rn, eng, q, logp, slots = r["rn"], r["eng"], r["q"], r["logp"], r["slots"]
    steps = [0, 1, 2, 3]
    kset = eng.generate_hybrid_rotation_key_set(r["sk"], steps, r["rng"], 2, hoisted=True)
    x = r["a"][1]
    M = np.zeros((slots, slots))
    s = np.arange(slots)
    diags = r["host"].uniform(-1, 1, (len(steps), slots))
    for d, row in zip(steps, diags):
        M[s, (s + d) % slots] = row
    rot = CkksEngine.rotate_hoisted_hybrid(r["cts"][1], kset)
    assert rot.c0.n_polys == len(steps)
    got = CkksEngine.plain_mac(rot, len(steps), CkksEngine.prepare_plaintext(_encode_batch(r, diags, logp)))
    assert got.c0.n_polys == 1 and got.logp == 2 * logp - q[-1].bit_length()
    err = float(np.max(np.abs(_decode(rn, eng, got, r["sk"], q, got.logp, slots) - M @ x)))
    tol = _tolerance()
    print(f"hoisted rotations + plain_mac, 4 diagonals: decode error {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
