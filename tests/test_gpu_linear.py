"""rnt_ct_linear on the GPU: out = sum_t diag_t * rotate_ciphertext(ct, steps[t]).

Every step of the composition (rnt_ct_rotate, the coefficient-domain product,
rnt_add) is exact arithmetic mod q_j with canonical outputs, so the fused call
must reproduce it word for word: against the CPU yardstick (tests/lt_ref.py,
itself checked in tests/test_linear_ref.py) and against the library's own
composition, on every kind of ring the key-switch treats differently.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from lt_ref import linear_ref

pytestmark = pytest.mark.gpu

T = orc.host_threads()
# a zero step, a negative step, a duplicate and more than two nonzero steps:
# both the writing and the accumulating store of the rows kernel run
STEPS = [0, 1, -3, 5, 1]


def _rand(rng, mod, n, batch):
    return orc.uniform_poly(mod, n, rng, batch=batch)


class Case:
    """Random ciphertexts, plaintexts and key channels on one ring, uploaded.
    With `drop`, the L limbs are a drop_last(drop) view of a root basis of
    L + drop primes (`root`) instead of a basis of their own."""

    def __init__(self, rn, log_n, L, B, bits, steps=STEPS, seed=0, edge=False, drop=0):
        self.rn, self.n, self.L, self.B, self.steps = rn, 1 << log_n, L, B, list(steps)
        n = self.n
        self.drop = drop
        self.root_mod = rn.generate_primes(bits, L + drop, n)
        self.mod = self.root_mod[:L]
        rng = np.random.default_rng(2100 + 31 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.diag = _rand(rng, self.mod, n, len(steps))  # coefficient domain
        if edge:  # an all-(q-1) ciphertext and an all-(q-1) diagonal
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.c0[B - 1] = self.c1[B - 1] = np.broadcast_to(qm1, (L, n))
            self.diag[min(2, len(steps) - 1)] = np.broadcast_to(qm1, (L, n))
        self.keys = [None if k == 0 else (_rand(rng, self.mod, n, L), _rand(rng, self.mod, n, L)) for k in steps]
        self.upload()

    def upload(self):
        rn = self.rn
        self.root = rn.RnsBasis(self.root_mod, self.n)
        self.basis = Bd = self.root.drop_last(self.drop) if self.drop else self.root
        self.gk = [None if kk is None else rn.RnsGadgetKey.from_channels(kk[0], kk[1], Bd, rotation=k)
                   for k, kk in zip(self.steps, self.keys)]
        self.keyset = rn.RnsGadgetKeySet(self.gk, Bd)
        self.d = rn.RnsPoly.from_channels(self.diag, Bd)
        self.d.to_ntt_domain()
        self.ct = rn.Ciphertext(rn.RnsPoly.from_channels(self.c0, Bd), rn.RnsPoly.from_channels(self.c1, Bd))

    def composed(self):
        """The library's own composition: rotate_ciphertext, product, add."""
        rn, acc = self.rn, None
        for t, k in enumerate(self.steps):
            r = self.ct if k == 0 else rn.rotate_ciphertext(self.ct, self.gk[t])
            m = rn.RnsPoly.from_channels(np.broadcast_to(self.diag[t], (self.B, self.L, self.n)).copy(), self.basis)
            p0, p1 = r.c0 * m, r.c1 * m
            acc = (p0, p1) if acc is None else (acc[0] + p0, acc[1] + p1)
        return acc[0].channels(), acc[1].channels()

    def reference(self, p):
        Bo = orc.Basis(self.mod, self.n)
        return linear_ref(Bo, self.c0[p], self.c1[p], self.steps, self.diag, self.keys, threads=T)


def _check_parity(c):
    out = c.rn.linear_transform(c.ct, c.d, c.keyset)
    g0, g1 = out.c0.channels(), out.c1.channels()
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    w0, w1 = c.composed()
    assert np.array_equal(g0, w0) and np.array_equal(g1, w1), "differs from the library's composition"
    for p in sorted({0, c.B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from linear_ref"


@pytest.mark.parametrize("log_n,L,B,bits,ws_mb,edge", [
    (8, 3, 3, 31, None, False),   # small four-step grid
    (8, 3, 3, 31, None, True),    # the same with all-(q-1) operands
    (14, 3, 3, 31, "1", False),   # three one-ciphertext chunks: chunk-local accumulators
    (12, 3, 2, 61, None, False),  # u64 rows kernel
    (14, 2, 2, 61, None, False),  # u64 rows of 128 words: the epilogue whose loop stays rolled
    (16, 4, 2, 31, None, False),  # the matrix-core ring's key-switch
    (17, 4, 1, 31, None, False),  # the KSPLIT instantiation
    (12, 3, 2, 31, None, False),  # whole-plane fallback
])
def test_linear_parity(gpu, monkeypatch, log_n, L, B, bits, ws_mb, edge):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    _check_parity(Case(gpu, log_n, L, B, bits, edge=edge))


def test_linear_shares_one_pair_of_inverse_column_passes(gpu):
    """Fusion: four terms in one chunk run three decompositions, three rows
    launches and -- beyond what the step-0 product itself launches -- exactly
    two inverse column passes.  A wrapper over the composition would run two
    per rotation and one per product."""
    c = Case(gpu, 14, 3, 2, 31, steps=[0, 1, 2, 3])
    zero = Case(gpu, 14, 3, 2, 31, steps=[0])
    counts = {}
    for name, case in (("zero", zero), ("full", c)):
        case.rn.linear_transform(case.ct, case.d, case.keyset)  # warm: workspaces cached
        case.basis.profile_enable(True)
        case.rn.linear_transform(case.ct, case.d, case.keyset)
        counts[name] = {k: case.basis.profile_read(k)[0] for k in ("col_inv", "ks_rows", "ks_decompose")}
        case.basis.profile_enable(False)
    print(counts)
    assert counts["full"]["col_inv"] - counts["zero"]["col_inv"] == 2
    assert counts["full"]["ks_rows"] == 3
    assert counts["full"]["ks_decompose"] == 3
    assert counts["zero"]["ks_rows"] == 0 and counts["zero"]["ks_decompose"] == 0


@pytest.mark.parametrize("log_n,L,B,bits", [(8, 3, 3, 31), (12, 3, 2, 31)])
def test_linear_in_place(gpu, log_n, L, B, bits):
    c = Case(gpu, log_n, L, B, bits)
    out = c.rn.linear_transform(c.ct, c.d, c.keyset)
    w0, w1 = out.c0.channels(), out.c1.channels()
    same = c.rn.linear_transform(c.ct, c.d, c.keyset, out=c.ct)
    assert same is c.ct
    assert np.array_equal(c.ct.c0.channels(), w0) and np.array_equal(c.ct.c1.channels(), w1)


@pytest.mark.parametrize("log_n,L,B,bits", [(14, 3, 2, 31), (12, 3, 2, 31)])
def test_linear_captured(gpu, log_n, L, B, bits):
    """Only device ops are queued: the call records into a graph, and two
    replays leave the eager output."""
    c = Case(gpu, log_n, L, B, bits)
    rn = c.rn
    eager = rn.linear_transform(c.ct, c.d, c.keyset)
    w0, w1 = eager.c0.channels(), eager.c1.channels()
    out = rn.Ciphertext(rn.RnsPoly(c.basis, B), rn.RnsPoly(c.basis, B))
    with c.basis.capture() as g:
        rn.linear_transform(c.ct, c.d, c.keyset, out=out)
    for _ in range(2):
        g.replay()
    c.basis.sync()
    assert np.array_equal(out.c0.channels(), w0) and np.array_equal(out.c1.channels(), w1)


def test_copy_polys_packs_key_sets(gpu):
    c = Case(gpu, 8, 3, 2, 31)
    L = c.L
    pa, pb = c.keyset.a, c.keyset.b
    assert pa.n_polys == len(STEPS) * L and pa.is_ntt_domain() and pb.is_ntt_domain()
    for t, k in enumerate(c.gk):
        if k is None:
            assert not pa.channels_of(t * L, L).any() and not pb.channels_of(t * L, L).any()
            continue
        assert np.array_equal(pa.channels_of(t * L, L), k.a.channels())
        assert np.array_equal(pb.channels_of(t * L, L), k.b.channels())
    rn = c.rn
    dst, src = rn.RnsPoly(c.basis, 4), rn.RnsPoly.from_channels(c.c0, c.basis)
    for args in ((3, 0, 2), (0, 1, 2), (5, 0, 1), (0, 3, 1), (0, 0, 0)):
        with pytest.raises(rn.RnsNttError) as e:
            dst.copy_polys(src, *args)
        assert e.value.kind == "BadArgument", args
    dst.copy_polys(src, 2, 0, 2)
    assert np.array_equal(dst.channels_of(2, 2), c.c0) and not dst.channels_of(0, 2).any()
    # a partial copy keeps the destination's domain, so the domains must agree
    src.to_ntt_domain()
    with pytest.raises(rn.RnsNttError) as e:
        dst.copy_polys(src, 0, 0, 2)
    assert e.value.kind == "DomainMismatch"
    whole = rn.RnsPoly(c.basis, 2)
    whole.copy_polys(src)  # all of dst: it takes src's domain
    assert whole.is_ntt_domain() and np.array_equal(whole.channels(), src.channels())


def test_linear_errors(gpu):
    """Every row of the issue's error table, with its fields."""
    c = Case(gpu, 8, 3, 2, 31, steps=[0, 1])
    rn, lib, Bd, L, B = c.rn, c.rn.load(), c.basis, c.L, c.B
    o0, o1 = rn.RnsPoly(Bd, B), rn.RnsPoly(Bd, B)
    steps = (ctypes.c_int32 * 2)(0, 1)
    ks = c.keyset

    def call(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, st=steps, nt=2, diag=c.d, ka=ks.a, kb=ks.b):
        h = lambda x: None if x is None else x.handle  # noqa: E731
        return lib.rnt_ct_linear(h(out0), h(out1), h(c0), h(c1), st, nt, h(diag), h(ka), h(kb))

    def fails(kind, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(call(**kw))
        assert e.value.kind == kind, (kind, kw.keys())
        if fields is not None:
            assert e.value.fields == fields

    rn.check(call())  # the valid call
    fails("BadArgument", nt=0)
    fails("BadArgument", st=None)
    fails("BadArgument", diag=rn.RnsPoly.from_channels(c.diag[:1], Bd, in_ntt_domain=True))
    short = rn.RnsPoly.from_channels(np.zeros((L, L, c.n), np.uint64), Bd, in_ntt_domain=True)
    fails("ChannelCountMismatch", {"expected": 2 * L, "actual": L}, ka=short)
    fails("ChannelCountMismatch", {"expected": 2 * L, "actual": L}, kb=short)
    fails("DomainMismatch", diag=rn.RnsPoly.from_channels(c.diag, Bd))
    raw = rn.RnsPoly.from_channels(np.zeros((2 * L, L, c.n), np.uint64), Bd)
    fails("DomainMismatch", ka=raw)
    ntt = c.ct.c0.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", c0=ntt)
    fails("DomainMismatch", c1=ntt)
    other = rn.RnsBasis(c.mod, c.n)
    fails("BasisMismatch", c1=rn.RnsPoly.from_channels(c.c1, other))
    fails("BasisMismatch", diag=rn.RnsPoly.from_channels(c.diag, other, in_ntt_domain=True))
    fails("BasisMismatch", ka=rn.RnsPoly.from_channels(np.zeros((2 * L, L, c.n), np.uint64), other,
                                                      in_ntt_domain=True))
    fails("BasisMismatch", out0=rn.RnsPoly(other, B))
    # aliasing: out0 == out1 and an output on another input
    fails("BadArgument", out1=o0)
    fails("BadArgument", out0=c.ct.c1)
    fails("BadArgument", out1=c.ct.c0)
    fails("BadArgument", ka=None)  # a nonzero step needs its key
    # every step 0: the key buffers may be NULL
    z = (ctypes.c_int32 * 2)(0, 0)
    rn.check(call(st=z, ka=None, kb=None))


def test_engine_linear_transform_end_to_end(gpu):
    """Encode -> encrypt -> a 3-diagonal matrix (diagonals 0, 1 and slots - 1)
    through CkksEngine.linear_transform -> rescale -> decrypt -> decode at
    N = 64, 4 x 31-bit primes, ciphertext scale 2^58, diagonal scale 2^30,
    x and the diagonals uniform in (-1, 1).

    (a) The ciphertext equals the composed engine path word for word.
    (b) The slots match M @ x.  The same pipeline on the CPU (oracle/pyoracle,
    encoder.py, numpy draws; tests/lt_ref.py for the transform) decodes with a
    largest absolute error of 8.94e-6 over eight seeds (3.6e-6 .. 8.9e-6;
    max|y| 1.1 .. 1.8, i.e. below 1e-5 of max|y|, against the 1e-3 asked of
    the parameters).  Tolerance: 4 x 8.94e-6 = 3.58e-5; the margin covers other
    random draws, the arithmetic being identical."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L = 64, 32, 4
    eng = CkksEngine(rn.generate_primes(31, L, n), n, error_std=3.2, hamming_weight=n // 2)
    rng = np.random.default_rng(77)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    steps = [0, 1, slots - 1]
    keyset = eng.generate_rotation_key_set(sk, steps, rng)
    assert keyset.steps == steps
    x = rng.uniform(-1, 1, slots)
    M = np.zeros((slots, slots))
    i = np.arange(slots)
    for k in steps:
        M[i, (i + k) % slots] = rng.uniform(-1, 1, slots)
    enc_x, enc_d = rn.CkksEncoder(n, 58), rn.CkksEncoder(n, 30)
    ct = eng.encrypt(enc_x.encode(x, eng.basis), pk, rng)
    diags = eng.encode_diagonals(M, steps, enc_d)
    assert diags.poly.n_polys == 3 and diags.poly.is_ntt_domain()
    out = CkksEngine.linear_transform(ct, diags, keyset)
    assert out.logp == 58 + 30 and out.logq == ct.logq
    # (a) the composed engine path: rotate, coefficient-domain product, add
    dc = diags.poly.clone()
    dc.to_coeff_domain()
    dch = dc.channels()
    acc = None
    for t, k in enumerate(steps):
        r = ct if k == 0 else CkksEngine.rotate_ciphertext(ct, _key_of(rn, keyset, t, eng.basis))
        m = rn.RnsPoly.from_channels(dch[t], eng.basis)
        p0, p1 = r.c0 * m, r.c1 * m
        acc = (p0, p1) if acc is None else (acc[0] + p0, acc[1] + p1)
    assert np.array_equal(out.c0.channels(), acc[0].channels())
    assert np.array_equal(out.c1.channels(), acc[1].channels())
    # (b) rescale, decrypt, decode
    res = CkksEngine.rescale_ciphertext(out)
    pt = CkksEngine.decrypt_plaintext(res, CkksEngine.secret_on(sk, res.c0.basis))
    got = enc_x.decode(pt)
    y = M @ x
    err = float(np.max(np.abs(got - y)))
    print(f"linear transform decode error {err:.3e}, max|y| {np.max(np.abs(y)):.3f}")
    assert err <= 4 * 8.94e-6


def _key_of(rn, keyset, t, basis):
    """Term t's gadget key out of a packed set, as a key of its own (already
    NTT-resident: rnt_key_prepare leaves an NTT-domain buffer alone)."""
    L = basis.channel_count()
    a, b = rn.RnsPoly(basis, L), rn.RnsPoly(basis, L)
    a.copy_polys(keyset.a, 0, t * L, L)
    b.copy_polys(keyset.b, 0, t * L, L)
    return rn.RnsGadgetKey(a, b, keyset.steps[t])
