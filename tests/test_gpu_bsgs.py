"""rnt_ct_linear_bsgs on the GPU:

    R_i = rotate_ciphertext(ct, baby[i]),  V_j = sum_i P[j][i] * R_i,
    out = sum_j rotate_ciphertext(V_j, giant[j]).

Every step of the composition (rnt_ct_rotate, the coefficient-domain product,
rnt_add) is exact arithmetic mod q_j with canonical outputs, so the call must
reproduce it word for word: against the CPU yardstick (tests/bsgs_ref.py,
itself checked in tests/test_bsgs_ref.py) and against the library's own
composition, on every kind of ring the key-switch treats differently.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import pyoracle as orc
from bsgs_ref import bsgs_ref

pytestmark = pytest.mark.gpu

T = orc.host_threads()
# each list has a zero, a negative step and a duplicate; two nonzero giants and
# more: both the storing and the accumulating rows epilogue run
BABY = [0, 1, -3, 1]
GIANT = [0, 4, -8, 4]
SMALL = ([0, 1], [0, 2, -4])


def _rand(rng, mod, n, batch):
    return orc.uniform_poly(mod, n, rng, batch=batch)


class Case:
    """Random ciphertexts, plaintexts and key channels on one ring, uploaded.
    With `drop`, the L limbs are a drop_last(drop) view of a root basis of
    L + drop primes (`root`) instead of a basis of their own."""

    def __init__(self, rn, log_n, L, B, bits, baby=BABY, giant=GIANT, seed=0, edge=False, drop=0):
        self.rn, self.n, self.L, self.B = rn, 1 << log_n, L, B
        self.baby, self.giant = list(baby), list(giant)
        n, nt = self.n, len(baby) * len(giant)
        self.drop = drop
        self.root_mod = rn.generate_primes(bits, L + drop, n)
        self.mod = self.root_mod[:L]
        rng = np.random.default_rng(3100 + 31 * log_n + seed)
        self.c0, self.c1 = _rand(rng, self.mod, n, B), _rand(rng, self.mod, n, B)
        self.diag = _rand(rng, self.mod, n, nt)  # coefficient domain, poly j n1 + i
        if edge:  # an all-(q-1) ciphertext and an all-(q-1) plaintext
            qm1 = np.array(self.mod, dtype=np.uint64)[:, None] - np.uint64(1)
            self.c0[B - 1] = self.c1[B - 1] = np.broadcast_to(qm1, (L, n))
            self.diag[min(len(baby) + 1, nt - 1)] = np.broadcast_to(qm1, (L, n))
        self.bkeys = [None if k == 0 else (_rand(rng, self.mod, n, L), _rand(rng, self.mod, n, L)) for k in baby]
        self.gkeys = [None if k == 0 else (_rand(rng, self.mod, n, L), _rand(rng, self.mod, n, L)) for k in giant]
        self.upload()

    def upload(self):
        rn = self.rn
        self.root = rn.RnsBasis(self.root_mod, self.n)
        self.basis = Bd = self.root.drop_last(self.drop) if self.drop else self.root

        def up(steps, keys):
            return [None if kk is None else rn.RnsGadgetKey.from_channels(kk[0], kk[1], Bd, rotation=k)
                    for k, kk in zip(steps, keys)]

        self.bgk, self.ggk = up(self.baby, self.bkeys), up(self.giant, self.gkeys)
        self.bset, self.gset = rn.RnsGadgetKeySet(self.bgk, Bd), rn.RnsGadgetKeySet(self.ggk, Bd)
        self.d = rn.RnsPoly.from_channels(self.diag, Bd)
        self.d.to_ntt_domain()
        self.ct = rn.Ciphertext(rn.RnsPoly.from_channels(self.c0, Bd), rn.RnsPoly.from_channels(self.c1, Bd))

    def run(self, out=None):
        return self.rn.linear_transform_bsgs(self.ct, self.d, self.bset, self.gset, out=out)

    def composed(self):
        """The library's own composition: rotate_ciphertext, product, add."""
        rn, ct = self.rn, self.ct
        n1 = len(self.baby)
        rot = [ct if k == 0 else rn.rotate_ciphertext(ct, self.bgk[i]) for i, k in enumerate(self.baby)]
        acc = None
        for j, g in enumerate(self.giant):
            v = None
            for i in range(n1):
                m = rn.RnsPoly.from_channels(
                    np.broadcast_to(self.diag[j * n1 + i], (self.B, self.L, self.n)).copy(), self.basis)
                p0, p1 = rot[i].c0 * m, rot[i].c1 * m
                v = (p0, p1) if v is None else (v[0] + p0, v[1] + p1)
            vc = rn.Ciphertext(v[0], v[1])
            r = vc if g == 0 else rn.rotate_ciphertext(vc, self.ggk[j])
            acc = (r.c0, r.c1) if acc is None else (acc[0] + r.c0, acc[1] + r.c1)
        return acc[0].channels(), acc[1].channels()

    def reference(self, p):
        Bo = orc.Basis(self.mod, self.n)
        return bsgs_ref(Bo, self.c0[p], self.c1[p], self.baby, self.giant, self.diag, self.bkeys, self.gkeys,
                        threads=T)


def _check_parity(c, ref_polys=None):
    out = c.run()
    g0, g1 = out.c0.channels(), out.c1.channels()
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    w0, w1 = c.composed()
    assert np.array_equal(g0, w0) and np.array_equal(g1, w1), "differs from the library's composition"
    for p in sorted({0, c.B - 1}) if ref_polys is None else ref_polys:
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from bsgs_ref"
    return g0, g1


@pytest.mark.parametrize("log_n,L,B,bits,ws_mb,edge,steps", [
    (8, 3, 3, 31, None, False, None),    # small four-step grid
    (8, 3, 3, 31, None, True, None),     # the same with all-(q-1) operands
    (14, 3, 3, 31, "1", False, None),    # three one-ciphertext chunks: chunk-local blocks
    (12, 3, 2, 61, None, False, None),   # u64 kernels
    (14, 2, 2, 61, None, False, None),   # u64 rows of 128 words
    (16, 4, 2, 31, None, False, SMALL),  # the matrix-core ring's transforms
    (17, 4, 1, 31, None, False, SMALL),  # the KSPLIT instantiation
    (12, 3, 2, 31, None, False, None),   # whole-plane: the composition inside the call
])
def test_bsgs_parity(gpu, monkeypatch, log_n, L, B, bits, ws_mb, edge, steps):
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    baby, giant = steps or (BABY, GIANT)
    _check_parity(Case(gpu, log_n, L, B, bits, baby=baby, giant=giant, edge=edge),
                  ref_polys=[0] if log_n >= 16 else None)


@pytest.mark.parametrize("baby,giant", [
    ([1, 2], [3, 5]),   # no zero anywhere: no addend, no copy
    ([1, 0], [2, 0]),   # the zero not first
    ([2], [0, 3, -1]),  # n1 = 1
])
def test_bsgs_step_sets(gpu, baby, giant):
    _check_parity(Case(gpu, 8, 3, 3, 31, baby=baby, giant=giant, seed=len(baby) + 7 * len(giant)))


def test_bsgs_one_zero_giant_is_linear_transform(gpu):
    """n2 = 1, g = [0]: the words of rnt_ct_linear on steps = baby."""
    c = Case(gpu, 8, 3, 3, 31, baby=BABY, giant=[0], seed=5)
    g0, g1 = _check_parity(c)
    lt = c.rn.linear_transform(c.ct, c.d, c.bset)
    assert np.array_equal(g0, lt.c0.channels()) and np.array_equal(g1, lt.c1.channels())


def test_bsgs_key_switch_count(gpu):
    """12 diagonals as 4 x 3 in one chunk: a decomposition and a rows launch per
    nonzero step, 3 + 2, where rnt_ct_linear runs 11; the inner sums take at
    most 2 n2 launches."""
    c = Case(gpu, 14, 3, 2, 31, baby=[0, 1, 2, 3], giant=[0, 4, 8])
    rn = c.rn
    c.run()  # warm: workspaces cached
    c.basis.profile_enable(True)
    c.run()
    counts = {k: c.basis.profile_read(k)[0] for k in ("ks_rows", "ks_decompose", "bsgs_mac", "col_inv")}
    c.basis.profile_enable(False)
    # the same 12 diagonals, one term each
    steps = [g + b for g in c.giant for b in c.baby]
    rng = np.random.default_rng(9)
    gk = [None if k == 0 else rn.RnsGadgetKey.from_channels(_rand(rng, c.mod, c.n, c.L), _rand(rng, c.mod, c.n, c.L),
                                                            c.basis, rotation=k) for k in steps]
    keyset = rn.RnsGadgetKeySet(gk, c.basis)
    rn.linear_transform(c.ct, c.d, keyset)
    c.basis.profile_enable(True)
    rn.linear_transform(c.ct, c.d, keyset)
    flat = c.basis.profile_read("ks_rows")[0]
    c.basis.profile_enable(False)
    print(counts, "rnt_ct_linear ks_rows", flat)
    assert counts["ks_rows"] == 5
    assert counts["ks_decompose"] == 5
    assert 1 <= counts["bsgs_mac"] <= 6
    assert flat == 11


@pytest.mark.parametrize("log_n,L,B,bits", [(8, 3, 3, 31), (12, 3, 2, 31)])
def test_bsgs_in_place(gpu, log_n, L, B, bits):
    c = Case(gpu, log_n, L, B, bits)
    out = c.run()
    w0, w1 = out.c0.channels(), out.c1.channels()
    same = c.run(out=c.ct)
    assert same is c.ct
    assert np.array_equal(c.ct.c0.channels(), w0) and np.array_equal(c.ct.c1.channels(), w1)


@pytest.mark.parametrize("log_n,L,B,bits", [(14, 3, 2, 31), (12, 3, 2, 31)])
def test_bsgs_captured(gpu, log_n, L, B, bits):
    """Only device ops are queued: the call records into a graph; a replay
    leaves the eager output, and a replay after the input buffers changed
    leaves the eager output for the new input."""
    c = Case(gpu, log_n, L, B, bits)
    rn = c.rn
    eager = c.run()
    w0, w1 = eager.c0.channels(), eager.c1.channels()
    out = rn.Ciphertext(rn.RnsPoly(c.basis, B), rn.RnsPoly(c.basis, B))
    with c.basis.capture() as g:
        c.run(out=out)
    g.replay()
    c.basis.sync()
    assert np.array_equal(out.c0.channels(), w0) and np.array_equal(out.c1.channels(), w1)
    rng = np.random.default_rng(41)
    c.ct.c0.copy_polys(rn.RnsPoly.from_channels(_rand(rng, c.mod, c.n, B), c.basis))
    c.ct.c1.copy_polys(rn.RnsPoly.from_channels(_rand(rng, c.mod, c.n, B), c.basis))
    g.replay()
    c.basis.sync()
    n0, n1 = c.composed()
    assert not np.array_equal(n0, w0)
    assert np.array_equal(out.c0.channels(), n0) and np.array_equal(out.c1.channels(), n1)


def test_bsgs_errors(gpu):
    """Every validation rule of the entry point, with its status and fields."""
    c = Case(gpu, 8, 3, 2, 31, baby=[0, 1], giant=[0, 2, 3])
    rn, lib, Bd, L, B = c.rn, c.rn.load(), c.basis, c.L, c.B
    o0, o1 = rn.RnsPoly(Bd, B), rn.RnsPoly(Bd, B)
    baby, giant = (ctypes.c_int32 * 2)(0, 1), (ctypes.c_int32 * 3)(0, 2, 3)

    def call(out0=o0, out1=o1, c0=c.ct.c0, c1=c.ct.c1, bs=baby, n1=2, gs=giant, n2=3, diag=c.d,
             bka=c.bset.a, bkb=c.bset.b, gka=c.gset.a, gkb=c.gset.b):
        h = lambda x: None if x is None else x.handle  # noqa: E731
        return lib.rnt_ct_linear_bsgs(h(out0), h(out1), h(c0), h(c1), bs, n1, gs, n2, h(diag), h(bka), h(bkb),
                                      h(gka), h(gkb))

    def fails(kind, fields=None, **kw):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(call(**kw))
        assert e.value.kind == kind, (kind, kw.keys())
        if fields is not None:
            assert e.value.fields == fields

    def zeros(count, basis=Bd, ntt=True):
        return rn.RnsPoly.from_channels(np.zeros((count, L, c.n), np.uint64), basis, in_ntt_domain=ntt)

    rn.check(call())  # the valid call
    fails("BadArgument", bs=None)
    fails("BadArgument", gs=None)
    fails("BadArgument", n1=0)
    fails("BadArgument", n2=0)
    fails("BadArgument", diag=rn.RnsPoly.from_channels(c.diag[:5], Bd, in_ntt_domain=True))
    other = rn.RnsBasis(c.mod, c.n)
    fails("BasisMismatch", diag=rn.RnsPoly.from_channels(c.diag, other, in_ntt_domain=True))
    fails("BasisMismatch", c1=rn.RnsPoly.from_channels(c.c1, other))
    fails("BasisMismatch", out0=rn.RnsPoly(other, B))
    fails("BasisMismatch", bka=zeros(2 * L, other))
    fails("BasisMismatch", gkb=zeros(3 * L, other))
    fails("DomainMismatch", diag=rn.RnsPoly.from_channels(c.diag, Bd))
    ntt = c.ct.c0.clone()
    ntt.to_ntt_domain()
    fails("DomainMismatch", c0=ntt)
    fails("DomainMismatch", c1=ntt)
    # per stage: a nonzero step needs its keys, of the stage's own count, prepared
    fails("BadArgument", bka=None)
    fails("BadArgument", gkb=None)
    fails("ChannelCountMismatch", {"expected": 2 * L, "actual": 3 * L}, bka=c.gset.a)
    fails("ChannelCountMismatch", {"expected": 2 * L, "actual": L}, bkb=zeros(L))
    fails("ChannelCountMismatch", {"expected": 3 * L, "actual": 2 * L}, gka=c.bset.a)
    fails("ChannelCountMismatch", {"expected": 3 * L, "actual": L}, gkb=zeros(L))
    fails("DomainMismatch", bka=zeros(2 * L, ntt=False))
    fails("DomainMismatch", gka=zeros(3 * L, ntt=False))
    # aliasing: out0 == out1 and an output on another input
    fails("BadArgument", out1=o0)
    fails("BadArgument", out0=c.ct.c1)
    fails("BadArgument", out1=c.ct.c0)
    # a stage whose steps are all 0 runs without its key buffers
    z2, z3 = (ctypes.c_int32 * 2)(0, 0), (ctypes.c_int32 * 3)(0, 0, 0)
    rn.check(call(bs=z2, bka=None, bkb=None))
    rn.check(call(gs=z3, gka=None, gkb=None))
    rn.check(call(bs=z2, gs=z3, bka=None, bkb=None, gka=None, gkb=None))


def test_engine_linear_transform_bsgs_end_to_end(gpu):
    """Encode -> encrypt -> a 16-diagonal band (diagonals 0..15 as baby
    [0,1,2,3] x giant [0,4,8,12]) through CkksEngine.linear_transform_bsgs ->
    rescale -> decrypt -> decode at N = 64, 4 x 31-bit primes, ciphertext
    scale 2^58, diagonal scale 2^30, x and the entries uniform in (-1, 1).

    (a) The ciphertext equals the composed engine path word for word.
    (b) The slots match M_banded @ x.  The same pipeline on the CPU
    (tools/bsgs_tolerance.py: oracle/pyoracle, encoder.py, numpy draws,
    tests/bsgs_ref.py for the transform) decodes with a largest absolute error
    of 1.691e-5 over eight seeds (9.0e-6 .. 1.7e-5; max|y| 2.6 .. 4.8, i.e.
    3.3e-6 .. 5.7e-6 of max|y|, against the 1e-3 asked of the parameters).
    Tolerance: 4 x 1.691e-5 = 6.76e-5; the margin covers other random draws,
    the arithmetic being identical."""
    rn = gpu
    from rns_ntt.engine import CkksEngine

    n, slots, L = 64, 32, 4
    eng = CkksEngine(rn.generate_primes(31, L, n), n, error_std=3.2, hamming_weight=n // 2)
    rng = np.random.default_rng(78)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    baby, giant = [0, 1, 2, 3], [0, 4, 8, 12]
    bset = eng.generate_rotation_key_set(sk, baby, rng)
    gset = eng.generate_rotation_key_set(sk, giant, rng)
    x = rng.uniform(-1, 1, slots)
    M = np.zeros((slots, slots))
    s = np.arange(slots)
    for d in range(16):
        M[s, (s + d) % slots] = rng.uniform(-1, 1, slots)
    enc_x, enc_d = rn.CkksEncoder(n, 58), rn.CkksEncoder(n, 30)
    ct = eng.encrypt(enc_x.encode(x, eng.basis), pk, rng)
    diags = eng.encode_diagonals_bsgs(M, baby, giant, enc_d)
    assert diags.poly.n_polys == 16 and diags.poly.is_ntt_domain()
    out = CkksEngine.linear_transform_bsgs(ct, diags, bset, gset)
    assert out.logp == 58 + 30 and out.logq == ct.logq
    # (a) the composed engine path: rotate, coefficient-domain products, add, rotate, add
    dc = diags.poly.clone()
    dc.to_coeff_domain()
    dch = dc.channels()
    rot = [ct if k == 0 else CkksEngine.rotate_ciphertext(ct, _key_of(rn, bset, i, eng.basis))
           for i, k in enumerate(baby)]
    acc = None
    for j, g in enumerate(giant):
        v = None
        for i in range(len(baby)):
            m = rn.RnsPoly.from_channels(dch[j * len(baby) + i], eng.basis)
            p0, p1 = rot[i].c0 * m, rot[i].c1 * m
            v = (p0, p1) if v is None else (v[0] + p0, v[1] + p1)
        vc = rn.Ciphertext(v[0], v[1], out.logp, ct.logq)
        r = vc if g == 0 else CkksEngine.rotate_ciphertext(vc, _key_of(rn, gset, j, eng.basis))
        acc = (r.c0, r.c1) if acc is None else (acc[0] + r.c0, acc[1] + r.c1)
    assert np.array_equal(out.c0.channels(), acc[0].channels())
    assert np.array_equal(out.c1.channels(), acc[1].channels())
    # (b) rescale, decrypt, decode
    res = CkksEngine.rescale_ciphertext(out)
    pt = CkksEngine.decrypt_plaintext(res, CkksEngine.secret_on(sk, res.c0.basis))
    got = enc_x.decode(pt)
    y = M @ x
    err = float(np.max(np.abs(got - y)))
    print(f"bsgs linear transform decode error {err:.3e}, max|y| {np.max(np.abs(y)):.3f}")
    assert err <= 4 * 1.691e-5


def _key_of(rn, keyset, t, basis):
    """Step t's gadget key out of a packed set, as a key of its own (already
    NTT-resident: rnt_key_prepare leaves an NTT-domain buffer alone)."""
    L = basis.channel_count()
    a, b = rn.RnsPoly(basis, L), rn.RnsPoly(basis, L)
    a.copy_polys(keyset.a, 0, t * L, L)
    b.copy_polys(keyset.b, 0, t * L, L)
    return rn.RnsGadgetKey(a, b, keyset.steps[t])
