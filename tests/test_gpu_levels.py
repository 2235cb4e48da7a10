"""Every kernel path on drop_last views (levelled ciphertexts).

rnt_ctx_drop_last returns a prefix view that shares the root's device tables:
ctx->L shrinks while Tables::L, the [L][L] rescale tables, the twiddle and
LimbConst tables, the matrix-core tables and the external-rescale tables stay
those of the root ("What a drop_last view shares").  After the
first rescale every CKKS op runs on such a view, so each op family runs here
on views of depth 1 and 2 -- reached as root.drop_last(d) and as
root.drop_last(1).drop_last(1) -- on the smallest ring of every kernel family.

Arithmetic on a prefix of a basis is arithmetic on the basis of those moduli,
so each result is compared word for word (np.array_equal, integers only) with

1. the oracle on orc.Basis(mod[:Lv], n), first and last poly of the batch;
2. a fresh root context rn.RnsBasis(mod[:Lv], n) given the same host data,
   the whole batch (a consistency check; the oracle is the reference).

rnt_profile_read on the view's context shows which kernel served the call, so
a silent fallback cannot make a case pass for the wrong reason.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest

import encoder as enc
import pyoracle as orc
import sampler as smp
from test_gpu_bsgs import SMALL as BSGS_SMALL
from test_gpu_bsgs import Case as BsgsCase
from test_gpu_encoder import _assert_coeffs_match
from test_gpu_hoist import SMALL as HOIST_SMALL
from test_gpu_hoist import SMALL_BSGS as HOIST_BSGS_SMALL
from test_gpu_hoist import BsgsCase as HoistBsgsCase
from test_gpu_hoist import Case as HoistCase
from test_gpu_linear import Case as LinearCase
from test_gpu_parity import _centered_crt

pytestmark = pytest.mark.gpu

T = orc.host_threads()
KNOBS = ("RNT_PLANE", "RNT_MF_MUL", "RNT_KS_WS_MB", "RNT_ROT_FUSE", "RNT_KS_DIAG", "RNT_DEC_JG")

# name -> (log_n, ((bits, count), ...) of the root, batch, knobs)
RINGS = {
    "n8": (8, ((31, 4),), 3, {}),                 # small four-step grids
    "n12": (12, ((31, 4),), 3, {}),               # whole-plane rows, k_ks_whole, whole-plane tensor (u32)
    "n12_30": (12, ((30, 4),), 2, {}),            # the same, Harvey-lazy 30-bit arithmetic
    "n12_61": (12, ((61, 4),), 2, {}),            # u64 whole-plane rows and tensor
    "n13_61": (13, ((61, 4),), 2, {}),            # u64 whole-plane rows, four-step tensor and key-switch
    "n14": (14, ((31, 4),), 3, {}),               # tiled four-step, fused rescale, tensor diagonal, fused sigma(c0)
    "n14_ws1": (14, ((31, 4),), 3, {"RNT_KS_WS_MB": "1"}),  # one ciphertext per key-switch chunk
    "n14_61": (14, ((61, 3),), 2, {}),            # u64 tiled four-step, fused rescale
    "n16": (16, ((31, 4),), 2, {}),               # k_mf_ntt, k_mf_mul, k_mf_tensor
    "n17": (17, ((31, 4),), 1, {}),               # the KSPLIT instantiation
    "n12_wide": (12, ((31, 2), (40, 1)), 2, {}),  # u64 root tables, the view's moduli all fit 31 bits
    "n14_wide": (14, ((31, 2), (40, 1)), 2, {}),
    "n12_mix30": (12, ((30, 2), (31, 1)), 2, {}),  # root not lazy30-eligible, the view's moduli all 30-bit
}


def _root_len(ring):
    return sum(c for _, c in RINGS[ring][1])


def _cases(rings=None):
    """(ring, how): depth 1 and 2; depth 2 both ways on the 4-limb roots."""
    out = []
    for ring in rings or RINGS:
        out += [(ring, "d1"), (ring, "d2")]
        if _root_len(ring) == 4:
            out.append((ring, "d1d1"))
    return out


def root_moduli(rn, ring):
    log_n, spec, _, _ = RINGS[ring]
    mod = []
    for bits, count in spec:
        mod += rn.generate_primes(bits, count, 1 << log_n)
    return mod


def prefix_basis(mod, lv, n):
    """The high-precision reference of a view of `lv` limbs: the oracle's
    basis of the first `lv` moduli (host side, no device)."""
    return orc.Basis(list(mod[:lv]), n)


class Lvl:
    """A root, one view of it, and the view's two references."""

    def __init__(self, rn, ring, how, monkeypatch, env=None):
        log_n, _, self.B, knobs = RINGS[ring]
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in {**knobs, **(env or {})}.items():
            monkeypatch.setenv(k, v)  # read at rnt_ctx_create; the view inherits them
        self.rn, self.ring, self.how, self.log_n, self.n = rn, ring, how, log_n, 1 << log_n
        self.mod = root_moduli(rn, ring)
        self.L = len(self.mod)
        self.root = rn.RnsBasis(self.mod, self.n)
        self.view = self.drop(how)
        self.d = 1 if how == "d1" else 2
        self.Lv = self.L - self.d
        self.vmod = self.mod[:self.Lv]
        assert self.view.channel_count() == self.Lv and self.view.moduli() == self.vmod
        self.Bo = prefix_basis(self.mod, self.Lv, self.n)
        self.fresh = rn.RnsBasis(self.vmod, self.n)
        self.wide_root = max(self.mod).bit_length() > 32
        self.rng = np.random.default_rng(sum(map(ord, ring + how)) + 8100)

    def drop(self, how):
        """A new context handle of the same depth."""
        r = self.root
        return {"d1": lambda: r.drop_last(1), "d2": lambda: r.drop_last(2),
                "d1d1": lambda: r.drop_last(1).drop_last(1)}[how]()

    def rand(self, batch, mod=None):
        return orc.uniform_poly(self.vmod if mod is None else mod, self.n, self.rng, batch=batch)

    def batch(self, B=None):
        """[B][Lv][N], every poly distinct."""
        return self.rand(self.B if B is None else B)

    def picks(self, B=None):
        return sorted({0, (self.B if B is None else B) - 1})

    def chunks(self):
        """Key-switch chunks of the batch (ks_chunk: S = [Lv][Lv][Bc][N] words
        within RNT_KS_WS_MB; only the n14_ws1 row sets it, to 1 MiB)."""
        if self.ring != "n14_ws1":
            return 1
        bc = max(1, (1 << 20) // (self.Lv * self.Lv * self.n * 4))
        return -(-self.B // min(bc, self.B))

    def counts(self, fn, *names):
        """Launch counts of `names` on the view's context while fn() runs
        (after one warm call, as test_launch_counts does)."""
        fn()
        self.view.profile_enable(True)
        fn()
        got = {k: self.view.profile_read(k)[0] for k in names}
        self.view.profile_enable(False)
        print(self.ring, self.how, got)
        return got


@contextlib.contextmanager
def _raises(rn, kind, fields=None):
    with pytest.raises(rn.RnsNttError) as e:
        yield e
    assert e.value.kind == kind, (e.value.kind, kind)
    if fields is not None:
        assert e.value.fields == fields, (e.value.fields, fields)


def test_case_table():
    """CPU: every row of the ring table is present with its depths."""
    assert len(RINGS) == 13
    assert ("n12", "d1d1") in _cases() and ("n14_61", "d1d1") not in _cases() and ("n14_61", "d2") in _cases()


def test_prefix_basis_is_the_basis_of_the_prefix():
    """CPU: the reference of a view is the oracle's basis of the first Lv
    moduli -- a product there equals the first Lv limbs of the product on the
    full basis."""
    n = 64
    mod = orc.generate_primes(31, 4, n)
    rng = np.random.default_rng(5)
    a, b = orc.uniform_poly(mod, n, rng), orc.uniform_poly(mod, n, rng)
    full = orc.mul(orc.Basis(mod, n), a, b)
    for lv in (1, 2, 3):
        assert np.array_equal(orc.mul(prefix_basis(mod, lv, n), a[:lv], b[:lv]), full[:lv])


# ---------------------------------------------------------------------------
# 1. ring ops
# ---------------------------------------------------------------------------
def _autos(n):
    return (3, 5 ** 7, 2 * n - 1, 6, 2 * n)


def _ring_ops(rn, basis, a_h, b_h, x_h, small):
    """Every ring op on `basis`; name -> host result."""
    n = basis.degree
    out = {}
    a, b = rn.RnsPoly.from_channels(a_h, basis), rn.RnsPoly.from_channels(b_h, basis)
    ntt = a.clone()
    ntt.to_ntt_domain()
    assert ntt.is_ntt_domain()
    out["ntt"] = ntt.channels()  # natural-order download
    back = ntt.clone()
    back.to_coeff_domain()
    out["ntt_roundtrip"] = back.channels()
    up = rn.RnsPoly.from_channels(x_h, basis, in_ntt_domain=True)  # natural-order upload
    up.to_coeff_domain()
    out["ntt_upload_inv"] = up.channels()
    out["mul"] = (a * b).channels()
    t = a.clone()
    t *= b
    out["imul"] = t.channels()
    bn = b.clone()
    bn.to_ntt_domain()
    pn = ntt * bn
    assert pn.is_ntt_domain()
    out["mul_ntt"] = pn.channels()
    t = ntt.clone()
    t *= bn
    out["imul_ntt"] = t.channels()
    out["add"] = (a + b).channels()
    out["sub"] = (a - b).channels()
    out["neg"] = (-a).channels()
    for g in _autos(n):
        out[f"auto_{g}"] = a.automorphism(g).channels()
        r = ntt.automorphism(g)
        out[f"auto_ntt_{g}"] = r.channels()
        out[f"auto_ntt_flag_{g}"] = np.array(r.is_ntt_domain())
    for k in (1, -3):
        out[f"rot_{k}"] = a.rotate_slots(k).channels()
    if basis.channel_count() >= 2:
        r = a.rescale()
        assert r.basis.channel_count() == basis.channel_count() - 1 and not r.is_ntt_domain()
        out["rescale"] = r.channels()
        out["rescale_ntt"] = ntt.rescale().channels()
        out["mod_drop"] = a.mod_drop_last(1).channels()
    else:
        with _raises(rn, "InvalidModDrop", {"drop_count": 1, "channel_count": 1}):
            a.rescale()
        with _raises(rn, "InvalidModDrop", {"drop_count": 1, "channel_count": 1}):
            basis.drop_last(1)
        with _raises(rn, "InvalidModDrop", {"drop_count": 1, "channel_count": 1}):
            rn.check(rn.load().rnt_rescale(rn.RnsPoly(basis, a.n_polys).handle, a.handle))
    out["clone"] = a.clone().channels()
    out["to_coeffs"] = np.asarray(a.to_coeffs())
    out["to_coeffs_ntt"] = np.asarray(ntt.to_coeffs())
    out["exact"] = a.to_coeffs_exact()
    out["coeffs_identity"] = np.asarray(rn.RnsPoly.from_coeffs(small, basis).to_coeffs())
    return out


@pytest.mark.parametrize("ring,how", _cases())
def test_ring_ops_on_view(gpu, monkeypatch, ring, how):
    rn = gpu
    v = Lvl(rn, ring, how, monkeypatch)
    n, B, Bo, q = v.n, v.B, v.Bo, np.array(v.vmod, dtype=np.uint64)[:, None]
    a_h, b_h, x_h = v.batch(), v.batch(), v.batch()
    small = v.rng.integers(-(1 << 20), 1 << 20, size=(B, n), dtype=np.int64)
    small[:, :3] = [0, 1, -1]
    got = _ring_ops(rn, v.view, a_h, b_h, x_h, small)
    # 2. the fresh context of the same moduli, the whole batch
    ref = _ring_ops(rn, v.fresh, a_h, b_h, x_h, small)
    assert got.keys() == ref.keys()
    for name in got:
        if name == "exact":
            assert got[name] == ref[name], name
        else:
            assert np.array_equal(got[name], ref[name]), f"{name}: view differs from the fresh context"
    # 1. the oracle on the prefix basis
    assert np.array_equal(got["ntt_roundtrip"], a_h) and np.array_equal(got["clone"], a_h)
    assert np.array_equal(got["imul"], got["mul"]) and np.array_equal(got["imul_ntt"], got["mul_ntt"])
    assert np.array_equal(got["coeffs_identity"], small)
    assert np.array_equal(got["to_coeffs_ntt"], got["to_coeffs"])
    if v.Lv >= 2:
        assert np.array_equal(got["mod_drop"], a_h[:, :v.Lv - 1])
    for p in v.picks():
        a, b = a_h[p], b_h[p]
        an = orc.to_ntt(Bo, a)
        assert np.array_equal(got["ntt"][p], an), p
        assert np.array_equal(got["ntt_upload_inv"][p], orc.to_coeff(Bo, x_h[p])), p
        assert np.array_equal(got["mul"][p], orc.mul(Bo, a, b)), p
        assert np.array_equal(got["mul_ntt"][p], orc.mul(Bo, an, orc.to_ntt(Bo, b), ntt=True)), p
        assert np.array_equal(got["add"][p], orc.add(Bo, a, b)), p
        assert np.array_equal(got["sub"][p], (a + q - b) % q), p
        assert np.array_equal(got["neg"][p], orc.neg(Bo, a)), p
        for g in _autos(n):
            assert np.array_equal(got[f"auto_{g}"][p], orc.automorphism(Bo, a, g)[0]), (g, p)
            want, flag = orc.automorphism(Bo, an, g, in_ntt=True)
            assert np.array_equal(got[f"auto_ntt_{g}"][p], want), (g, p)
            assert bool(got[f"auto_ntt_flag_{g}"]) == flag
        for k in (1, -3):
            assert np.array_equal(got[f"rot_{k}"][p], orc.rotate_slots(Bo, a, k)[0]), (k, p)
        if v.Lv >= 2:
            want = orc.rescale(Bo, a)  # reads rescale-table row Lv-1 at the root's stride
            assert np.array_equal(got["rescale"][p], want) and np.array_equal(got["rescale_ntt"][p], want), p
        for i in v.rng.integers(0, n, size=64):
            x = _centered_crt(v.vmod, a[:, i])
            assert got["exact"][p][i] == x, (p, i)
            lo = x & ((1 << 64) - 1)
            assert int(got["to_coeffs"][p][i]) == (lo - (1 << 64) if lo >> 63 else lo), (p, i)
    # which kernels served the view
    a, b = rn.RnsPoly.from_channels(a_h, v.view), rn.RnsPoly.from_channels(b_h, v.view)
    c = v.counts(lambda: a * b, "whole_mul", "mf_mul", "plane_fused", "row_mul")
    want = "whole_mul" if 10 <= v.log_n <= 14 else "mf_mul" if v.log_n == 16 else "row_mul"
    assert c[want] == 1 and sum(c.values()) == 1, c
    t = a.clone()

    def fwd_inv():
        t.to_ntt_domain()
        t.to_coeff_domain()

    c = v.counts(fwd_inv, "whole_fwd", "whole_inv", "mf_ntt_fwd", "mf_ntt_inv", "col_fwd", "col_inv")
    want = ("whole_fwd", "whole_inv") if 10 <= v.log_n <= 14 else \
        ("mf_ntt_fwd", "mf_ntt_inv") if v.log_n == 16 else ("col_fwd", "col_inv")
    assert c[want[0]] == 1 and c[want[1]] == 1 and sum(c.values()) == 2, c  # no other family ran


@pytest.mark.parametrize("env,kernel", [({"RNT_MF_MUL": "0"}, "plane_fused"), ({"RNT_PLANE": "0"}, "row_mul")])
@pytest.mark.parametrize("how", ["d1", "d2", "d1d1"])
def test_product_paths_at_2_16_on_view(gpu, monkeypatch, how, env, kernel):
    """rnt_mul at N = 2^16 on a view through the VALU whole-plane product
    (RNT_MF_MUL=0) and the four-step kernels (RNT_PLANE=0), both forms."""
    rn = gpu
    v = Lvl(rn, "n16", how, monkeypatch, env)
    a_h, b_h = v.batch(), v.batch()
    outs = []
    for basis in (v.view, v.fresh):
        a, b = rn.RnsPoly.from_channels(a_h, basis), rn.RnsPoly.from_channels(b_h, basis)
        outs.append((a * b).channels())
        a *= b
        assert np.array_equal(a.channels(), outs[-1])
    assert np.array_equal(outs[0], outs[1])
    for p in v.picks():
        assert np.array_equal(outs[0][p], orc.mul(v.Bo, a_h[p], b_h[p])), p
    a, b = rn.RnsPoly.from_channels(a_h, v.view), rn.RnsPoly.from_channels(b_h, v.view)
    c = v.counts(lambda: a * b, "whole_mul", "mf_mul", "plane_fused", "row_mul")
    assert c[kernel] == 1 and sum(c.values()) == 1, c


# ---------------------------------------------------------------------------
# 2. upload contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring,how", _cases(["n8", "n12", "n12_61", "n12_wide", "n14"]))
def test_upload_contract_on_view(gpu, monkeypatch, ring, how):
    rn = gpu
    v = Lvl(rn, ring, how, monkeypatch)
    n, Lv = v.n, v.Lv
    over = orc.uniform_poly(v.mod[:Lv + 1], n, v.rng, batch=2)
    with _raises(rn, "ChannelCountMismatch", {"expected": Lv, "actual": Lv + 1}):
        rn.RnsPoly.from_channels(over, v.view)
    bad = v.batch(3)
    q = v.vmod[Lv - 1]
    bad[1, Lv - 1, 5] = q  # the last limb of the second poly
    with _raises(rn, "NonReducedCoefficient", {"coefficient": q, "modulus": q}):
        rn.RnsPoly.from_channels(bad, v.view)
    bad[1, Lv - 1, 5] = q - 1  # the largest reduced value is accepted
    assert np.array_equal(rn.RnsPoly.from_channels(bad, v.view).channels(), bad)
    x_h = v.batch()
    x, y = rn.RnsPoly.from_channels(x_h, v.view), rn.RnsPoly.from_channels(x_h, v.fresh)
    for other in (y, rn.RnsPoly.from_channels(x_h, v.drop(how))):  # equal moduli, another handle
        with _raises(rn, "BasisMismatch"):
            x + other
        with _raises(rn, "BasisMismatch"):
            x * other
    if v.L - v.d - 2 >= 1:
        with _raises(rn, "BasisMismatch"):
            x.rescale_into(v.root.drop_last(v.d + 2))
    if Lv >= 2:
        with _raises(rn, "BasisMismatch"):
            x.rescale_into(v.fresh.drop_last(1))
        with _raises(rn, "BasisMismatch"):
            x.rescale_into(v.view)


# ---------------------------------------------------------------------------
# 3. key-switch family
# ---------------------------------------------------------------------------
def _ks_family(rn, basis, h):
    """keyswitch, ct-mul, rescale, fused ct-mul + rescale and two rotations
    on `basis` from the host data `h`; name -> (out0, out1) host arrays."""
    up = lambda x: rn.RnsPoly.from_channels(x, basis)  # noqa: E731
    rlk = rn.RnsGadgetKey.from_channels(h["ka"], h["kb"], basis)
    tb = basis.total_bits()
    ct1 = rn.Ciphertext(up(h["c0"]), up(h["c1"]), 31, tb)
    ct2 = rn.Ciphertext(up(h["c0p"]), up(h["c1p"]), 31, tb)
    out = {}
    a0, a1 = rn.keyswitch(up(h["c1"]), rlk)
    out["ks"] = (a0.channels(), a1.channels())
    m = rn.mul_ciphertexts_gadget(ct1, ct2, rlk)
    out["mul"] = (m.c0.channels(), m.c1.channels())
    if basis.channel_count() >= 2:
        r = rn.rescale_ciphertext(m)
        f = rn.mul_ciphertexts_gadget_rescale(ct1, ct2, rlk)
        assert f.c0.basis.channel_count() == basis.channel_count() - 1
        assert (f.logp, f.logq) == (r.logp, r.logq)
        out["rescale"] = (r.c0.channels(), r.c1.channels())
        out["fused"] = (f.c0.channels(), f.c1.channels())
    else:
        for fn in (lambda: rn.rescale_ciphertext(m), lambda: rn.mul_ciphertexts_gadget_rescale(ct1, ct2, rlk)):
            with _raises(rn, "InvalidModDrop", {"drop_count": 1, "channel_count": 1}):
                fn()
    for k in (1, -3):
        rotk = rn.RnsGadgetKey.from_channels(h["ra"], h["rb"], basis, rotation=k)
        r = rn.rotate_ciphertext(ct1, rotk)
        out[f"rot_{k}"] = (r.c0.channels(), r.c1.channels())
    return out


def _ks_host(v):
    h = {k: v.batch() for k in ("c0", "c1", "c0p", "c1p")}
    for k in ("ka", "kb", "ra", "rb"):
        h[k] = v.rand(v.Lv)  # [Lv][Lv][N]: a key of the view's level
    return h


def _ks_check_oracle(v, h, got):
    Bo = v.Bo
    for p in v.picks():
        w = orc.keyswitch(Bo, h["c1"][p], h["ka"], h["kb"], threads=T)
        assert np.array_equal(got["ks"][0][p], w[0]) and np.array_equal(got["ks"][1][p], w[1]), p
        w = orc.mul_ciphertexts_gadget(Bo, h["c0"][p], h["c1"][p], h["c0p"][p], h["c1p"][p], h["ka"], h["kb"],
                                       threads=T)
        assert np.array_equal(got["mul"][0][p], w[0]) and np.array_equal(got["mul"][1][p], w[1]), p
        if v.Lv >= 2:
            for o in (0, 1):
                want = orc.rescale(Bo, w[o])
                assert np.array_equal(got["rescale"][o][p], want), (p, o)
                assert np.array_equal(got["fused"][o][p], want), (p, o)
        for k in (1, -3):
            w = orc.rotate_ciphertext(Bo, h["c0"][p], h["c1"][p], k, h["ra"], h["rb"], threads=T)
            assert np.array_equal(got[f"rot_{k}"][0][p], w[0]), (k, p)
            assert np.array_equal(got[f"rot_{k}"][1][p], w[1]), (k, p)


@pytest.mark.parametrize("ring,how", _cases())
def test_keyswitch_family_on_view(gpu, monkeypatch, ring, how):
    rn = gpu
    v = Lvl(rn, ring, how, monkeypatch)
    h = _ks_host(v)
    got = _ks_family(rn, v.view, h)
    ref = _ks_family(rn, v.fresh, h)
    assert got.keys() == ref.keys()
    for name in got:
        for o in (0, 1):
            assert np.array_equal(got[name][o], ref[name][o]), f"{name} out{o}: view differs from the fresh context"
    if v.Lv >= 2:  # the fused op equals the two calls word for word
        assert np.array_equal(got["fused"][0], got["rescale"][0]) and np.array_equal(got["fused"][1], got["rescale"][1])
    _ks_check_oracle(v, h, got)
    # which kernels served the view
    up = lambda x: rn.RnsPoly.from_channels(x, v.view)  # noqa: E731
    rlk = rn.RnsGadgetKey.from_channels(h["ka"], h["kb"], v.view)
    ct1, ct2 = rn.Ciphertext(up(h["c0"]), up(h["c1"])), rn.Ciphertext(up(h["c0p"]), up(h["c1p"]))
    names = ("ks_whole", "ks_rows", "tensor_whole", "tensor_rows", "mf_tensor", "rescale", "col_inv")
    c = v.counts(lambda: rn.mul_ciphertexts_gadget(ct1, ct2, rlk), *names)
    u32 = not v.wide_root
    ks_whole = u32 and 10 <= v.log_n <= 13
    tensor = "tensor_whole" if 10 <= v.log_n <= (13 if u32 else 12) else "mf_tensor" if v.log_n == 16 else "tensor_rows"
    chunks = v.chunks()
    assert (c["ks_whole"] > 0) == ks_whole and (c["ks_rows"] > 0) == (not ks_whole), c
    assert c[tensor] == chunks and c["tensor_whole"] + c["tensor_rows"] + c["mf_tensor"] == chunks, c
    if v.Lv >= 2:
        c = v.counts(lambda: rn.mul_ciphertexts_gadget_rescale(ct1, ct2, rlk), *names)
        if v.log_n >= 14:  # the rescale is the key-switch inverse's epilogue: no launch of its own
            assert c["rescale"] == 0 and c["col_inv"] > 0 and c["ks_rows"] == chunks, c
        elif ks_whole:  # the two-op fallback
            assert c["rescale"] > 0 and c["ks_whole"] > 0, c
    # a key of another context is refused, not read
    key_l = rn.RnsPoly.from_channels(v.rand(v.L, v.mod), v.root)
    foreign = [rn.RnsGadgetKey(key_l, key_l.clone(), rotation=1),
               rn.RnsGadgetKey.from_channels(h["ka"], h["kb"], v.drop(how), rotation=1),
               rn.RnsGadgetKey.from_channels(h["ka"], h["kb"], v.fresh, rotation=1)]
    for key in foreign:
        for fn in (lambda: rn.keyswitch(ct1.c1, key), lambda: rn.mul_ciphertexts_gadget(ct1, ct2, key),
                   lambda: rn.rotate_ciphertext(ct1, key)):
            with _raises(rn, "BasisMismatch"):
                fn()
        if v.Lv >= 2:
            with _raises(rn, "BasisMismatch"):
                rn.mul_ciphertexts_gadget_rescale(ct1, ct2, key)


@pytest.mark.parametrize("how", ["d1", "d2", "d1d1"])
def test_rotation_fused_sigma_c0_on_view(gpu, monkeypatch, how):
    """rnt_ct_rotate at 2^14 on a view with sigma(c0) gathered inside the
    inverse column pass (RNT_ROT_FUSE=2) and by a launch of its own (0):
    equal words, and the oracle's."""
    rn = gpu
    outs = {}
    for fuse in ("2", "0"):
        v = Lvl(rn, "n14", how, monkeypatch, {"RNT_ROT_FUSE": fuse})  # same seed: same host data
        c0, c1, ra, rb = v.batch(), v.batch(), v.rand(v.Lv), v.rand(v.Lv)
        ct = rn.Ciphertext(rn.RnsPoly.from_channels(c0, v.view), rn.RnsPoly.from_channels(c1, v.view))
        for k in (1, -3):
            rotk = rn.RnsGadgetKey.from_channels(ra, rb, v.view, rotation=k)
            r = rn.rotate_ciphertext(ct, rotk)
            outs[fuse, k] = (r.c0.channels(), r.c1.channels())
            c = v.counts(lambda: rn.rotate_ciphertext(ct, rotk), "automorphism", "ks_rows")
            assert c["ks_rows"] == 1 and c["automorphism"] == (1 if fuse == "2" else 2), c  # sigma(c1) [, sigma(c0)]
    for k in (1, -3):
        assert np.array_equal(outs["2", k][0], outs["0", k][0]) and np.array_equal(outs["2", k][1], outs["0", k][1])
        for p in v.picks():
            w = orc.rotate_ciphertext(v.Bo, c0[p], c1[p], k, ra, rb, threads=T)
            assert np.array_equal(outs["2", k][0][p], w[0]) and np.array_equal(outs["2", k][1][p], w[1]), (k, p)


# ---------------------------------------------------------------------------
# 4. a level chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["n12", "n14", "n16"])
def test_level_chain(gpu, monkeypatch, ring):
    """Fused mul + rescale on the root, again on the view it returns with a
    key of that level, then a rotation and an addition one level deeper:
    every step against the oracle on the matching prefix basis."""
    rn = gpu
    v = Lvl(rn, ring, "d1", monkeypatch)
    n, L, B, mod = v.n, v.L, 2, v.mod
    picks = (0, B - 1)

    def fused_step(basis, lv, x0, x1):
        """(x0, x1) times a new ciphertext on `basis` (lv limbs), relinearised
        with a new lv-poly key and rescaled; the oracle's words per pick."""
        m = mod[:lv]
        Bo = prefix_basis(mod, lv, n)
        y0, y1 = v.rand(B, m), v.rand(B, m)
        ka, kb = v.rand(lv, m), v.rand(lv, m)
        key = rn.RnsGadgetKey.from_channels(ka, kb, basis)
        ct = rn.Ciphertext(rn.RnsPoly.from_channels(x0, basis), rn.RnsPoly.from_channels(x1, basis), 31, 31 * lv)
        ct2 = rn.Ciphertext(rn.RnsPoly.from_channels(y0, basis), rn.RnsPoly.from_channels(y1, basis), 31, 31 * lv)
        res = rn.mul_ciphertexts_gadget_rescale(ct, ct2, key)
        assert res.c0.basis.channel_count() == lv - 1 and res.c1.basis is res.c0.basis
        g0, g1 = res.c0.channels(), res.c1.channels()
        for p in picks:
            w = orc.mul_ciphertexts_gadget(Bo, x0[p], x1[p], y0[p], y1[p], ka, kb, threads=T)
            assert np.array_equal(g0[p], orc.rescale(Bo, w[0])), (lv, p)
            assert np.array_equal(g1[p], orc.rescale(Bo, w[1])), (lv, p)
        return res, g0, g1, (ct, ct2, key)

    x0, x1 = v.rand(B, mod), v.rand(B, mod)
    r1, g0, g1, _ = fused_step(v.root, L, x0, x1)          # root -> view L-1
    view1 = r1.c0.basis
    r2, g0, g1, args = fused_step(view1, L - 1, g0, g1)    # view L-1 -> view L-2
    names = ("tensor_whole", "tensor_rows", "mf_tensor", "ks_whole", "ks_rows", "rescale")
    c = v.counts(lambda: rn.mul_ciphertexts_gadget_rescale(*args), *names)
    if ring == "n12":
        assert c["tensor_whole"] == 1 and c["ks_whole"] == 1 and c["ks_rows"] == 0 and c["rescale"] > 0, c
    elif ring == "n14":
        assert c["tensor_rows"] == 1 and c["ks_rows"] == 1 and c["ks_whole"] == 0 and c["rescale"] == 0, c
    else:
        assert c["mf_tensor"] == 1 and c["ks_rows"] == 1 and c["ks_whole"] == 0 and c["rescale"] == 0, c
    view2, lv = r2.c0.basis, L - 2
    m, Bo = mod[:lv], prefix_basis(mod, lv, n)
    ra, rb = v.rand(lv, m), v.rand(lv, m)
    z0, z1 = v.rand(B, m), v.rand(B, m)
    for k in (1, -3):
        rot = rn.rotate_ciphertext(r2, rn.RnsGadgetKey.from_channels(ra, rb, view2, rotation=k))
        s0 = (rot.c0 + rn.RnsPoly.from_channels(z0, view2)).channels()
        s1 = (rot.c1 + rn.RnsPoly.from_channels(z1, view2)).channels()
        for p in picks:
            w = orc.rotate_ciphertext(Bo, g0[p], g1[p], k, ra, rb, threads=T)
            assert np.array_equal(s0[p], orc.add(Bo, w[0], z0[p])), (k, p)
            assert np.array_equal(s1[p], orc.add(Bo, w[1], z1[p])), (k, p)


# ---------------------------------------------------------------------------
# 5. linear transforms: Lv = 3 limbs of a 4-limb root
# ---------------------------------------------------------------------------
# (log_n, B, bits, RNT_KS_WS_MB); 2^16 and 2^17 run the SMALL step sets
LT_RINGS = [(8, 3, 31, None), (12, 2, 31, None), (12, 2, 61, None), (14, 3, 31, "1"), (16, 2, 31, None),
            (17, 1, 31, None)]


def _lt_pair(cls, rn, monkeypatch, log_n, B, bits, ws_mb, **kw):
    """The same case on a drop_last(1) view of four primes and on a fresh
    basis of the first three: equal seeds, so equal host data."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if ws_mb is not None:
        monkeypatch.setenv("RNT_KS_WS_MB", ws_mb)  # read at rnt_ctx_create
    c = cls(rn, log_n, 3, B, bits, drop=1, **kw)
    f = cls(rn, log_n, 3, B, bits, **kw)
    assert c.root.channel_count() == 4 and c.basis.channel_count() == 3 and c.basis is not c.root
    assert c.mod == f.mod and np.array_equal(c.c1, f.c1)
    return c, f


def _same(out, ref):
    g0, g1 = out.c0.channels(), out.c1.channels()
    assert not out.c0.is_ntt_domain() and not out.c1.is_ntt_domain()
    assert np.array_equal(g0, ref.c0.channels()) and np.array_equal(g1, ref.c1.channels()), \
        "view differs from the fresh context"
    return g0, g1


@pytest.mark.parametrize("log_n,B,bits,ws_mb", LT_RINGS)
def test_linear_transform_on_view(gpu, monkeypatch, log_n, B, bits, ws_mb):
    kw = {"steps": HOIST_SMALL} if log_n >= 16 else {}
    c, f = _lt_pair(LinearCase, gpu, monkeypatch, log_n, B, bits, ws_mb, **kw)
    g0, g1 = _same(c.rn.linear_transform(c.ct, c.d, c.keyset), f.rn.linear_transform(f.ct, f.d, f.keyset))
    for p in sorted({0, B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from linear_ref"


@pytest.mark.parametrize("log_n,B,bits,ws_mb", LT_RINGS)
def test_linear_transform_bsgs_on_view(gpu, monkeypatch, log_n, B, bits, ws_mb):
    kw = {"baby": BSGS_SMALL[0], "giant": BSGS_SMALL[1]} if log_n >= 16 else {}
    c, f = _lt_pair(BsgsCase, gpu, monkeypatch, log_n, B, bits, ws_mb, **kw)
    g0, g1 = _same(c.run(), f.run())
    for p in sorted({0, B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from bsgs_ref"


@pytest.mark.parametrize("log_n,B,bits,ws_mb", LT_RINGS)
def test_rotate_hoisted_on_view(gpu, monkeypatch, log_n, B, bits, ws_mb):
    kw = {"steps": HOIST_SMALL} if log_n >= 16 else {}
    c, f = _lt_pair(HoistCase, gpu, monkeypatch, log_n, B, bits, ws_mb, **kw)
    assert c.kset.hoisted and c.kset.a.n_polys == len(c.steps) * 3
    out = c.run()
    assert out.c0.n_polys == len(c.steps) * B
    g0, g1 = _same(out, f.run())
    for p in sorted({0, B - 1}):
        for t in range(len(c.steps)):
            r0, r1 = c.reference(p, t)
            assert np.array_equal(g0[t * B + p], r0), f"out0 of step {t} ({c.steps[t]}), ciphertext {p}"
            assert np.array_equal(g1[t * B + p], r1), f"out1 of step {t} ({c.steps[t]}), ciphertext {p}"
    if log_n == 14:  # the hoisted kernels ran on the view, not a per-step key-switch
        c.basis.profile_enable(True)
        c.run()
        counts = {k: c.basis.profile_read(k)[0] for k in ("ks_rows", "ks_decompose", "hoist_digits", "hoist_mac")}
        c.basis.profile_enable(False)
        assert counts["ks_rows"] == 0 and counts["ks_decompose"] == 0, counts
        assert counts["hoist_digits"] > 0 and counts["hoist_mac"] > 0, counts


@pytest.mark.parametrize("log_n,B,bits,ws_mb", LT_RINGS)
def test_linear_transform_bsgs_hoisted_on_view(gpu, monkeypatch, log_n, B, bits, ws_mb):
    kw = {"baby": HOIST_BSGS_SMALL[0], "giant": HOIST_BSGS_SMALL[1]} if log_n >= 16 else {}
    c, f = _lt_pair(HoistBsgsCase, gpu, monkeypatch, log_n, B, bits, ws_mb, **kw)
    g0, g1 = _same(c.run(), f.run())
    for p in sorted({0, B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from bsgs_hoisted_ref"


# ---------------------------------------------------------------------------
# 6. limb-sharded blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring,how", _cases(["n12", "n14"]))
def test_sharded_blocks_on_view(gpu, monkeypatch, ring, how):
    rn = gpu
    v = Lvl(rn, ring, how, monkeypatch)
    n, L, Lv, B = v.n, v.L, v.Lv, v.B
    Bo_root = orc.Basis(v.mod, n)
    # rnt_keyswitch_ext: the view's limbs as targets over all L source limbs
    d = v.rand(B, v.mod)                                  # [B][L][N] on the root
    ka, kb = v.rand(L, v.mod), v.rand(L, v.mod)           # [L][L][N]
    key = rn.RnsGadgetKey.from_channels(np.ascontiguousarray(ka[:, :Lv]), np.ascontiguousarray(kb[:, :Lv]), v.view)
    src = rn.RnsPoly.from_channels(d, v.root)
    ptr, wb = src.device_ptr()
    assert wb == 4
    a0, a1 = rn.keyswitch_ext(ptr, L, key, v.view, B)
    assert a0.basis is v.view
    g0, g1 = a0.channels(), a1.channels()
    for p in v.picks():
        w0, w1 = orc.keyswitch(Bo_root, d[p], ka, kb, threads=T)
        assert np.array_equal(g0[p], w0[:Lv]) and np.array_equal(g1[p], w1[:Lv]), p
    c = v.counts(lambda: rn.keyswitch_ext(ptr, L, key, v.view, B), "ks_whole", "ks_rows")
    assert (c["ks_whole"], c["ks_rows"]) == ((1, 0) if ring == "n12" else (0, 1)), c
    # rnt_rescale_ext by a modulus outside the view: a foreign prime, and the
    # root's limb Lv (in the shared tables, not in the view); every limb kept
    x_h = v.batch()
    x = rn.RnsPoly.from_channels(x_h, v.view)
    for q_last in (rn.generate_primes(31, L + 1, n)[L], v.mod[Lv]):
        assert q_last not in v.vmod
        xl = v.rand(B, [q_last])[:, 0]                    # [B][N] mod q_last
        last = rn.RnsPoly.from_channels(xl[:, None, :], rn.RnsBasis([q_last], n))
        lptr, lwb = last.device_ptr()
        assert lwb == 4
        got = rn.rescale_ext(x, lptr, q_last, v.view)
        assert got.basis is v.view
        gh = got.channels()
        Bx = orc.Basis(v.vmod + [q_last], n)
        for p in v.picks():
            assert np.array_equal(gh[p], orc.rescale(Bx, np.concatenate([x_h[p], xl[p][None]]))), (q_last, p)
    # rnt_rescale_ext by the view's own last limb: onto the deeper view
    xptr, _ = x.device_ptr()
    if Lv >= 2:
        deep = v.view.drop_last(1)
        got = rn.rescale_ext(x, xptr + (Lv - 1) * B * n * wb, v.vmod[-1], deep)
        assert got.basis.channel_count() == Lv - 1
        gh = got.channels()
        assert np.array_equal(gh, x.rescale().channels())
        for p in v.picks():
            assert np.array_equal(gh[p], orc.rescale(v.Bo, x_h[p])), p
        with _raises(rn, "BasisMismatch"):
            rn.rescale_ext(x, xptr + (Lv - 1) * B * n * wb, v.vmod[-1], v.view)
    else:
        with _raises(rn, "InvalidModDrop"):
            rn.rescale_ext(x, xptr, v.vmod[-1], v.view)


# ---------------------------------------------------------------------------
# 7. samplers and encoder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["d1", "d2", "d1d1"])
def test_samplers_on_view(gpu, monkeypatch, how):
    rn = gpu
    n = 1 << 10
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    mod = rn.generate_primes(31, 4, n)
    root = rn.RnsBasis(mod, n)
    view = {"d1": lambda: root.drop_last(1), "d2": lambda: root.drop_last(2),
            "d1d1": lambda: root.drop_last(1).drop_last(1)}[how]()
    vmod = view.moduli()
    assert vmod == mod[:len(vmod)]
    seed = 0x1234_5678_9ABC_DEF0
    rng = rn.DeviceRng(seed)
    rng.stream = 7
    got = rn.RnsPoly.sample_uniform(view, rng, n_polys=3).channels()
    assert got.shape == (3, len(vmod), n)
    assert np.array_equal(got, smp.uniform(vmod, n, 3, seed, 7))
    rng = rn.DeviceRng(42)
    p = rn.RnsPoly.sample_gaussian(3.2, view, rng, n_polys=2)
    ints = np.asarray(p.to_coeffs())
    want = smp.gaussian_ints(n, 2, 3.2, 42, 0)
    assert np.abs(ints - want).max() <= 1 and np.count_nonzero(ints - want) <= 2
    ch = p.channels()
    for limb in range(len(vmod)):
        assert np.array_equal(ch[:, limb], smp.residues(ints, vmod)[:, limb]), limb
    rng = rn.DeviceRng(99)
    rng.stream = 3
    p = rn.RnsPoly.sample_tribits(64, view, rng, n_polys=2)
    ints = np.asarray(p.to_coeffs()).reshape(2, n)
    assert np.array_equal(ints, smp.ternary_ints(n, 2, 64, 99, 3))
    assert np.array_equal(p.channels(), smp.residues(ints, vmod))


@pytest.mark.parametrize("how", ["d1", "d2", "d1d1"])
def test_encoder_on_view(gpu, monkeypatch, how):
    rn = gpu
    n = 1 << 10
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    mod = rn.generate_primes(31, 4, n)
    root = rn.RnsBasis(mod, n)
    view = {"d1": lambda: root.drop_last(1), "d2": lambda: root.drop_last(2),
            "d1d1": lambda: root.drop_last(1).drop_last(1)}[how]()
    vmod = view.moduli()
    rng = np.random.default_rng(10)
    scale = 30
    B, nv = 3, n // 2 - 3
    vals = rng.uniform(-4, 4, (B, nv)) + 1j * rng.uniform(-4, 4, (B, nv))
    e = rn.CkksEncoder(n, scale)
    pt = e.encode_complex(vals, view)
    assert pt.poly.basis is view and pt.poly.basis.channel_count() == len(vmod)
    got = np.asarray(pt.poly.to_coeffs())
    for p in range(B):
        _assert_coeffs_match(got[p], enc.encode_fft_real(vals[p], n, scale))
    ch = pt.poly.channels()
    for p in range(B):
        want = np.stack([np.asarray(got[p], dtype=object) % q for q in vmod]).astype(np.uint64)
        assert np.array_equal(ch[p], want), p
    z = e.decode_complex(pt)
    for p in range(B):
        want = enc.decode_fft(got[p], n, scale, nv)
        assert np.allclose(z[p], want, atol=1e-9 * np.max(np.abs(want)), rtol=0), p
    # decode of given integers below Q / 2 of the view (Q >= 2^30 at one limb)
    a = rng.integers(-(2 ** 28), 2 ** 28, (2, n))
    poly = rn.RnsPoly.from_coeffs(a, view)
    for slots in (n // 2, 3):
        z = rn.CkksEncoder(n, 25).decode_complex(rn.Plaintext(poly, 25, slots))
        for p in range(2):
            want = enc.decode_fft(a[p], n, 25, slots)
            assert np.allclose(z[p], want, atol=1e-9 * np.max(np.abs(want)), rtol=0), (slots, p)


# ---------------------------------------------------------------------------
# 8. lifetime and capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [1, 2])
def test_view_outlives_the_root_handle(gpu, drop):
    """The raw C-ABI: the root handle is destroyed before the view is used;
    the shared tables live as long as any handle or buffer (rnsntt.h)."""
    rn, lib = gpu, gpu.load()
    n, L, B = 1 << 12, 4, 2
    mod = rn.generate_primes(31, L, n)
    Lv = L - drop
    u64p = ctypes.POINTER(ctypes.c_uint64)
    arr = np.array(mod, dtype=np.uint64)
    root, view = ctypes.c_void_p(), ctypes.c_void_p()
    rn.check(lib.rnt_ctx_create(12, arr.ctypes.data_as(u64p), L, 0, ctypes.byref(root)))
    rn.check(lib.rnt_ctx_drop_last(root, drop, ctypes.byref(view)))
    rn.check(lib.rnt_ctx_destroy(root))
    bufs = [ctypes.c_void_p() for _ in range(3)]
    try:
        count = ctypes.c_size_t(0)
        rn.check(lib.rnt_ctx_channel_count(view, ctypes.byref(count)))
        assert count.value == Lv
        rng = np.random.default_rng(12 + drop)
        a_h, b_h = orc.uniform_poly(mod[:Lv], n, rng, batch=B), orc.uniform_poly(mod[:Lv], n, rng, batch=B)
        for b in bufs:
            rn.check(lib.rnt_buf_alloc(view, B, ctypes.byref(b)))
        rn.check(lib.rnt_upload(bufs[0], a_h.ctypes.data_as(u64p), B, Lv, 0))
        rn.check(lib.rnt_upload(bufs[1], b_h.ctypes.data_as(u64p), B, Lv, 0))
        rn.check(lib.rnt_mul(bufs[2], bufs[0], bufs[1]))
        out = np.zeros((B, Lv, n), dtype=np.uint64)
        rn.check(lib.rnt_download(bufs[2], out.ctypes.data_as(u64p), B))
        Bo = prefix_basis(mod, Lv, n)
        for p in range(B):
            assert np.array_equal(out[p], orc.mul(Bo, a_h[p], b_h[p])), p
        rn.check(lib.rnt_ntt_fwd(bufs[0]))
        rn.check(lib.rnt_download(bufs[0], out.ctypes.data_as(u64p), B))
        assert np.array_equal(out[B - 1], orc.to_ntt(Bo, a_h[B - 1]))
    finally:
        for b in bufs:
            if b.value:
                lib.rnt_buf_free(b)
        lib.rnt_ctx_destroy(view)


@pytest.mark.parametrize("ring", ["n12", "n14"])
def test_fused_mul_rescale_captured_on_view(gpu, monkeypatch, ring):
    """The fused mul + rescale on a view, once un-recorded and then recorded
    with view.capture(): two replays with changed input contents, each equal
    to the oracle for the contents it ran on."""
    rn = gpu
    v = Lvl(rn, ring, "d1", monkeypatch)
    B, lib = v.B, rn.load()
    h = _ks_host(v)
    up = lambda x: rn.RnsPoly.from_channels(x, v.view)  # noqa: E731
    rlk = rn.RnsGadgetKey.from_channels(h["ka"], h["kb"], v.view)
    c0, c1, c0p, c1p = up(h["c0"]), up(h["c1"]), up(h["c0p"]), up(h["c1p"])
    deep = v.view.drop_last(1)
    out0, out1 = rn.RnsPoly(deep, B), rn.RnsPoly(deep, B)

    def call():
        rn.check(lib.rnt_ct_mul_relin_rescale(out0.handle, out1.handle, c0.handle, c1.handle, c0p.handle,
                                              c1p.handle, rlk.a.handle, rlk.b.handle))

    def check(x0, x1):
        g0, g1 = out0.channels(), out1.channels()
        for p in v.picks():
            w = orc.mul_ciphertexts_gadget(v.Bo, x0[p], x1[p], h["c0p"][p], h["c1p"][p], h["ka"], h["kb"], threads=T)
            assert np.array_equal(g0[p], orc.rescale(v.Bo, w[0])), p
            assert np.array_equal(g1[p], orc.rescale(v.Bo, w[1])), p
        return g0

    call()  # un-recorded: workspaces cached
    first = check(h["c0"], h["c1"])
    with v.view.capture() as g:
        call()
    prev = first
    for _ in range(2):
        n0, n1 = v.batch(), v.batch()
        c0.copy_polys(up(n0))
        c1.copy_polys(up(n1))
        g.replay()
        v.view.sync()
        now = check(n0, n1)
        assert not np.array_equal(now, prev)
        prev = now
