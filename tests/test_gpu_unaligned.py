"""Every op family on buffers that are only word-aligned.

rnt_buf_wrap accepts any device pointer aligned to the context's word width
(include/rnsntt.h).  A slice of a larger allocation -- a collective's staging
buffer, a torch tensor at an offset -- gives planes that are 4- or 8-byte
aligned and no more.  The library meets them in two ways ("Alignment
of caller planes"): launchers that test the pointers and pick a one-word
instantiation, and kernels that issue 16-byte accesses to caller planes with no
test.  Each family runs here on views that start ONE WORD PAST a 16-byte
boundary (% 16 == 4 for u32, == 8 for u64), between two guard regions of a
sentinel that is no reduced residue; every case asserts the % 16 of every view
it shifted, so no case can pass on the aligned instantiations.

Reference: word for word (np.array_equal) the oracle on orc.Basis(mod, n) --
tests/lincomb_ref.py for the lincomb family, the linear and BSGS families'
own references (tests/lt_ref.py, tests/bsgs_ref.py through their Case
classes) -- on the first and the last poly; the library's aligned result on
the whole batch is an extra, never the reference.  Inputs: poly 0 uniform, the
last poly all-(q - 1).  rnt_profile_read names the kernel family that served
each call.

What stays out, and why:
* k_elementwise's op 4 (the bare Montgomery product): no entry point passes
  op 4 to launch_elementwise (rnt_mul passes 3, rnt_add / rnt_sub 0 / 1,
  rnt_neg 2, the internal add_assign 0).
* The one-word forms of k_bcast_mul KIND 0 and of k_bsgs_mac: every call hands
  them library workspace alone (the products' planes, the Montgomery-form
  plaintexts), which is 16-byte aligned whatever the caller wrapped.  KIND 1
  reads the caller's plaintext planes and runs here in its one-word form.
* The one-word form of k_dot_tensor, for the same reason.
No hook is added to reach them.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import encoder as enc
import pyoracle as orc
import sampler as smp
from test_gpu_bsgs import Case as BsgsCase
from test_gpu_encoder import _assert_coeffs_match
from test_gpu_levels import KNOBS, RINGS, root_moduli
from test_gpu_lincomb import Case as LincombCase
from test_gpu_linear import Case as LinearCase

pytestmark = pytest.mark.gpu

T = orc.host_threads()
SENTINEL = 0xA5A5A5A5  # above every 31-bit q; doubled, above every 61-bit q
U64P = ctypes.POINTER(ctypes.c_uint64)
BAD_ARGUMENT = 11

ALL_RINGS = ["n8", "n12", "n12_30", "n12_61", "n14", "n14_61", "n16", "n17"]
# n16 again on the VALU whole-plane product and on the four-step kernels
N16_KNOBS = [("n16", {"RNT_MF_MUL": "0"}), ("n16", {"RNT_PLANE": "0"})]
RING_ENVS = [(r, {}) for r in ALL_RINGS] + N16_KNOBS


def _ids(cases):
    return [r + "".join(f"-{k}={v}" for k, v in env.items()) for r, env in cases]


def _word_bytes(rn, basis):
    wb = basis.__dict__.get("_word_bytes")
    if wb is None:
        wb = basis.__dict__["_word_bytes"] = rn.RnsPoly(basis, 1).device_ptr()[1]
    return wb


def shifted(rn, basis, host_channels_or_src, ntt=False):
    """A view of `basis` one word past a 16-byte boundary, inside a torch
    tensor whose every other byte holds SENTINEL.  `host_channels_or_src` is
    host residues [B][L][N] (rnt_upload, in the NTT domain with `ntt`), an
    RnsPoly (rnt_copy_polys; its domain) or a poly count (an output: its own
    words start as the sentinel too, so a word the op never wrote shows).
    The view's check_guards() asserts that the 16 + word bytes before it and
    the bytes after its last word still hold the sentinel."""
    import torch

    src = host_channels_or_src
    if isinstance(src, (int, np.integer)):
        n_polys = int(src)
    elif isinstance(src, rn.RnsPoly):
        n_polys, ntt = src.n_polys, src.is_ntt_domain()
    else:
        src = np.ascontiguousarray(src, dtype=np.uint64)
        assert src.ndim == 3 and src.shape[1:] == (basis.channel_count(), basis.degree)
        n_polys = src.shape[0]
    wb = _word_bytes(rn, basis)
    words = n_polys * basis.channel_count() * basis.degree
    lead, body = 4 + wb // 4, words * wb // 4
    dev = torch.device("cuda", basis.device)
    t = torch.full((body + 8,), int(np.uint32(SENTINEL).astype(np.int32)), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    assert t.data_ptr() % 16 == 0
    v = rn.RnsPoly.wrap(basis, t.data_ptr() + 16 + wb, n_polys, in_ntt_domain=ntt, owner=t)
    assert v.device_ptr() == (t.data_ptr() + 4 * lead, wb)
    if isinstance(src, rn.RnsPoly):
        v.copy_polys(src)
    elif isinstance(src, np.ndarray):
        rn.check(rn.load().rnt_upload(v.handle, src.ctypes.data_as(U64P), n_polys, src.shape[1], 1 if ntt else 0))
    assert v.device_ptr()[0] % 16 == wb

    def check_guards():
        basis.sync()
        torch.cuda.synchronize(dev)
        want = np.uint32(SENTINEL)
        before = t[:lead].cpu().numpy().view(np.uint32)
        after = t[lead + body:].cpu().numpy().view(np.uint32)
        assert after.size == 4 - wb // 4
        assert np.all(before == want), f"words below the view were written: {before}"
        assert np.all(after == want), f"words past the view were written: {after}"

    v.check_guards = check_guards
    v.check_guards()
    return v


def guards(*views):
    for v in views:
        v.check_guards()


class Ring:
    """One root ring of test_gpu_levels.RINGS, its oracle basis and inputs."""

    def __init__(self, rn, ring, monkeypatch, env=None):
        log_n, _, self.B, knobs = RINGS[ring]
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in {**knobs, **(env or {})}.items():
            monkeypatch.setenv(k, v)  # read at rnt_ctx_create
        self.rn, self.ring, self.env, self.log_n, self.n = rn, ring, dict(env or {}), log_n, 1 << log_n
        self.mod = root_moduli(rn, ring)
        self.L = len(self.mod)
        self.basis = rn.RnsBasis(self.mod, self.n)
        self.Bo = orc.Basis(self.mod, self.n)
        self.u32 = max(self.mod).bit_length() <= 32
        self.wb = 4 if self.u32 else 8
        assert _word_bytes(rn, self.basis) == self.wb
        self.q = np.array(self.mod, dtype=np.uint64)[:, None]
        self.rng = np.random.default_rng(sum(map(ord, ring)) + 9100)

    def batch(self, B=None, basis_mod=None):
        """[B][L][N]: poly 0 uniform, the last poly (of two or more) all q - 1."""
        mod = self.mod if basis_mod is None else basis_mod
        B = self.B if B is None else B
        x = orc.uniform_poly(mod, self.n, self.rng, batch=B)
        if B > 1:
            x[B - 1] = np.broadcast_to(np.array(mod, dtype=np.uint64)[:, None] - np.uint64(1), x.shape[1:])
        return x

    def rand(self, B):
        return orc.uniform_poly(self.mod, self.n, self.rng, batch=B)

    def picks(self, B=None):
        return sorted({0, (self.B if B is None else B) - 1})

    def sh(self, src, ntt=False, basis=None):
        v = shifted(self.rn, basis or self.basis, src, ntt)
        assert v.device_ptr()[0] % 16 == self.wb
        return v

    def up(self, x, ntt=False):
        return self.rn.RnsPoly.from_channels(x, self.basis, in_ntt_domain=ntt)

    def counts(self, fn, *names):
        """Launch counts of `names` on the ring's context while fn() runs."""
        self.basis.profile_enable(True)
        try:
            fn()
            got = {k: self.basis.profile_read(k)[0] for k in names}
        finally:
            self.basis.profile_enable(False)
        print(self.ring, self.env, got)
        return got

    # the kernel family test_gpu_levels expects on this ring
    def product_kernel(self):
        if self.env.get("RNT_PLANE") == "0":
            return "row_mul"
        if 10 <= self.log_n <= 14:
            return "whole_mul"
        if self.log_n == 16:
            return "plane_fused" if self.env.get("RNT_MF_MUL") == "0" else "mf_mul"
        return "row_mul"

    def transform_kernels(self):
        if self.env.get("RNT_PLANE") == "0":
            return ("col_fwd", "col_inv")
        if 10 <= self.log_n <= 14:
            return ("whole_fwd", "whole_inv")
        return ("mf_ntt_fwd", "mf_ntt_inv") if self.log_n == 16 else ("col_fwd", "col_inv")

    def ks_kernel(self):
        if self.env.get("RNT_PLANE") == "0":
            return "ks_rows"
        return "ks_whole" if self.u32 and 10 <= self.log_n <= 13 else "ks_rows"

    def tensor_kernel(self):
        if self.env.get("RNT_PLANE") == "0":
            return "tensor_rows"
        if 10 <= self.log_n <= (13 if self.u32 else 12):
            return "tensor_whole"
        return "mf_tensor" if self.log_n == 16 else "tensor_rows"


PRODUCTS = ("whole_mul", "mf_mul", "plane_fused", "row_mul")
TRANSFORMS = ("whole_fwd", "whole_inv", "mf_ntt_fwd", "mf_ntt_inv", "col_fwd", "col_inv")


def test_case_table():
    """CPU: the rings come from test_gpu_levels' table, every width among them."""
    assert set(ALL_RINGS) <= set(RINGS)
    assert {RINGS[r][1][0][0] for r in ALL_RINGS} == {30, 31, 61}
    assert RINGS["n17"][2] == 1 and RINGS["n16"][2] == 2


# ---------------------------------------------------------------------------
# the contract: word alignment, and nothing more
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["n8", "n12_61"])
def test_wrap_refuses_a_pointer_that_is_not_word_aligned(gpu, monkeypatch, ring):
    import torch

    rn = gpu
    r = Ring(rn, ring, monkeypatch)
    t = torch.zeros(r.B * r.L * r.n * r.wb // 4 + 8, dtype=torch.int32, device=torch.device("cuda", r.basis.device))
    base = t.data_ptr()
    assert base % 16 == 0
    for off in range(1, r.wb):  # u64: % 8 == 4 among them
        with pytest.raises(rn.RnsNttError) as e:
            rn.RnsPoly.wrap(r.basis, base + 16 + off, r.B, owner=t)
        assert e.value.code == BAD_ARGUMENT, (off, e.value)
    h = ctypes.c_void_p()
    assert rn.load().rnt_buf_wrap(r.basis.handle, ctypes.c_void_p(base + r.wb // 2), r.B, 0, ctypes.byref(h)) == BAD_ARGUMENT
    assert not h.value
    for off in (0, r.wb, 16 - r.wb):  # every word-aligned offset is accepted
        v = rn.RnsPoly.wrap(r.basis, base + off, r.B, owner=t)
        assert v.device_ptr() == (base + off, r.wb)


# ---------------------------------------------------------------------------
# 1. k_elementwise, ops 0..3
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ntt", [False, True], ids=["coeff", "ntt"])
@pytest.mark.parametrize("ring", ["n8", "n12_61"])
def test_elementwise_ops(gpu, monkeypatch, ring, ntt):
    """rnt_add / rnt_sub / rnt_neg in both domains and the pointwise rnt_mul
    (op 3, NTT-domain operands): every operand shifted, only the output, only
    b, and in place on a shifted a."""
    rn, lib = gpu, gpu.load()
    r = Ring(rn, ring, monkeypatch)
    a_h, b_h = r.batch(), r.batch()
    b_h[0, :, :5] = a_h[0, :, :5]  # a - b == 0 and a + b == 2 a among the words
    q = r.q
    want = {"add": (a_h + b_h) % q, "sub": (a_h + q - b_h) % q, "neg": (q - a_h) % q}
    ops = {"add": lambda o, a, b: lib.rnt_add(o.handle, a.handle, b.handle),
           "sub": lambda o, a, b: lib.rnt_sub(o.handle, a.handle, b.handle),
           "neg": lambda o, a, b: lib.rnt_neg(o.handle, a.handle)}
    if ntt:
        ops["mul"] = lambda o, a, b: lib.rnt_mul(o.handle, a.handle, b.handle)
        al = (r.up(a_h, True) * r.up(b_h, True)).channels()  # the aligned result, the whole batch
        want["mul"] = al
    a_al, b_al = r.up(a_h, ntt), r.up(b_h, ntt)
    a_sh, b_sh = r.sh(a_h, ntt), r.sh(b_h, ntt)
    for name, op in ops.items():
        places = {"all": lambda: (r.sh(r.B), a_sh, b_sh), "out": lambda: (r.sh(r.B), a_al, b_al),
                  "b": lambda: (rn.RnsPoly(r.basis, r.B), a_al, b_sh)}
        x = r.sh(a_h, ntt)
        places["in_place"] = lambda: (x, x, b_sh)
        for place, make in places.items():
            o, a, b = make()
            c = r.counts(lambda: rn.check(op(o, a, b)), "elementwise")
            assert c["elementwise"] == 1, (name, place, c)
            got = o.channels()
            assert o.is_ntt_domain() == ntt
            assert np.array_equal(got, want[name]), (name, place)
            for p in r.picks():
                ref = {"add": lambda: orc.add(r.Bo, a_h[p], b_h[p], ntt=ntt), "sub": lambda: want["sub"][p],
                       "neg": lambda: orc.neg(r.Bo, a_h[p]),
                       "mul": lambda: orc.mul(r.Bo, a_h[p], b_h[p], ntt=True)}[name]()
                assert np.array_equal(got[p], ref), (name, place, p)
            guards(*(v for v in (o, a, b) if hasattr(v, "check_guards")))
    assert np.array_equal(a_sh.channels(), a_h) and np.array_equal(b_sh.channels(), b_h)  # inputs never written


# ---------------------------------------------------------------------------
# 2. transforms in place
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring,env", RING_ENVS[:-2] + [N16_KNOBS[1]], ids=_ids(RING_ENVS[:-2] + [N16_KNOBS[1]]))
def test_transforms_in_place(gpu, monkeypatch, ring, env):
    rn = gpu
    r = Ring(rn, ring, monkeypatch, env)
    a_h = r.batch()
    v = r.sh(a_h)
    fwd, inv = r.transform_kernels()
    c = r.counts(v.to_ntt_domain, *TRANSFORMS)
    assert c[fwd] == 1 and sum(c.values()) == 1, c
    v.check_guards()
    assert v.is_ntt_domain()
    got = v.channels()
    for p in r.picks():
        assert np.array_equal(got[p], orc.to_ntt(r.Bo, a_h[p])), p
    al = r.up(a_h)
    al.to_ntt_domain()
    assert np.array_equal(got, al.channels())
    c = r.counts(v.to_coeff_domain, *TRANSFORMS)
    assert c[inv] == 1 and sum(c.values()) == 1, c
    v.check_guards()
    assert np.array_equal(v.channels(), a_h)
    # natural-order NTT-domain words uploaded into a shifted view, inverted in place
    w = r.sh(a_h, ntt=True)
    w.to_coeff_domain()
    w.check_guards()
    got = w.channels()
    for p in r.picks():
        assert np.array_equal(got[p], orc.to_coeff(r.Bo, a_h[p])), p


# ---------------------------------------------------------------------------
# 3. the coefficient-domain product
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring,env", RING_ENVS, ids=_ids(RING_ENVS))
def test_coefficient_product(gpu, monkeypatch, ring, env):
    rn, lib = gpu, gpu.load()
    r = Ring(rn, ring, monkeypatch, env)
    a_h, b_h = r.batch(), r.batch()
    a, b, o = r.sh(a_h), r.sh(b_h), r.sh(r.B)
    c = r.counts(lambda: rn.check(lib.rnt_mul(o.handle, a.handle, b.handle)), *PRODUCTS)
    assert c[r.product_kernel()] == 1 and sum(c.values()) == 1, c
    guards(o, a, b)
    got = o.channels()
    assert not o.is_ntt_domain()
    for p in r.picks():
        assert np.array_equal(got[p], orc.mul(r.Bo, a_h[p], b_h[p])), p
    assert np.array_equal(got, (r.up(a_h) * r.up(b_h)).channels())
    assert np.array_equal(a.channels(), a_h) and np.array_equal(b.channels(), b_h)
    rn.check(lib.rnt_mul(a.handle, a.handle, b.handle))  # out aliases a
    guards(a, b)
    assert np.array_equal(a.channels(), got)


# ---------------------------------------------------------------------------
# 4. rescale, automorphism, copies, partial download
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ring", ["n8", "n12", "n12_61", "n14", "n14_61", "n16"])
def test_rescale_automorphism_and_copies(gpu, monkeypatch, ring):
    rn, lib = gpu, gpu.load()
    r = Ring(rn, ring, monkeypatch)
    n, B, Bo = r.n, r.B, r.Bo
    a_h, b_h = r.batch(), r.batch()
    low = r.basis.drop_last(1)
    a, b = r.sh(a_h), r.sh(b_h)
    # rnt_rescale, from either domain
    want = [orc.rescale(Bo, a_h[p]) for p in range(B)]
    o = r.sh(B, basis=low)
    c = r.counts(lambda: rn.check(lib.rnt_rescale(o.handle, a.handle)), "rescale")
    assert c["rescale"] > 0, c
    guards(o, a)
    assert np.array_equal(o.channels(), np.stack(want))
    an = r.sh(a_h)
    an.to_ntt_domain()
    o = r.sh(B, basis=low)
    rn.check(lib.rnt_rescale(o.handle, an.handle))
    guards(o, an)
    assert np.array_equal(o.channels(), np.stack(want)) and not o.is_ntt_domain()
    assert np.array_equal(o.channels(), r.up(a_h).rescale().channels())
    # rnt_ct_rescale: both outputs on one shared context
    o0, o1 = r.sh(B, basis=low), r.sh(B, basis=low)
    c = r.counts(lambda: rn.check(lib.rnt_ct_rescale(o0.handle, o1.handle, a.handle, b.handle)), "rescale")
    assert c["rescale"] > 0, c
    guards(o0, o1, a, b)
    got0, got1 = o0.channels(), o1.channels()
    for p in r.picks():
        assert np.array_equal(got0[p], want[p]) and np.array_equal(got1[p], orc.rescale(Bo, b_h[p])), p
    # rnt_automorphism: odd, even and the identity exponent 2N
    for g in (3, 2 * n - 1, 6, 2 * n):
        o = r.sh(B)
        c = r.counts(lambda: rn.check(lib.rnt_automorphism(o.handle, a.handle, g)), "automorphism", "copy")
        assert c["automorphism"] + c["copy"] > 0 or g == 2 * n, (g, c)
        guards(o, a)
        got = o.channels()
        for p in r.picks():
            assert np.array_equal(got[p], orc.automorphism(Bo, a_h[p], g)[0]), (g, p)
        assert np.array_equal(got, r.up(a_h).automorphism(g).channels()), g
    x = r.sh(a_h)
    rn.check(lib.rnt_automorphism(x.handle, x.handle, 3))  # in place, through the workspace
    x.check_guards()
    assert np.array_equal(x.channels()[0], orc.automorphism(Bo, a_h[0], 3)[0])
    # rnt_copy: a pair that is not 16-byte aligned takes the memcpy branch (no kernel)
    al = r.up(b_h)
    for dst, src, src_h, kernel in ((r.sh(B), a, a_h, 0), (r.sh(B), al, b_h, 0), (rn.RnsPoly(r.basis, B), a, a_h, 0),
                                    (rn.RnsPoly(r.basis, B), al, b_h, 1)):
        c = r.counts(lambda: rn.check(lib.rnt_copy(dst.handle, src.handle)), "copy")
        assert c["copy"] == kernel, c
        guards(*(v for v in (dst, src) if hasattr(v, "check_guards")))
        assert np.array_equal(dst.channels(), src_h)
    # rnt_copy_polys of a sub-range (a memcpy per limb), shifted on either side and on both
    for dst, src in ((r.sh(b_h), a), (r.sh(b_h), r.up(a_h)), (r.up(b_h), a)):
        dst.copy_polys(src, 1, 0, B - 1)
        guards(*(v for v in (dst, src) if hasattr(v, "check_guards")))
        assert np.array_equal(dst.channels(), np.concatenate([b_h[:1], a_h[:B - 1]]))
    # rnt_download_polys of a sub-range of a shifted view
    c = r.counts(lambda: a.channels_of(1, B - 1), "export")
    assert c["export"] == 1, c
    assert np.array_equal(a.channels_of(1, B - 1), a_h[1:B]) and np.array_equal(a.channels_of(0, 1), a_h[:1])
    assert np.array_equal(a.channels(), a_h) and np.array_equal(b.channels(), b_h)


# ---------------------------------------------------------------------------
# 5. the tensor product
# ---------------------------------------------------------------------------
TENSOR_RINGS = [(r, {}) for r in ("n8", "n12", "n12_30", "n12_61", "n14", "n14_61", "n16")] + [N16_KNOBS[1]]


@pytest.mark.parametrize("ring,env", TENSOR_RINGS, ids=_ids(TENSOR_RINGS))
def test_ct_tensor(gpu, monkeypatch, ring, env):
    rn, lib = gpu, gpu.load()
    r = Ring(rn, ring, monkeypatch, env)
    Bo, B = r.Bo, r.B
    h = [r.batch() for _ in range(4)]  # c0, c1, c0', c1'
    ins = [r.sh(x) for x in h]
    d = [r.sh(B) for _ in range(3)]
    names = ("tensor_whole", "tensor_rows", "mf_tensor")
    c = r.counts(lambda: rn.check(lib.rnt_ct_tensor(*[x.handle for x in d + ins])), *names)
    assert c[r.tensor_kernel()] > 0 and sum(c.values()) == c[r.tensor_kernel()], c
    guards(*d, *ins)
    assert d[0].is_ntt_domain() and d[1].is_ntt_domain() and not d[2].is_ntt_domain()
    got = [x.channels() for x in d]

    def seed(x):
        """The key-switch seed of x: NTT(x) 2^-w mod q, w the word width (a
        Montgomery product of plain transforms, rnt_kernels.hip)."""
        xn = orc.to_ntt(Bo, x).astype(object)
        rinv = [pow(1 << (8 * r.wb), -1, q) for q in r.mod]
        return np.stack([xn[l] * rinv[l] % r.mod[l] for l in range(r.L)]).astype(np.uint64)

    for p in r.picks():
        c0, c1, c0p, c1p = (x[p] for x in h)
        assert np.array_equal(got[2][p], orc.mul(Bo, c1, c1p)), p
        # (a seed is a residue class: the header promises no canonical word)
        assert np.array_equal(got[0][p] % r.q, seed(orc.mul(Bo, c0, c0p))), p
        assert np.array_equal(got[1][p] % r.q, seed(orc.add(Bo, orc.mul(Bo, c0, c1p), orc.mul(Bo, c1, c0p)))), p
    al = rn.ct_tensor(*(r.up(x) for x in h))
    for i in range(3):
        assert np.array_equal(got[i], al[i].channels()), i
    for x, x_h in zip(ins, h):
        assert np.array_equal(x.channels(), x_h)


# ---------------------------------------------------------------------------
# 6. the gadget key-switch family
# ---------------------------------------------------------------------------
def _shifted_key(r, ka_h, kb_h):
    """A gadget key whose planes are shifted: uploaded into the views and made
    NTT-resident there (rnt_key_prepare transforms in place)."""
    ka, kb = r.sh(ka_h), r.sh(kb_h)
    r.rn.check(r.rn.load().rnt_key_prepare(ka.handle, kb.handle))
    guards(ka, kb)
    assert ka.is_ntt_domain() and kb.is_ntt_domain()
    return ka, kb


@pytest.mark.parametrize("ring", ALL_RINGS)
def test_keyswitch(gpu, monkeypatch, ring):
    rn, lib = gpu, gpu.load()
    r = Ring(rn, ring, monkeypatch)
    B = r.B
    d_h, ka_h, kb_h = r.batch(), r.rand(r.L), r.rand(r.L)
    ka, kb = _shifted_key(r, ka_h, kb_h)
    d, a0, a1 = r.sh(d_h), r.sh(B), r.sh(B)
    c = r.counts(lambda: rn.check(lib.rnt_keyswitch(a0.handle, a1.handle, d.handle, ka.handle, kb.handle)),
                 "ks_whole", "ks_rows")
    assert c[r.ks_kernel()] > 0 and sum(c.values()) == c[r.ks_kernel()], c
    guards(a0, a1, d, ka, kb)
    g0, g1 = a0.channels(), a1.channels()
    for p in r.picks():
        w = orc.keyswitch(r.Bo, d_h[p], ka_h, kb_h, threads=T)
        assert np.array_equal(g0[p], w[0]) and np.array_equal(g1[p], w[1]), p
    w0, w1 = rn.keyswitch(r.up(d_h), rn.RnsGadgetKey.from_channels(ka_h, kb_h, r.basis))
    assert np.array_equal(g0, w0.channels()) and np.array_equal(g1, w1.channels())
    assert np.array_equal(d.channels(), d_h)


@pytest.mark.parametrize("ring", ALL_RINGS[:-1])
def test_rotate_and_mul_relin(gpu, monkeypatch, ring):
    """rnt_ct_rotate, rnt_ct_mul_relin and rnt_ct_mul_relin_rescale with a
    shifted key, shifted inputs and shifted outputs."""
    rn, lib = gpu, gpu.load()
    r = Ring(rn, ring, monkeypatch)
    B, Bo = r.B, r.Bo
    h = [r.batch() for _ in range(4)]  # c0, c1, c0', c1'
    ka_h, kb_h = r.rand(r.L), r.rand(r.L)
    ka, kb = _shifted_key(r, ka_h, kb_h)
    ins = [r.sh(x) for x in h]
    key_al = rn.RnsGadgetKey.from_channels(ka_h, kb_h, r.basis)
    ct1, ct2 = rn.Ciphertext(r.up(h[0]), r.up(h[1])), rn.Ciphertext(r.up(h[2]), r.up(h[3]))
    names = ("ks_whole", "ks_rows", "tensor_whole", "tensor_rows", "mf_tensor")
    for k in (1, -3) if r.log_n <= 14 else (1,):
        o0, o1 = r.sh(B), r.sh(B)
        c = r.counts(lambda: rn.check(lib.rnt_ct_rotate(o0.handle, o1.handle, ins[0].handle, ins[1].handle, k,
                                                        ka.handle, kb.handle)), *names)
        assert c[r.ks_kernel()] > 0, c
        guards(o0, o1, *ins, ka, kb)
        g0, g1 = o0.channels(), o1.channels()
        for p in r.picks():
            w = orc.rotate_ciphertext(Bo, h[0][p], h[1][p], k, ka_h, kb_h, threads=T)
            assert np.array_equal(g0[p], w[0]) and np.array_equal(g1[p], w[1]), (k, p)
        key_al.rotation = k
        al = rn.rotate_ciphertext(ct1, key_al)
        assert np.array_equal(g0, al.c0.channels()) and np.array_equal(g1, al.c1.channels()), k
    o0, o1 = r.sh(B), r.sh(B)
    c = r.counts(lambda: rn.check(lib.rnt_ct_mul_relin(o0.handle, o1.handle, *[x.handle for x in ins], ka.handle,
                                                       kb.handle)), *names)
    assert c[r.ks_kernel()] > 0 and c[r.tensor_kernel()] > 0, c
    guards(o0, o1, *ins, ka, kb)
    g0, g1 = o0.channels(), o1.channels()
    low = r.basis.drop_last(1)
    f0, f1 = r.sh(B, basis=low), r.sh(B, basis=low)
    c = r.counts(lambda: rn.check(lib.rnt_ct_mul_relin_rescale(f0.handle, f1.handle, *[x.handle for x in ins],
                                                               ka.handle, kb.handle)), *names)
    assert c[r.ks_kernel()] > 0 and c[r.tensor_kernel()] > 0, c
    guards(f0, f1, *ins, ka, kb)
    r0, r1 = f0.channels(), f1.channels()
    for p in r.picks():
        w = orc.mul_ciphertexts_gadget(Bo, h[0][p], h[1][p], h[2][p], h[3][p], ka_h, kb_h, threads=T)
        assert np.array_equal(g0[p], w[0]) and np.array_equal(g1[p], w[1]), p
        assert np.array_equal(r0[p], orc.rescale(Bo, w[0])) and np.array_equal(r1[p], orc.rescale(Bo, w[1])), p
    al = rn.mul_ciphertexts_gadget(ct1, ct2, key_al)
    assert np.array_equal(g0, al.c0.channels()) and np.array_equal(g1, al.c1.channels())
    al = rn.mul_ciphertexts_gadget_rescale(ct1, ct2, key_al)
    assert np.array_equal(r0, al.c0.channels()) and np.array_equal(r1, al.c1.channels())
    for x, x_h in zip(ins, h):
        assert np.array_equal(x.channels(), x_h)


# ---------------------------------------------------------------------------
# 7. linear transforms: k_bcast_mul KIND 1 reads the caller's plaintext planes
# ---------------------------------------------------------------------------
LT = [(12, 3, 31), (14, 3, 31), (12, 2, 61)]  # log_n, B, bits: RINGS' n12, n14 and n12_61 at three limbs


def _lt_shift(rn, c, sets):
    """Shifted copies of a linear-transform case's ciphertext, plaintexts and
    key sets, and two shifted outputs."""
    wb = _word_bytes(rn, c.basis)

    def sh(src, ntt=False):
        v = shifted(rn, c.basis, src, ntt)
        assert v.device_ptr()[0] % 16 == wb
        return v

    d = sh(c.d)
    assert d.is_ntt_domain()
    keys = [sh(s) for s in sets]
    return sh(c.B), sh(c.B), sh(c.c0), sh(c.c1), d, keys


@pytest.mark.parametrize("log_n,B,bits", LT)
def test_linear_transform(gpu, monkeypatch, log_n, B, bits):
    rn, lib = gpu, gpu.load()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    c = LinearCase(rn, log_n, 3, B, bits, edge=True, seed=5)
    o0, o1, c0, c1, d, keys = _lt_shift(rn, c, (c.keyset.a, c.keyset.b))
    steps = (ctypes.c_int32 * len(c.steps))(*c.steps)
    c.basis.profile_enable(True)
    rn.check(lib.rnt_ct_linear(o0.handle, o1.handle, c0.handle, c1.handle, steps, len(c.steps), d.handle,
                               keys[0].handle, keys[1].handle))
    counts = {k: c.basis.profile_read(k)[0] for k in ("elementwise", "ks_whole", "ks_rows")}
    c.basis.profile_enable(False)
    print(counts)
    assert counts["elementwise"] > 0 and counts["ks_whole" if log_n == 12 and bits == 31 else "ks_rows"] > 0, counts
    guards(o0, o1, c0, c1, d, *keys)
    g0, g1 = o0.channels(), o1.channels()
    for p in sorted({0, B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from linear_ref"
    al = rn.linear_transform(c.ct, c.d, c.keyset)
    assert np.array_equal(g0, al.c0.channels()) and np.array_equal(g1, al.c1.channels())
    # in place on the shifted ciphertext
    rn.check(lib.rnt_ct_linear(c0.handle, c1.handle, c0.handle, c1.handle, steps, len(c.steps), d.handle,
                               keys[0].handle, keys[1].handle))
    guards(c0, c1, d, *keys)
    assert np.array_equal(c0.channels(), g0) and np.array_equal(c1.channels(), g1)


@pytest.mark.parametrize("log_n,B,bits", LT)
def test_linear_transform_bsgs(gpu, monkeypatch, log_n, B, bits):
    rn, lib = gpu, gpu.load()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    c = BsgsCase(rn, log_n, 3, B, bits, edge=True, seed=5)
    o0, o1, c0, c1, d, keys = _lt_shift(rn, c, (c.bset.a, c.bset.b, c.gset.a, c.gset.b))
    baby, giant = (ctypes.c_int32 * len(c.baby))(*c.baby), (ctypes.c_int32 * len(c.giant))(*c.giant)
    c.basis.profile_enable(True)
    rn.check(lib.rnt_ct_linear_bsgs(o0.handle, o1.handle, c0.handle, c1.handle, baby, len(c.baby), giant,
                                    len(c.giant), d.handle, *[x.handle for x in keys]))
    counts = {k: c.basis.profile_read(k)[0] for k in ("elementwise", "bsgs_mac", "ks_whole", "ks_rows")}
    c.basis.profile_enable(False)
    print(counts)
    assert counts["elementwise"] > 0 and counts["ks_whole" if log_n == 12 and bits == 31 else "ks_rows"] > 0, counts
    guards(o0, o1, c0, c1, d, *keys)
    g0, g1 = o0.channels(), o1.channels()
    for p in sorted({0, B - 1}):
        r0, r1 = c.reference(p)
        assert np.array_equal(g0[p], r0) and np.array_equal(g1[p], r1), f"ciphertext {p} differs from bsgs_ref"
    al = c.run()
    assert np.array_equal(g0, al.c0.channels()) and np.array_equal(g1, al.c1.channels())


# ---------------------------------------------------------------------------
# 8. k_lincomb's one-word forms
# ---------------------------------------------------------------------------
def _lincomb(rn, c, out0, out1, x0, x1, with_bias, rescale):
    f = rn.load().rnt_ct_lincomb_rescale if rescale else rn.load().rnt_ct_lincomb
    w = np.ascontiguousarray(c.w, dtype=np.uint64)
    b = np.ascontiguousarray(c.bias, dtype=np.uint64)
    assert w.shape == (c.n_out, c.n_in, c.Lv) and b.shape == (c.n_out, c.Lv)
    c.basis.profile_enable(True)
    try:
        rn.check(f(out0.handle, out1.handle, x0.handle, x1.handle, c.n_in, c.n_out, w.ctypes.data_as(U64P),
                   b.ctypes.data_as(U64P) if with_bias else None))
        assert c.basis.profile_read("lincomb")[0] == 1 and c.basis.profile_read("rescale")[0] == 0
    finally:
        c.basis.profile_enable(False)


@pytest.mark.parametrize("n_in,n_out", [(3, 2), (5, 1), (9, 2), (16, 16)])
@pytest.mark.parametrize("bits", [30, 60])
def test_lincomb(gpu, bits, n_in, n_out):
    """One shape per register tier and the 64 KiB LDS case, with and without
    the bias (its lane test `(i & nmask) == 0` at one word a lane) and the
    rescale: inputs and outputs shifted."""
    rn = gpu
    c = LincombCase(rn, bits, 3, n_in, n_out, 3, seed=bits + 31 * n_in + n_out + 5)
    wb = 4 if bits == 30 else 8
    low = c.basis.drop_last(1)
    x0, x1 = shifted(rn, c.basis, c.x0), shifted(rn, c.basis, c.x1)
    assert x0.device_ptr()[0] % 16 == wb and x1.device_ptr()[0] % 16 == wb
    for with_bias in (False, True):
        for rescale in (False, True):
            ob = low if rescale else c.basis
            o0, o1 = shifted(rn, ob, n_out * 3), shifted(rn, ob, n_out * 3)
            assert o0.device_ptr()[0] % 16 == wb and o1.device_ptr()[0] % 16 == wb
            _lincomb(rn, c, o0, o1, x0, x1, with_bias, rescale)
            guards(o0, o1, x0, x1)
            want0, want1 = c.reference(with_bias, rescale)
            assert np.array_equal(o0.channels(), want0), (with_bias, rescale, "out0 differs from the definition")
            assert np.array_equal(o1.channels(), want1), (with_bias, rescale, "out1 differs from the definition")
            al = rn.ct_lincomb(c.ct, n_in, c.ints, c.bias_ints if with_bias else None, rescale=rescale)
            assert np.array_equal(o0.channels(), al.c0.channels_batch())
            assert np.array_equal(o1.channels(), al.c1.channels_batch())
    assert np.array_equal(x0.channels(), c.x0) and np.array_equal(x1.channels(), c.x1)


@pytest.mark.parametrize("which", ["x1", "out1"])
@pytest.mark.parametrize("bits", [30, 60])
def test_lincomb_one_shifted_operand(gpu, bits, which):
    """One unaligned pointer among four is enough for the one-word form."""
    rn = gpu
    c = LincombCase(rn, bits, 3, 3, 2, 3, seed=bits + 77)
    wb = 4 if bits == 30 else 8
    for rescale in (False, True):
        ob = c.basis.drop_last(1) if rescale else c.basis
        x0, x1 = c.ct.c0, c.ct.c1
        o0, o1 = rn.RnsPoly(ob, 6), rn.RnsPoly(ob, 6)
        if which == "x1":
            x1 = sh = shifted(rn, c.basis, c.x1)
        else:
            o1 = sh = shifted(rn, ob, 6)
        assert sh.device_ptr()[0] % 16 == wb
        assert all(v.device_ptr()[0] % 16 == 0 for v in (x0, x1, o0, o1) if v is not sh)
        _lincomb(rn, c, o0, o1, x0, x1, True, rescale)
        sh.check_guards()
        want0, want1 = c.reference(True, rescale)
        assert np.array_equal(o0.channels(), want0) and np.array_equal(o1.channels(), want1), rescale


# ---------------------------------------------------------------------------
# 9. sampler and encoder into a shifted destination
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [31, 61])
def test_sample_uniform_into_a_shifted_view(gpu, monkeypatch, bits):
    rn, lib = gpu, gpu.load()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    n, B = 1 << 10, 3
    mod = rn.generate_primes(bits, 3, n)
    basis = rn.RnsBasis(mod, n)
    v = shifted(rn, basis, B)
    assert v.device_ptr()[0] % 16 == (4 if bits == 31 else 8)
    seed, stream = 0x1234_5678_9ABC_DEF0, 7
    basis.profile_enable(True)
    rn.check(lib.rnt_sample_uniform(v.handle, seed, stream))
    count = basis.profile_read("sample")[0]
    basis.profile_enable(False)
    assert count > 0
    v.check_guards()
    assert np.array_equal(v.channels(), smp.uniform(mod, n, B, seed, stream))


@pytest.mark.parametrize("bits", [31, 61])
def test_encode_into_a_shifted_view(gpu, monkeypatch, bits):
    rn, lib = gpu, gpu.load()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    n, B, scale = 1 << 10, 3, 30
    mod = rn.generate_primes(bits, 3, n)
    basis = rn.RnsBasis(mod, n)
    rng = np.random.default_rng(10 + bits)
    nv = n // 2 - 3
    vals = np.ascontiguousarray(rng.uniform(-4, 4, (B, nv)) + 1j * rng.uniform(-4, 4, (B, nv)))
    v = shifted(rn, basis, B)
    assert v.device_ptr()[0] % 16 == (4 if bits == 31 else 8)
    basis.profile_enable(True)
    rn.check(lib.rnt_encode(v.handle, vals.ctypes.data_as(ctypes.c_void_p), nv, scale))
    count = basis.profile_read("sfft")[0]
    basis.profile_enable(False)
    assert count > 0
    v.check_guards()
    assert not v.is_ntt_domain()
    ints = np.asarray(v.to_coeffs())
    ch = v.channels()
    for p in range(B):
        _assert_coeffs_match(ints[p], enc.encode_fft_real(vals[p], n, scale))
        want = np.stack([np.asarray(ints[p], dtype=object) % q for q in mod]).astype(np.uint64)
        assert np.array_equal(ch[p], want), p
    al = rn.CkksEncoder(n, scale).encode_complex(vals, basis)
    assert np.array_equal(ch, al.poly.channels())
