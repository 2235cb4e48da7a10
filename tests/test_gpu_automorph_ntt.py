"""The automorphism in the NTT domain on the GPU (rnt_automorphism_ntt,
k_automorph_ntt): automorphism_ntt(ntt(x), g) equals ntt(automorphism(x, g))
word for word -- the library's own transforms and coefficient-domain
automorphism on one side, one gather on the other -- and the gather is the
index function tests/rotsum_ref.py pins on the CPU."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from rotsum_ref import ntt_automorphism_source

pytestmark = pytest.mark.gpu

B = 3
# log_n, limbs, bits
RINGS = [(8, 3, 31), (12, 2, 31), (12, 2, 61), (16, 2, 31)]


def _exponents(n):
    return [5, 25, 2 * n - 1, pow(5, 7, 2 * n) * (2 * n - 1) % (2 * n)]


def _case(rn, log_n, L, bits, seed=0):
    n = 1 << log_n
    mod = rn.generate_primes(bits, L, n)
    basis = rn.RnsBasis(mod, n)
    x = orc.uniform_poly(mod, n, np.random.default_rng(8100 + log_n + seed), batch=B)
    return n, mod, basis, x


def _want(rn, basis, x, g):
    w = rn.RnsPoly.from_channels(x, basis).automorphism(g)
    w.to_ntt_domain()
    return w


@pytest.mark.parametrize("log_n,L,bits", RINGS)
def test_equals_the_transform_of_the_coefficient_domain_automorphism(gpu, log_n, L, bits):
    rn = gpu
    n, mod, basis, x = _case(rn, log_n, L, bits)
    xn = rn.RnsPoly.from_channels(x, basis)
    xn.to_ntt_domain()
    before = xn.channels()
    for g in _exponents(n):
        got = rn.automorphism_ntt(xn, g)
        assert got.is_ntt_domain() and got.n_polys == B
        want = _want(rn, basis, x, g)
        assert np.array_equal(got.channels(), want.channels()), g
        assert np.array_equal(rn.RnsPoly.automorphism_ntt(xn, g).channels(), want.channels())
    assert np.array_equal(xn.channels(), before)  # the input is only read
    # the oracle agrees on the first poly (its transform, its automorphism)
    Bo = orc.Basis(mod, n)
    g = _exponents(n)[3]
    assert np.array_equal(rn.automorphism_ntt(xn, g).channels_of(0)[0], orc.to_ntt(Bo, orc.automorphism(Bo, x[0], g)[0]))
    # g is taken mod 2N, and g = 1 is the identity
    assert np.array_equal(rn.automorphism_ntt(xn, 5 + 2 * n).channels(), rn.automorphism_ntt(xn, 5).channels())
    assert np.array_equal(rn.automorphism_ntt(xn, 1).channels(), before)


def test_is_the_pinned_index_function_in_device_order(gpu):
    """Position p of every plane reads position ntt_automorphism_source(g)[p]:
    the device words of an NTT-domain buffer whose word at position p IS p, read
    back through a coefficient-domain wrap of the same memory (no permutation)."""
    import torch

    rn = gpu
    log_n, n = 8, 256
    mod = rn.generate_primes(31, 2, n)
    basis = rn.RnsBasis(mod, n)
    dev = torch.device("cuda", basis.device)
    src_t = torch.arange(n, dtype=torch.int32, device=dev).repeat(2 * B)
    dst_t = torch.zeros(2 * B * n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    for g in _exponents(n):
        a = rn.RnsPoly.wrap(basis, src_t.data_ptr(), B, in_ntt_domain=True, owner=src_t)
        o = rn.RnsPoly.wrap(basis, dst_t.data_ptr(), B, in_ntt_domain=False, owner=dst_t)
        rn.automorphism_ntt(a, g, out=o)
        basis.sync()
        got = dst_t.cpu().numpy().reshape(2 * B, n)
        want = ntt_automorphism_source(g, log_n)
        assert (got == want[None, :]).all(), g


def test_drop_last_view(gpu):
    rn = gpu
    n, mod, root, _ = _case(rn, 12, 3, 31, seed=1)
    basis = root.drop_last(1)
    x = orc.uniform_poly(mod[:2], n, np.random.default_rng(8150), batch=B)
    xn = rn.RnsPoly.from_channels(x, basis)
    xn.to_ntt_domain()
    for g in _exponents(n):
        assert np.array_equal(rn.automorphism_ntt(xn, g).channels(), _want(rn, basis, x, g).channels()), g


@pytest.mark.parametrize("bits", [31, 61])
def test_word_aligned_wrapped_buffers_between_guards(gpu, bits):
    """Input and output wrapped one word past a 16-byte boundary inside tensors
    filled with a sentinel: the kernel moves single words, and writes none
    outside its output."""
    import torch

    rn = gpu
    n, mod, basis, x = _case(rn, 8, 2, bits, seed=2)
    wb = 4 if bits == 31 else 8
    L = len(mod)
    sentinel = np.uint32(0xA5A5A5A5)
    dev = torch.device("cuda", basis.device)
    body = B * L * n * wb // 4

    def shifted(src=None, ntt=False):
        t = torch.full((body + 8,), int(sentinel.astype(np.int32)), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        v = rn.RnsPoly.wrap(basis, t.data_ptr() + 16 + wb, B, in_ntt_domain=ntt, owner=t)
        assert v.device_ptr()[0] % 16 == wb
        if src is not None:
            v.copy_polys(src)
        return v, t

    def guards(t):
        basis.sync()
        torch.cuda.synchronize(dev)
        lead = 4 + wb // 4
        h = t.cpu().numpy().view(np.uint32)
        assert (h[:lead] == sentinel).all() and (h[lead + body:] == sentinel).all()

    xn = rn.RnsPoly.from_channels(x, basis)
    xn.to_ntt_domain()
    a, ta = shifted(xn, ntt=True)
    for g in _exponents(n):
        o, to = shifted()
        rn.automorphism_ntt(a, g, out=o)
        assert np.array_equal(o.channels(), _want(rn, basis, x, g).channels()), g
        guards(to)
        guards(ta)


def test_errors(gpu):
    rn, lib = gpu, gpu.load()
    n, mod, basis, x = _case(rn, 8, 3, 31, seed=3)
    xn = rn.RnsPoly.from_channels(x, basis)
    xn.to_ntt_domain()
    mark = orc.uniform_poly(mod, n, np.random.default_rng(8190), batch=B)
    out = rn.RnsPoly.from_channels(mark, basis)

    def fails(kind, o, i, g, fields=None):
        with pytest.raises(rn.RnsNttError) as e:
            rn.check(lib.rnt_automorphism_ntt(o.handle if o is not None else None,
                                              i.handle if i is not None else None, g))
        assert e.value.kind == kind, str(e.value)
        if fields is not None:
            assert e.value.fields == fields
        assert np.array_equal(out.channels(), mark) and not out.is_ntt_domain()

    fails("DomainMismatch", out, rn.RnsPoly.from_channels(x, basis), 5)  # a coefficient-domain input
    for g in (0, 2, 4, 2 * n):
        fails("BadArgument", out, xn, g)  # an even g
    fails("BadArgument", xn, xn, 5)  # out aliases in
    fails("BadArgument", None, xn, 5)
    fails("BadArgument", out, None, 5)
    fails("BadArgument", rn.RnsPoly(basis, B + 1), xn, 5)
    other = rn.RnsPoly(rn.RnsBasis(mod, n), B)
    fails("BasisMismatch", other, xn, 5)
    # a key level view in either position
    emod = rn.generate_primes(31, 5, n)
    ext = rn.RnsBasis(emod, n)
    beta = 2
    ka = orc.uniform_poly(emod, n, np.random.default_rng(8191), batch=beta)
    key = rn.RnsHybridKey.from_channels(ka, ka, ext, 2, rotation=1, n_special=2)
    view = key.at_level(2)
    plain = rn.RnsPoly(ext, beta)
    plain.to_ntt_domain()
    zero = {"degree": 0, "max_degree": 0}
    with pytest.raises(rn.RnsNttError) as e:
        rn.check(lib.rnt_automorphism_ntt(plain.handle, view.a.handle, 5))
    assert e.value.kind == "Unsupported" and e.value.fields == zero
    with pytest.raises(rn.RnsNttError) as e:
        rn.check(lib.rnt_automorphism_ntt(view.a.handle, plain.handle, 5))
    assert e.value.kind == "Unsupported" and e.value.fields == zero
    # the valid call still runs
    rn.automorphism_ntt(xn, 5, out=out)
    assert out.is_ntt_domain() and np.array_equal(out.channels(), _want(rn, basis, x, 5).channels())
