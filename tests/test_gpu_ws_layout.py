"""The call-scoped workspace every fused call requests, to the byte.

Each call family is warmed once un-recorded (first-use constants go up then),
the block cache is emptied (`pool_trim`), the call alone is recorded into a
graph, and `Graph.workspace()` -- (blocks, bytes) of the workspace the graph
keeps, a fresh block having exactly the requested size -- is compared with a
literal.  The literals are what the commit BEFORE the calls were moved onto
csrc/rnt_ws.hpp's layout type reported for this same script (cfebfc4, "Add
rotate-and-sum on hybrid keys"; both columns in profiles/ws_layout_bytes.txt),
never what the rewritten code reports.

Rings, the smallest that reach each path: w12 = 2^12 x 3 limbs u32 (whole-plane:
no gadget scratch), f15 = 2^15 x 3 u32 (four-step: S | U0 | U1), m16 = 2^16 x 2
u32 (matrix-core tensor, one scratch block), u64 = 2^12 x 2 at 61 bits.  The
hybrid calls have one special prime and alpha = 2 on every ring, alpha = 1 on w12.

Every family runs with one ciphertext.  The families that chunk run again on
f15 with three ciphertexts and RNT_KS_WS_MB set so that a chunk holds two -- the
last chunk is smaller than the others -- and there the outputs are also compared
bit for bit with the same call at the default cap: a part placed wrongly for the
smaller chunk breaks that.  That the capped call runs two chunks is asserted from
the launch counts of its per-chunk kernels: twice those of the uncapped call.  The caps (CAPS below): a plane of f15 is 2^15 x 4 B
= 1/8 MiB, so M MiB hold 8 M planes and a call of P planes per ciphertext gets
chunks of floor(8 M / P).

Not in the table: rnt_ct_lincomb(_rescale) refuses to be recorded (its weights
go up by a host copy); tests/test_gpu_lincomb.py covers its results.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import test_gpu_bsgs
import test_gpu_dot_hybrid
import test_gpu_hoist
import test_gpu_hybrid
import test_gpu_hybrid_hoist
import test_gpu_linear
import test_gpu_plain_mac
import test_gpu_rotsum

pytestmark = pytest.mark.gpu

RINGS = {"w12": (12, 3, 31), "f15": (15, 3, 31), "m16": (16, 2, 31), "u64": (12, 2, 61)}
STEPS = (0, 1, -3)          # a step 0 and two that rotate
BABY, GIANT = (0, 1), (0, 2)  # n1 = 2, two pairs of inner sums
N_TERMS = 2


# Fixtures, one of each kind per (ring, batch, alpha, cap): a context reads RNT_KS_WS_MB when it is created.
@functools.lru_cache(maxsize=None)
def _fix(rn, kind, ring, B, alpha, cap):
    log_n, L, bits = RINGS[ring]
    hyb = (rn, log_n, L, 1, alpha, B, bits)
    if kind == "linear":
        return test_gpu_linear.Case(rn, log_n, L, B, bits, steps=list(STEPS), seed=3)
    if kind == "bsgs":
        return test_gpu_bsgs.Case(rn, log_n, L, B, bits, baby=list(BABY), giant=list(GIANT), seed=3)
    if kind == "hoist":
        return test_gpu_hoist.Case(rn, log_n, L, B, bits, steps=list(STEPS), seed=3)
    if kind == "bsgs_hoist":
        return test_gpu_hoist.BsgsCase(rn, log_n, L, B, bits, baby=list(BABY), giant=list(GIANT), seed=3)
    if kind == "mac":
        return test_gpu_plain_mac.MacCase(rn, log_n, L, B, bits, N_TERMS, seed=3)
    if kind == "hybrid":
        return test_gpu_hybrid.Case(*hyb, seed=3)
    if kind == "dot":
        return test_gpu_dot_hybrid.DotCase(*hyb, N_TERMS, seed=3)
    if kind == "hybrid_hoist":
        return test_gpu_hybrid_hoist.Case(*hyb, steps=list(STEPS), seed=3)
    if kind == "hybrid_bsgs":
        return test_gpu_hybrid_hoist.BsgsCase(*hyb, baby=list(BABY), giant=list(GIANT), seed=3)
    if kind == "rotsum":
        return test_gpu_rotsum.Case(*hyb, steps=list(STEPS), seed=3)
    raise KeyError(kind)


def _polys(r):
    return (r.c0, r.c1) if hasattr(r, "c0") else tuple(r)


def _ext(rn, c):
    """rnt_keyswitch_ext: L - 1 target limbs (a limb shard) over the L source limbs."""
    if not hasattr(c, "ext"):
        Lt = c.L - 1
        Bt = rn.RnsBasis(c.mod[:Lt], c.n)
        ka, kb = c.keys[1]
        key_t = rn.RnsGadgetKey.from_channels(np.ascontiguousarray(ka[:, :Lt]), np.ascontiguousarray(kb[:, :Lt]), Bt)
        c.ext = (Bt, key_t)
    Bt, key_t = c.ext
    ptr, _ = c.ct.c1.device_ptr()
    return Bt, lambda: rn.keyswitch_ext(ptr, c.L, key_t, Bt, c.B)


# family -> (fixture kind, call on the fixture -> (basis, run)); `run` returns the outputs
def _on(f):
    return lambda rn, c: (c.basis, lambda: f(rn, c))


GADGET = {
    "keyswitch": ("linear", _on(lambda rn, c: rn.keyswitch(c.ct.c1, c.gk[1]))),
    "keyswitch_ext": ("linear", _ext),
    "ct_tensor": ("linear", _on(lambda rn, c: rn.ct_tensor(c.ct.c0, c.ct.c1, c.ct.c1, c.ct.c0))),
    "ct_mul_relin": ("linear", _on(lambda rn, c: rn.mul_ciphertexts_gadget(c.ct, rn.Ciphertext(c.ct.c1, c.ct.c0),
                                                                        c.gk[1]))),
    "ct_mul_relin_rescale": ("linear", _on(lambda rn, c: rn.mul_ciphertexts_gadget_rescale(
        c.ct, rn.Ciphertext(c.ct.c1, c.ct.c0), c.gk[1]))),
    "ct_rotate": ("linear", _on(lambda rn, c: rn.rotate_ciphertext(c.ct, c.gk[2]))),
    "ct_linear": ("linear", _on(lambda rn, c: rn.linear_transform(c.ct, c.d, c.keyset))),
    "ct_rotate_hoisted": ("hoist", _on(lambda rn, c: c.run())),
    "ct_linear_bsgs": ("bsgs", _on(lambda rn, c: c.run())),
    "ct_linear_bsgs_hoisted": ("bsgs_hoist", _on(lambda rn, c: c.run())),
    "ct_plain_mac": ("mac", _on(lambda rn, c: rn.ct_plain_mac(c.ct, c.nt, c.pt, None, rescale=False))),
    "ct_plain_mac_rescale": ("mac", _on(lambda rn, c: rn.ct_plain_mac(c.ct, c.nt, c.pt, None, rescale=True))),
}
HYBRID = {
    "keyswitch_hybrid": ("hybrid", _on(lambda rn, c: rn.keyswitch_hybrid(c.ct.c1, c.key))),
    "ct_rotate_hybrid": ("hybrid", _on(lambda rn, c: rn.rotate_ciphertext_hybrid(c.ct, c.key))),
    "ct_mul_relin_hybrid": ("hybrid", _on(lambda rn, c: rn.mul_ciphertexts_hybrid(c.ct, c.ctp, c.key))),
    "ct_mul_relin_rescale_hybrid": ("hybrid", _on(lambda rn, c: rn.mul_ciphertexts_hybrid_rescale(c.ct, c.ctp, c.key))),
    "ct_dot_relin_hybrid": ("dot", _on(lambda rn, c: rn.dot_ciphertexts_hybrid(c.ctx, c.cty, c.nt, c.key,
                                                                              rescale=False))),
    "ct_dot_relin_rescale_hybrid": ("dot", _on(lambda rn, c: rn.dot_ciphertexts_hybrid(c.ctx, c.cty, c.nt, c.key,
                                                                                      rescale=True))),
    "ct_rotate_hybrid_hoisted": ("hybrid_hoist", _on(lambda rn, c: c.run())),
    "ct_rotsum_hybrid": ("rotsum", _on(lambda rn, c: c.run())),
    "ct_linear_bsgs_hybrid": ("hybrid_bsgs", _on(lambda rn, c: c.run())),
    "ct_linear_bsgs_hybrid_rescale": ("hybrid_bsgs", _on(lambda rn, c: rn.linear_transform_bsgs_hybrid_rescale(
        c.ct, c.d, c.bset, c.gset))),
}
FAMILIES = {**GADGET, **HYBRID}

# RNT_KS_WS_MB for chunks of two on f15 (L = 3; hybrid: LE = 4, alpha = 2, beta = 2, so D | A0 | A1 is 16
# planes): M with floor(8 M / P) = 2, P the planes per ciphertext the call's chunk rule counts.
CAPS = {
    "keyswitch": 3,                # S = L L = 9: 24 / 9
    "keyswitch_ext": 2,            # S = Lt Ls = 2 x 3 = 6: 16 / 6
    "ct_mul_relin": 3,             # 9
    "ct_mul_relin_rescale": 3,     # 9
    "ct_rotate": 3,                # 9
    "ct_linear": 3,                # 9
    "ct_rotate_hoisted": 8,        # L L + (2 tg + 2) L, tg = 2: 9 + 18 = 27: 64 / 27
    "ct_linear_bsgs": 16,          # (2 n1 + 2 nv + 4) L + L L + 2 L = 36 + 15 = 51: 128 / 51
    "ct_linear_bsgs_hoisted": 24,  # (12 + 2 kHoistT) L + 15 = 60 + 15 = 75: 192 / 75
    "ct_plain_mac": 4,             # 2 gmax L = 12: 32 / 12
    "ct_plain_mac_rescale": 6,     # (2 gmax + 2) L = 18: 48 / 18
    "keyswitch_hybrid": 4,         # 16: 32 / 16
    "ct_rotate_hybrid": 4,         # 16
    "ct_mul_relin_hybrid": 12,     # 16 + (4 T + 3 D) L = 37: 96 / 37
    "ct_mul_relin_rescale_hybrid": 8,   # 16 + (4 + 1) L = 31 (seeded: d2 alone): 64 / 31
    "ct_dot_relin_hybrid": 16,     # 16 + (4 gmax + 3) L = 49: 128 / 49
    "ct_dot_relin_rescale_hybrid": 12,  # 16 + (4 gmax + 1) L = 43: 96 / 43
    "ct_rotate_hybrid_hoisted": 8,      # LE beta + 2 tg LE, tg = 2 (fused tail: no staging) = 24: 64 / 24
    "ct_rotsum_hybrid": 6,         # 16 + 2 Lv (S and S1) = 22: 48 / 22
    "ct_linear_bsgs_hybrid": 16,   # 16 + (2 n1 + 2 nv + 3) Lv = 16 + 33 = 49: 128 / 49
    "ct_linear_bsgs_hybrid_rescale": 16,
}

# (family, ring, B, alpha, cap in MiB or None)
CASES = [(f, ring, 1, 0, None) for ring in RINGS for f in GADGET]
CASES += [(f, ring, 1, 2, None) for ring in RINGS for f in HYBRID]
CASES += [(f, "w12", 1, 1, None) for f in HYBRID]
CASES += [(f, "f15", 3, 2 if f in HYBRID else 0, cap) for f, cap in CAPS.items()]


def case_id(case):
    f, ring, B, alpha, cap = case
    return f"{f}-{ring}-B{B}" + (f"-alpha{alpha}" if alpha else "") + (f"-cap{cap}" if cap else "")


def _call(rn, case):
    f, ring, B, alpha, cap = case
    kind, make = FAMILIES[f]
    return make(rn, _fix(rn, kind, ring, B, alpha, cap))


def measure(rn, case):
    """(blocks, bytes) of the workspace the call, recorded alone, leaves with its graph."""
    basis, run = _call(rn, case)
    keep = run()  # warm: the first-use constant uploads
    basis.sync()
    del keep
    rn.pool_trim(basis.device)  # an empty cache: a fresh block has exactly the requested size
    with basis.capture() as g:
        keep = run()
    got = g.workspace()
    del g, keep
    rn.pool_trim(basis.device)
    return got


# the kernels a call launches a fixed number of times per chunk (whichever of them the family runs)
PER_CHUNK = ("ks_decompose", "hoist_digits", "plain_mac", "modup")


def _outputs_and_chunk_launches(basis, run):
    basis.profile_enable(True)
    out = [p.channels() for p in _polys(run())]
    n = sum(basis.profile_read(k)[0] for k in PER_CHUNK)
    basis.profile_enable(False)
    return out, n


EXPECTED = {
    "keyswitch-w12-B1": (1, 16),
    "keyswitch_ext-w12-B1": (0, 0),
    "ct_tensor-w12-B1": (0, 0),
    "ct_mul_relin-w12-B1": (1, 147456),
    "ct_mul_relin_rescale-w12-B1": (3, 245760),
    "ct_rotate-w12-B1": (1, 98304),
    "ct_linear-w12-B1": (2, 442368),
    "ct_rotate_hoisted-w12-B1": (1, 393216),
    "ct_linear_bsgs-w12-B1": (2, 786432),
    "ct_linear_bsgs_hoisted-w12-B1": (2, 1327104),
    "ct_plain_mac-w12-B1": (1, 196608),
    "ct_plain_mac_rescale-w12-B1": (1, 294912),
    "keyswitch-f15-B1": (1, 1966080),
    "keyswitch_ext-f15-B1": (1, 1310720),
    "ct_tensor-f15-B1": (1, 1572864),
    "ct_mul_relin-f15-B1": (1, 5111808),
    "ct_mul_relin_rescale-f15-B1": (1, 5373952),
    "ct_rotate-f15-B1": (1, 2752512),
    "ct_linear-f15-B1": (1, 5505024),
    "ct_rotate_hoisted-f15-B1": (1, 3145728),
    "ct_linear_bsgs-f15-B1": (1, 7864320),
    "ct_linear_bsgs_hoisted-f15-B1": (1, 11010048),
    "ct_plain_mac-f15-B1": (1, 1572864),
    "ct_plain_mac_rescale-f15-B1": (1, 2359296),
    "keyswitch-m16-B1": (1, 2097152),
    "keyswitch_ext-m16-B1": (1, 1048576),
    "ct_tensor-m16-B1": (1, 524288),
    "ct_mul_relin-m16-B1": (1, 4718592),
    "ct_mul_relin_rescale-m16-B1": (1, 5242880),
    "ct_rotate-m16-B1": (1, 3145728),
    "ct_linear-m16-B1": (1, 6815744),
    "ct_rotate_hoisted-m16-B1": (1, 3670016),
    "ct_linear_bsgs-m16-B1": (1, 9961472),
    "ct_linear_bsgs_hoisted-m16-B1": (1, 14155776),
    "ct_plain_mac-m16-B1": (1, 2097152),
    "ct_plain_mac_rescale-m16-B1": (1, 3145728),
    "keyswitch-u64-B1": (1, 262144),
    "keyswitch_ext-u64-B1": (1, 131072),
    "ct_tensor-u64-B1": (0, 0),
    "ct_mul_relin-u64-B1": (1, 458752),
    "ct_mul_relin_rescale-u64-B1": (1, 524288),
    "ct_rotate-u64-B1": (1, 393216),
    "ct_linear-u64-B1": (1, 851968),
    "ct_rotate_hoisted-u64-B1": (1, 458752),
    "ct_linear_bsgs-u64-B1": (1, 1245184),
    "ct_linear_bsgs_hoisted-u64-B1": (1, 1769472),
    "ct_plain_mac-u64-B1": (1, 262144),
    "ct_plain_mac_rescale-u64-B1": (1, 393216),
    "keyswitch_hybrid-w12-B1-alpha2": (1, 262144),
    "ct_rotate_hybrid-w12-B1-alpha2": (1, 360448),
    "ct_mul_relin_hybrid-w12-B1-alpha2": (1, 409600),
    "ct_mul_relin_rescale_hybrid-w12-B1-alpha2": (1, 311296),
    "ct_dot_relin_hybrid-w12-B1-alpha2": (1, 802816),
    "ct_dot_relin_rescale_hybrid-w12-B1-alpha2": (1, 704512),
    "ct_rotate_hybrid_hoisted-w12-B1-alpha2": (1, 393216),
    "ct_rotsum_hybrid-w12-B1-alpha2": (1, 360448),
    "ct_linear_bsgs_hybrid-w12-B1-alpha2": (1, 999424),
    "ct_linear_bsgs_hybrid_rescale-w12-B1-alpha2": (1, 999424),
    "keyswitch_hybrid-f15-B1-alpha2": (1, 2097152),
    "ct_rotate_hybrid-f15-B1-alpha2": (1, 2883584),
    "ct_mul_relin_hybrid-f15-B1-alpha2": (1, 4849664),
    "ct_mul_relin_rescale_hybrid-f15-B1-alpha2": (1, 4063232),
    "ct_dot_relin_hybrid-f15-B1-alpha2": (1, 6422528),
    "ct_dot_relin_rescale_hybrid-f15-B1-alpha2": (1, 5636096),
    "ct_rotate_hybrid_hoisted-f15-B1-alpha2": (1, 3145728),
    "ct_rotsum_hybrid-f15-B1-alpha2": (1, 2883584),
    "ct_linear_bsgs_hybrid-f15-B1-alpha2": (1, 7995392),
    "ct_linear_bsgs_hybrid_rescale-f15-B1-alpha2": (1, 7995392),
    "keyswitch_hybrid-m16-B1-alpha2": (1, 2359296),
    "ct_rotate_hybrid-m16-B1-alpha2": (1, 3407872),
    "ct_mul_relin_hybrid-m16-B1-alpha2": (1, 4456448),
    "ct_mul_relin_rescale_hybrid-m16-B1-alpha2": (1, 3407872),
    "ct_dot_relin_hybrid-m16-B1-alpha2": (1, 8126464),
    "ct_dot_relin_rescale_hybrid-m16-B1-alpha2": (1, 7077888),
    "ct_rotate_hybrid_hoisted-m16-B1-alpha2": (1, 3932160),
    "ct_rotsum_hybrid-m16-B1-alpha2": (1, 3407872),
    "ct_linear_bsgs_hybrid-m16-B1-alpha2": (1, 10223616),
    "ct_linear_bsgs_hybrid_rescale-m16-B1-alpha2": (1, 10223616),
    "keyswitch_hybrid-u64-B1-alpha2": (1, 294912),
    "ct_rotate_hybrid-u64-B1-alpha2": (1, 425984),
    "ct_mul_relin_hybrid-u64-B1-alpha2": (1, 491520),
    "ct_mul_relin_rescale_hybrid-u64-B1-alpha2": (1, 360448),
    "ct_dot_relin_hybrid-u64-B1-alpha2": (1, 1015808),
    "ct_dot_relin_rescale_hybrid-u64-B1-alpha2": (1, 884736),
    "ct_rotate_hybrid_hoisted-u64-B1-alpha2": (1, 491520),
    "ct_rotsum_hybrid-u64-B1-alpha2": (1, 425984),
    "ct_linear_bsgs_hybrid-u64-B1-alpha2": (1, 1277952),
    "ct_linear_bsgs_hybrid_rescale-u64-B1-alpha2": (1, 1277952),
    "keyswitch_hybrid-w12-B1-alpha1": (1, 327680),
    "ct_rotate_hybrid-w12-B1-alpha1": (1, 425984),
    "ct_mul_relin_hybrid-w12-B1-alpha1": (1, 475136),
    "ct_mul_relin_rescale_hybrid-w12-B1-alpha1": (1, 376832),
    "ct_dot_relin_hybrid-w12-B1-alpha1": (1, 868352),
    "ct_dot_relin_rescale_hybrid-w12-B1-alpha1": (1, 770048),
    "ct_rotate_hybrid_hoisted-w12-B1-alpha1": (1, 458752),
    "ct_rotsum_hybrid-w12-B1-alpha1": (1, 425984),
    "ct_linear_bsgs_hybrid-w12-B1-alpha1": (1, 1064960),
    "ct_linear_bsgs_hybrid_rescale-w12-B1-alpha1": (1, 1064960),
    "keyswitch-f15-B3-cap3": (1, 3932160),
    "keyswitch_ext-f15-B3-cap2": (1, 2621440),
    "ct_mul_relin-f15-B3-cap3": (1, 10223616),
    "ct_mul_relin_rescale-f15-B3-cap3": (1, 10747904),
    "ct_rotate-f15-B3-cap3": (1, 6291456),
    "ct_linear-f15-B3-cap3": (1, 11403264),
    "ct_rotate_hoisted-f15-B3-cap8": (1, 7077888),
    "ct_linear_bsgs-f15-B3-cap16": (1, 15335424),
    "ct_linear_bsgs_hoisted-f15-B3-cap24": (1, 21626880),
    "ct_plain_mac-f15-B3-cap4": (1, 3145728),
    "ct_plain_mac_rescale-f15-B3-cap6": (1, 4718592),
    "keyswitch_hybrid-f15-B3-alpha2-cap4": (1, 4194304),
    "ct_rotate_hybrid-f15-B3-alpha2-cap4": (1, 6553600),
    "ct_mul_relin_hybrid-f15-B3-alpha2-cap12": (1, 9699328),
    "ct_mul_relin_rescale_hybrid-f15-B3-alpha2-cap8": (1, 8126464),
    "ct_dot_relin_hybrid-f15-B3-alpha2-cap16": (1, 12845056),
    "ct_dot_relin_rescale_hybrid-f15-B3-alpha2-cap12": (1, 11272192),
    "ct_rotate_hybrid_hoisted-f15-B3-alpha2-cap8": (1, 6291456),
    "ct_rotsum_hybrid-f15-B3-alpha2-cap6": (1, 5767168),
    "ct_linear_bsgs_hybrid-f15-B3-alpha2-cap16": (1, 14417920),
    "ct_linear_bsgs_hybrid_rescale-f15-B3-alpha2-cap16": (1, 14417920),
}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_requested_workspace(gpu, monkeypatch, case):
    cap = case[4]
    if cap:
        monkeypatch.setenv("RNT_KS_WS_MB", str(cap))  # read at rnt_ctx_create
    got = measure(gpu, case)
    print(case_id(case), got)
    assert got == EXPECTED[case_id(case)]
    if cap:  # chunks of 2 + 1 against one chunk of 3 at the default cap: twice the per-chunk launches, bit for bit
        small, n_small = _outputs_and_chunk_launches(*_call(gpu, case))
        monkeypatch.delenv("RNT_KS_WS_MB")
        whole, n_whole = _outputs_and_chunk_launches(*_call(gpu, case[:4] + (None,)))
        assert n_whole > 0 and n_small == 2 * n_whole, (n_small, n_whole)
        assert len(small) == len(whole) and all(np.array_equal(a, b) for a, b in zip(small, whole))


def test_every_case_has_a_literal_and_every_literal_a_case():
    assert sorted(EXPECTED) == sorted(case_id(c) for c in CASES)
