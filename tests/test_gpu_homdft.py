"""ModRaise -> CoeffToSlot -> SlotToCoeff and the conjugation helpers on the GPU
against the CPU model of tests/homdft_ref.py.

Ring: N = 2^8 and 2^10, 7 ciphertext primes of 30 bits, K = 2 special primes of
31 bits, alpha = 2, ternary secret of Hamming weight 32, depth 3, a batch of 2
ciphertexts encrypted on ONE limb at logp = 20 with slots uniform in the unit
square.  Keys are the model's, uploaded; the diagonal plaintexts are the
device's (CkksEngine.prepare_homdft), checked against the model's encoding up
to the rounding of a tie and handed to the model for the word-for-word runs.

MEASURED: tools/homdft_tolerance.py (profiles/homdft_tolerance.txt), eight
seeds of the CPU model, (N, depth, order) -> (slot-side, round-trip) largest
decode error at 2^20 against float64; the tolerance is 4 x.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from homdft_ref import HomDftModel, back_error, bit_reversed, packed_slots
from hybrid_ref import rotate_hybrid_ref

pytestmark = pytest.mark.gpu

MEASURED = {(256, 3, "bitrev"): (1.322e-03, 1.098e-02), (1024, 3, "bitrev"): (5.916e-03, 8.171e-02),
            (256, 1, "natural"): (4.269e-03, None)}
# the same tool: the conjugation of a fresh seven-limb ciphertext (the hybrid key-switch's own error)
MEASURED_CONJ = {256: 3.658e-03, 1024: 2.728e-02}
L, K, ALPHA, LOGP, HAMMING, DEPTH, B = 7, 2, 2, 20, 32, 3, 2


class Setup:
    def __init__(self, rn, n):
        import encoder as enc
        from rns_ntt.engine import CkksEngine

        self.rn, self.n = rn, n
        self.q, self.p = orc.generate_primes(30, L, n), orc.generate_primes(31, K, n)
        self.model = m = HomDftModel(self.q, self.p, n, ALPHA, HAMMING, seed=31 + n)
        self.engine = CkksEngine(self.q, n, hamming_weight=HAMMING, special_moduli=self.p)
        self.ext, self.basis = self.engine.ext_basis, self.engine.basis
        self.values = [m.rng.uniform(-1, 1, n // 2) + 1j * m.rng.uniform(-1, 1, n // 2) for _ in range(B)]
        self.first = [m.encrypt(enc.encode_fft(v, n, LOGP), 1) for v in self.values]
        self.low = self.basis.drop_last(L - 1)
        self.ct = self.up(self.first, self.low)
        self.raised = self.engine.mod_raise(self.ct)
        self.raised_host = [m.mod_raise(c, L) for c in self.first]
        self.a = [m.decrypt(c) for c in self.raised_host]

    def up(self, cts, basis):
        rn = self.rn
        return rn.Ciphertext(rn.RnsPoly.from_channels(np.stack([c[0] for c in cts]), basis),
                             rn.RnsPoly.from_channels(np.stack([c[1] for c in cts]), basis), LOGP, basis.total_bits())

    def key(self, step, hoisted=False):
        ka, kb = self.model.key(step)
        k = self.rn.RnsHybridKey.from_channels(ka, kb, self.ext, ALPHA, rotation=step, n_special=K)
        return k.prepare_hoisted() if hoisted else k

    def keysets(self, plan):
        rn = self.rn
        return [(rn.RnsHybridKeySet([None if s == 0 else self.key(s, True) for s in g.baby_steps], ALPHA),
                 rn.RnsHybridKeySet([None if s == 0 else self.key(s) for s in g.giant_steps], ALPHA))
                for g in plan.groups]

    def device_plaintexts(self, prepared):
        """[n2 n1][lv][N] coefficient-domain residues per group, as encoded on
        the device; each within 1 of the model's encoding (a rounding tie)."""
        out = []
        for s, pt in enumerate(prepared.plaintexts):
            c = pt.poly.clone()
            c.to_coeff_domain()
            w = c.channels_batch()
            lv = L - s if prepared.plan.direction == "coeff_to_slot" else L - DEPTH - s
            want = self.model.encode_group(prepared.plan.groups[s], lv)
            q0 = self.q[0]
            d = (w[:, 0].astype(np.int64) - want[:, 0].astype(np.int64) + q0 // 2) % q0 - q0 // 2
            assert np.abs(d).max() <= 1 and np.count_nonzero(d) <= 8, "the device plaintexts are not the model's"
            out.append(w)
        return out

    def words(self, ct):
        return ct.c0.channels_batch(), ct.c1.channels_batch()


_SETUPS = {}


@pytest.fixture(scope="module", params=[256, 1024], ids=["n8", "n10"])
def setup(gpu, request):
    if request.param not in _SETUPS:
        _SETUPS[request.param] = Setup(gpu, request.param)
    return _SETUPS[request.param]


@pytest.fixture(scope="module")
def transformed(gpu, setup):
    """The device pipeline, run once per ring and left unchanged: (c2s plan,
    slot ciphertext, s2c plan, final ciphertext, device plaintexts, launch counts)."""
    s, rn = setup, gpu
    c2s, s2c = rn.homdft_plan(s.n, "coeff_to_slot", DEPTH), rn.homdft_plan(s.n, "slot_to_coeff", DEPTH)
    names = ("moddown_rescale", "moddown", "ks_rows", "ks_whole", "ks_decompose", "bsgs_mac", "modup")
    counts = []
    pc = s.engine.prepare_homdft(c2s, s.basis)
    kc = s.keysets(c2s)
    s.basis.profile_enable(True)
    try:
        slot = s.engine.coeff_to_slot_hybrid(s.raised, pc, kc)
        counts.append({k: s.basis.profile_read(k)[0] for k in names})
    finally:
        s.basis.profile_enable(False)
    ps = s.engine.prepare_homdft(s2c, slot.c0.basis)
    ks = s.keysets(s2c)
    s.basis.profile_enable(True)
    try:
        back = s.engine.slot_to_coeff_hybrid(slot, ps, ks)
        counts.append({k: s.basis.profile_read(k)[0] for k in names})
    finally:
        s.basis.profile_enable(False)
    return dict(c2s=c2s, s2c=s2c, pc=pc, ps=ps, slot=slot, back=back, counts=counts, kc=kc, ks=ks)


def test_mod_raise_identity_on_the_device(gpu, setup):
    s = setup
    assert s.raised.c0.basis is s.basis and s.raised.logp == LOGP and s.raised.logq == s.basis.total_bits()
    w0, w1 = s.words(s.raised)
    Q0 = s.q[0]
    for b in range(B):
        assert np.array_equal(w0[b], s.raised_host[b][0]) and np.array_equal(w1[b], s.raised_host[b][1])
        m, t = s.model.decrypt(s.first[b]), s.model.decrypt((w0[b], w1[b]))
        assert all((u - v) % Q0 == 0 for u, v in zip(t, m))
        assert max(abs((u - v) // Q0) for u, v in zip(t, m)) <= (HAMMING + 1) / 2


def test_coeff_to_slot_matches_the_model_and_decodes(gpu, setup, transformed):
    s, t = setup, transformed
    slot = t["slot"]
    assert slot.c0.basis is t["pc"].bases[DEPTH] and slot.c0.basis.channel_count() == L - DEPTH
    assert slot.logp == LOGP and slot.c0.n_polys == B and not slot.c0.is_ntt_domain()
    assert slot.logq == s.raised.logq - sum(q.bit_length() for q in s.q[L - DEPTH:])
    pts = s.device_plaintexts(t["pc"])
    w0, w1 = s.words(slot)
    tol = 4 * MEASURED[(s.n, DEPTH, "bitrev")][0]
    for b in range(B):
        r0, r1 = s.model.transform(t["c2s"], s.raised_host[b], plaintexts=pts)
        assert np.array_equal(w0[b], r0) and np.array_equal(w1[b], r1), f"ciphertext {b} differs from the CPU model"
        want = bit_reversed(packed_slots(s.a[b], s.n)) / 2.0 ** LOGP
        err = float(np.max(np.abs(s.model.decode((w0[b], w1[b]), LOGP) - want)))
        print(f"N {s.n} ciphertext {b}: slot-side decode error {err:.3e} (tolerance {tol:.3e})")
        assert err < tol


def test_slot_to_coeff_matches_the_model_and_returns_a(gpu, setup, transformed):
    s, t = setup, transformed
    back = t["back"]
    assert back.c0.basis is t["ps"].bases[DEPTH] and back.c0.basis.channel_count() == 1 and back.logp == LOGP
    pts = s.device_plaintexts(t["ps"])
    s0, s1 = s.words(t["slot"])
    w0, w1 = s.words(back)
    tol = 4 * MEASURED[(s.n, DEPTH, "bitrev")][1]
    for b in range(B):
        r0, r1 = s.model.transform(t["s2c"], (s0[b], s1[b]), plaintexts=pts)
        assert np.array_equal(w0[b], r0) and np.array_equal(w1[b], r1), f"ciphertext {b} differs from the CPU model"
        err = back_error(s.model, (w0[b], w1[b]), s.a[b], LOGP)
        print(f"N {s.n} ciphertext {b}: round-trip decode error {err:.3e} (tolerance {tol:.3e})")
        assert err < tol


def test_launch_counts_are_depth_bsgs_calls_and_no_other_keyswitch(gpu, setup, transformed):
    for c in transformed["counts"]:
        print(c)
        assert c["moddown_rescale"] == 2 * DEPTH  # the closing ModDown + rescale of each call, both components
        assert c["moddown"] == 0 and c["ks_rows"] == 0 and c["ks_whole"] == 0 and c["ks_decompose"] == 0
    assert transformed["c2s"].n_keyswitches() == sum(len(b) + len(g) for b, g in transformed["c2s"].rotation_steps())


def test_natural_order_in_one_level(gpu):
    rn = gpu
    s = _SETUPS.get(256) or _SETUPS.setdefault(256, Setup(rn, 256))
    plan = rn.homdft_plan(256, "coeff_to_slot", 1, order="natural")
    prepared = s.engine.prepare_homdft(plan, s.basis)
    slot = s.engine.coeff_to_slot_hybrid(s.raised, prepared, s.keysets(plan))
    assert slot.c0.basis.channel_count() == L - 1 and slot.logp == LOGP
    w0, w1 = s.words(slot)
    tol = 4 * MEASURED[(256, 1, "natural")][0]
    for b in range(B):
        err = float(np.max(np.abs(s.model.decode((w0[b], w1[b]), LOGP) - packed_slots(s.a[b], 256) / 2.0 ** LOGP)))
        print(f"natural order, ciphertext {b}: decode error {err:.3e} (tolerance {tol:.3e})")
        assert err < tol


def test_conjugation_and_the_parts(gpu, setup):
    import encoder as enc

    rn, s = gpu, setup
    n, m = s.n, s.model
    full = [m.encrypt(enc.encode_fft(v, n, LOGP), L) for v in s.values]
    ct = s.up(full, s.basis)
    ck = s.key(-(n // 2))
    cj = rn.conjugate_hybrid(ct, ck)
    rot = rn.rotate_ciphertext_hybrid(ct, ck)
    assert all(np.array_equal(x, y) for x, y in zip(s.words(cj), s.words(rot)))
    r0, r1 = rotate_hybrid_ref(m.Bc, m.Be, *full[0], -(n // 2), *m.key(-(n // 2)), ALPHA)
    assert np.array_equal(s.words(cj)[0][0], r0) and np.array_equal(s.words(cj)[1][0], r1)
    re, im = rn.split_real_imag_hybrid(ct, ck)
    assert re.logp == im.logp == LOGP + 1 and re.logq == ct.logq
    merged = rn.merge_real_imag(re, im)
    assert merged.logp == LOGP + 1
    plus, minus = rn.mul_i(ct), rn.mul_i(ct, -1)
    assert (plus.logp, plus.logq) == (ct.logp, ct.logq)

    def dec(c, b, logp):
        w0, w1 = s.words(c)
        return m.decode((w0[b], w1[b]), logp)

    for b in range(B):
        v = s.values[b]
        e0 = float(np.max(np.abs(dec(ct, b, LOGP) - v)))
        assert e0 < 1e-3  # fresh: 3.2 sqrt(N) / 2^20 and the encoder's rounding
        tol = 4 * MEASURED_CONJ[n]
        ec = float(np.max(np.abs(dec(cj, b, LOGP) - np.conj(v))))
        print(f"N {n} ciphertext {b}: conjugation decode error {ec:.3e} (tolerance {tol:.3e})")
        assert ec < tol
        # (ct +- conj(ct)) / 2: half the sum of the two errors, below the conjugate's bound
        assert np.max(np.abs(dec(re, b, LOGP + 1) - v.real)) < tol
        assert np.max(np.abs(dec(im, b, LOGP + 1) - v.imag)) < tol
        # re + i im = 2 ct exactly, carried at logp + 1: the input's own error
        assert abs(float(np.max(np.abs(dec(merged, b, LOGP + 1) - v))) - e0) < 1e-9
        # the shift is exact: the error against i v is the input's error against v
        ep = float(np.max(np.abs(dec(plus, b, LOGP) - 1j * v)))
        em = float(np.max(np.abs(dec(minus, b, LOGP) + 1j * v)))
        print(f"N {n} ciphertext {b}: errors ct {e0:.3e}, i ct {ep:.3e}, -i ct {em:.3e}")
        assert abs(ep - e0) < 1e-9 and abs(em - e0) < 1e-9


def test_engine_layer_value_errors(gpu, setup, transformed):
    rn, s, t = gpu, setup, transformed
    from rns_ntt.engine import CkksEngine

    with pytest.raises(ValueError, match="-N/2"):
        rn.conjugate_hybrid(s.raised, s.key(1))
    with pytest.raises(ValueError, match="sign"):
        rn.mul_i(s.raised, 2)
    with pytest.raises(ValueError, match="direction"):
        CkksEngine.slot_to_coeff_hybrid(s.raised, t["pc"], t["kc"])
    with pytest.raises(ValueError, match="basis object"):
        CkksEngine.coeff_to_slot_hybrid(t["slot"], t["pc"], t["kc"])
    with pytest.raises(ValueError, match="key set pairs"):
        CkksEngine.coeff_to_slot_hybrid(s.raised, t["pc"], t["kc"][:1])
    with pytest.raises(ValueError, match="steps"):
        CkksEngine.coeff_to_slot_hybrid(s.raised, t["pc"], t["ks"])
    with pytest.raises(ValueError, match="levels"):
        s.engine.prepare_homdft(t["c2s"], s.basis.drop_last(L - DEPTH))
    with pytest.raises(ValueError, match="logp"):
        rn.merge_real_imag(s.raised, rn.Ciphertext(s.raised.c0, s.raised.c1, LOGP + 1, s.raised.logq))
    g = t["c2s"].groups[0]
    e = rn.CkksEncoder(s.n, 30)
    with pytest.raises(ValueError, match="both give diagonal"):
        CkksEngine.encode_diagonal_rows_bsgs(g.diags, [0, 1], [0, 1], e, s.basis)
    with pytest.raises(ValueError, match=r"\[0, slots\)"):
        CkksEngine.encode_diagonal_rows_bsgs(g.diags, [0, -1], [0], e, s.basis)
    with pytest.raises(ValueError, match="does not name"):
        CkksEngine.encode_diagonal_rows_bsgs(g.diags, [0], [0], e, s.basis)
