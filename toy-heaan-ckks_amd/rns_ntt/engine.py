"""Device-resident CKKS engine sequences.

Mirrors the RNS half of `CkksEngine` (src/crypto/engine.rs): key
generation (:288-399), encrypt / decrypt / add (:84-151), and the gadget
multiply, rotate and rescale already in `rns_ntt`.  Every polynomial stays
in device memory and every ring operation runs through librnsntt; only the
random samples are drawn on the host.

The samplers run on the device when ``rng`` is an ``rns_ntt.DeviceRng``
(Philox4x32-10 streams, rnt_sample_*: ternary secret with a fixed Hamming
weight, rounded Gaussian errors, uniform residues), or on the host with a
numpy Generator; neither reproduces the reference's ChaCha20 + rand_distr
streams bit-exactly.  Parity for
these paths is therefore relational: key relations and decryption error
bounds (tests/test_gpu_engine.py), as SURVEY §8f prescribes.  Plaintexts
are either scaled integer coefficients (an RnsPoly) or slot-encoded
``Plaintext``s from ``CkksEncoder`` (the device special FFT, §8f row 4).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import (Ciphertext, CkksEncoder, DeviceRng, Plaintext, RnsBasis, RnsGadgetKey, RnsGadgetKeySet, RnsHybridKey,
               RnsHybridKeySet, RnsPoly, bsgs_diagonal_rows, check, conjugate_hybrid, ct_lincomb, ct_plain_mac,
               dot_ciphertexts_hybrid, hybrid_level_moduli, linear_bsgs_hybrid_dh, linear_transform,
               linear_transform_bsgs, merge_real_imag, mul_i,
               split_real_imag_hybrid,
               linear_transform_bsgs_hoisted, linear_transform_bsgs_hybrid, linear_transform_bsgs_hybrid_rescale,
               linear_transform_hybrid, load, mul_ciphertexts_gadget, mul_ciphertexts_hybrid,
               mul_ciphertexts_hybrid_rescale, mul_ciphertexts_hybrid_rescale_affine, poly_eval_plan,
               poly_eval_plan_fused, rescale_ciphertext, rotate_ciphertext,
               rotate_ciphertext_hoisted, rotate_ciphertext_hybrid, rotate_ciphertext_hybrid_hoisted,
               rotsum_ciphertext_hybrid)


@dataclass
class PreparedHomDft:
    """A ``homdft_plan`` made ready for one top basis (``CkksEngine.prepare_homdft``):
    ``bases[s]`` is the ONE basis object of level s (group s reads its input on
    ``bases[s]`` and writes onto ``bases[s + 1]``), ``plaintexts[s]`` the BSGS
    diagonal plaintexts of group s, NTT domain, on ``bases[s]``."""

    plan: object
    bases: list
    plaintexts: list


@dataclass
class PublicKey:
    """public_key.rs: b = -a*s + e."""

    b: RnsPoly
    a: RnsPoly


def _check_levels(name: str, ct: Ciphertext, depth: int, what: str) -> None:
    """A circuit of ``depth`` levels at the scale 2^logp: enough limbs, and
    every consumed prime of logp bits."""
    p = int(ct.logp)
    mods = ct.c0.basis.moduli()
    if len(mods) - depth < 1:
        raise ValueError(f"{name}: {what} consumes {depth} levels, the ciphertext has {len(mods)} limbs")
    for q in mods[len(mods) - depth:]:
        if q.bit_length() != p:
            raise ValueError(f"{name}: the consumed prime {q} has {q.bit_length()} bits, the ciphertext's logp "
                             f"is {p}")


class CkksEngine:
    """The RNS-backend engine over one basis.

    ``error_std`` is the Gaussian width of every error sample.  The
    reference passes sqrt(error_variance) in key generation (engine.rs:316)
    but error_variance itself in encrypt (engine.rs:92).  Both call sites
    here take ``error_std``, and the caller chooses its value.

    ``special_moduli`` (K primes, none of them a ciphertext modulus) turns on
    the hybrid key-switch: ``ext_basis`` is then the basis over ``moduli +
    special_moduli`` the hybrid keys live on and ``basis`` its
    ``drop_last(K)`` view; everything else works on ``basis`` as before.
    """

    def __init__(self, moduli, degree: int, error_std: float = 3.2,
                 hamming_weight: Optional[int] = None, device: int = 0, special_moduli=None):
        self.ext_basis = None
        self._dh_bases = {}  # level -> the root basis over q_0..q_{level-1}, p (dh_plain_basis)
        self.special_moduli = [int(p) for p in special_moduli] if special_moduli is not None else []
        if self.special_moduli:
            if isinstance(moduli, RnsBasis):
                raise ValueError("special_moduli need the ciphertext moduli as a list (the extended basis is the root)")
            self.ext_basis = RnsBasis(list(moduli) + self.special_moduli, degree, device=device)
            moduli = self.ext_basis.drop_last(len(self.special_moduli))
        # an existing RnsBasis is shared, as CkksEngine::new(basis.clone(), ..)
        # shares the Arc (engine.rs:36-41): a level-l engine built on a
        # rescaled ciphertext's basis encrypts onto that same basis
        if isinstance(moduli, RnsBasis):
            if moduli.degree != degree:
                raise ValueError(f"basis degree {moduli.degree} != engine degree {degree}")
            self.basis = moduli
        else:
            self.basis = RnsBasis(list(moduli), degree, device=device)
        self.degree = degree
        self.error_std = error_std
        self.hamming_weight = hamming_weight if hamming_weight is not None else degree // 2

    # -- samplers (traits.rs PolySampler): device for a DeviceRng, else host -
    # count=None draws the reference's single polynomial, count=k a batch of k
    def _tern_poly(self, rng, count=None) -> RnsPoly:
        if isinstance(rng, DeviceRng):
            return RnsPoly.sample_tribits(self.hamming_weight, self.basis, rng, count)
        c = self._ternary(rng, count or 1)
        return RnsPoly.from_coeffs(c if count else c[0], self.basis)

    def _gauss_poly(self, rng, count=None) -> RnsPoly:
        if isinstance(rng, DeviceRng):
            return RnsPoly.sample_gaussian(self.error_std, self.basis, rng, count)
        c = self._gaussian(rng, count or 1)
        return RnsPoly.from_coeffs(c if count else c[0], self.basis)

    def _ternary(self, rng, count=1):
        n = self.degree
        out = np.zeros((count, n), dtype=np.int64)
        for c in range(count):
            idx = rng.choice(n, size=self.hamming_weight, replace=False)
            out[c, idx] = rng.choice(np.array([-1, 1], dtype=np.int64), size=self.hamming_weight)
        return out

    def _gaussian(self, rng, count=1):
        return np.rint(rng.normal(0.0, self.error_std, size=(count, self.degree))).astype(np.int64)

    def _uniform(self, rng, count=None, basis: Optional[RnsBasis] = None):
        b = basis or self.basis
        if isinstance(rng, DeviceRng):
            return RnsPoly.sample_uniform(b, rng, count)
        q = np.array(b.moduli(), dtype=np.uint64)[None, :, None]
        ch = rng.integers(0, 1 << 62, size=(count or 1, len(b.moduli()), self.degree), dtype=np.uint64) % q
        return RnsPoly.from_channels(ch if count else ch[0], b)

    # -- keys (engine.rs:288-399, keys/*.rs) ---------------------------------
    def generate_secret_key(self, rng) -> RnsPoly:
        return self._tern_poly(rng)

    def generate_public_key(self, sk: RnsPoly, rng) -> PublicKey:
        a = self._uniform(rng)
        b = -(a * sk) + self._gauss_poly(rng)
        return PublicKey(b, a)

    def _gadget_key(self, sk: RnsPoly, target: RnsPoly, rng, rotation=None) -> RnsGadgetKey:
        """b_i = -(a_i s) + e_i + e_i-plaintext(target) for every channel i,
        as one batch of L polys on the device."""
        L, n = self.basis.channel_count(), self.degree
        t = target.channels()  # [L][N], coefficient domain
        plain = np.zeros((L, L, n), dtype=np.uint64)
        for i in range(L):
            plain[i, i] = t[i]
        s_rep = RnsPoly.from_channels(np.broadcast_to(sk.channels(), (L, L, n)).copy(), self.basis)
        a = self._uniform(rng, count=L)
        e = self._gauss_poly(rng, count=L)
        b = -(a * s_rep) + e + RnsPoly.from_channels(plain, self.basis)
        return RnsGadgetKey(a, b, rotation)

    def generate_gadget_relin_key(self, sk: RnsPoly, rng) -> RnsGadgetKey:
        return self._gadget_key(sk, sk * sk, rng)

    def generate_gadget_rotation_key(self, sk: RnsPoly, rotation: int, rng) -> RnsGadgetKey:
        return self._gadget_key(sk, sk.rotate_slots(rotation), rng, rotation)

    # -- hybrid keys (special primes) -----------------------------------------
    def _lift(self, poly: RnsPoly, basis: RnsBasis, count: int) -> RnsPoly:
        """``count`` copies of a small polynomial (a secret, a product of
        secrets) on ``basis``, from its centred coefficients."""
        c = np.array(poly.to_coeffs_exact(), dtype=object).reshape(-1)
        mods = basis.moduli()
        ch = np.stack([np.array([int(v) % m for v in c], dtype=np.uint64) for m in mods])
        return RnsPoly.from_channels(np.broadcast_to(ch, (count,) + ch.shape).copy(), basis)

    def _hybrid_key(self, sk: RnsPoly, target: RnsPoly, rng, alpha: int, rotation=None) -> RnsHybridKey:
        """b_d = -(a_d s) + e_d + G_d for every digit d as one batch of beta
        polys on ext_basis: limb t of G_d is P s' mod q_t on the limbs of
        digit d and zero elsewhere (every special limb included)."""
        if self.ext_basis is None:
            raise ValueError("hybrid keys need an engine built with special_moduli")
        alpha = int(alpha)
        if alpha < 1:
            raise ValueError("alpha must be at least 1")
        q = self.basis.moduli()
        L, K, n = len(q), len(self.special_moduli), self.degree
        beta = -(-L // alpha)
        P = 1
        for p in self.special_moduli:
            P *= p
        qd_max = 1
        for d in range(beta):
            qd = 1
            for i in range(d * alpha, min((d + 1) * alpha, L)):
                qd *= q[i]
            qd_max = max(qd_max, qd)
        if P < alpha * qd_max:
            raise ValueError(f"the special primes are too small for alpha = {alpha}: P has {P.bit_length()} bits, "
                             f"alpha max Q_d {(alpha * qd_max).bit_length()}")
        t = target.channels()  # [L][N]: s' mod q_t, coefficient domain
        plain = np.zeros((beta, L + K, n), dtype=np.uint64)
        for d in range(beta):
            for i in range(d * alpha, min((d + 1) * alpha, L)):
                plain[d, i] = np.array([int(v) * (P % q[i]) % q[i] for v in t[i]], dtype=np.uint64)
        s_rep = self._lift(sk, self.ext_basis, beta)
        a = self._uniform(rng, count=beta, basis=self.ext_basis)
        if isinstance(rng, DeviceRng):
            e = RnsPoly.sample_gaussian(self.error_std, self.ext_basis, rng, beta)
        else:
            e = RnsPoly.from_coeffs(self._gaussian(rng, beta), self.ext_basis)
        b = -(a * s_rep) + e + RnsPoly.from_channels(plain, self.ext_basis)
        return RnsHybridKey(a, b, alpha, rotation, n_special=K)

    def generate_hybrid_relin_key(self, sk: RnsPoly, rng, alpha: int) -> RnsHybridKey:
        return self._hybrid_key(sk, sk * sk, rng, alpha)

    def generate_hybrid_rotation_key(self, sk: RnsPoly, rotation: int, rng, alpha: int) -> RnsHybridKey:
        return self._hybrid_key(sk, sk.rotate_slots(rotation), rng, alpha, rotation)

    def generate_hybrid_conjugation_key(self, sk: RnsPoly, rng, alpha: int) -> RnsHybridKey:
        """The hybrid rotation key of step ``-N/2``: its automorphism exponent
        is ``5^(N/2) (2N - 1) = 2N - 1 mod 2N``, the conjugation, so every
        hybrid rotation call conjugates with it (``conjugate_hybrid``)."""
        return self.generate_hybrid_rotation_key(sk, -(self.degree // 2), rng, alpha)

    conjugate_hybrid = staticmethod(conjugate_hybrid)
    mul_i = staticmethod(mul_i)
    split_real_imag_hybrid = staticmethod(split_real_imag_hybrid)
    merge_real_imag = staticmethod(merge_real_imag)

    def mod_raise(self, ct: Ciphertext, basis: Optional[RnsBasis] = None) -> Ciphertext:
        """ModRaise: both components of a ciphertext on 1..4 limbs as the same
        centred integers on ``basis`` (default: the engine's), rnt_mod_raise.
        The result decrypts to ``m + Q0 I`` with a small integer polynomial I
        (|I| <= (h + 1) / 2 for a secret of Hamming weight h): the input of
        CoeffToSlot.  logp is unchanged, logq the new basis' bits."""
        b = basis if basis is not None else self.basis
        return Ciphertext(ct.c0.mod_raise(b), ct.c1.mod_raise(b), ct.logp, b.total_bits())

    rotate_ciphertext_hybrid = staticmethod(rotate_ciphertext_hybrid)
    mul_ciphertexts_hybrid = staticmethod(mul_ciphertexts_hybrid)
    mul_ciphertexts_hybrid_rescale = staticmethod(mul_ciphertexts_hybrid_rescale)
    dot_ciphertexts_hybrid = staticmethod(dot_ciphertexts_hybrid)

    def generate_hybrid_rotation_key_set(self, sk: RnsPoly, steps, rng, alpha: int,
                                         hoisted: bool = False) -> RnsHybridKeySet:
        """One hybrid rotation key per step, packed for the hoisted hybrid
        calls (no key for a step of 0); with ``hoisted`` every key in its
        hoisting form, for ``rotate_hoisted_hybrid``, ``linear_transform_hybrid``
        and the baby keys of ``linear_transform_bsgs_hybrid``."""
        keys = [None if int(s) == 0 else self.generate_hybrid_rotation_key(sk, int(s), rng, alpha) for s in steps]
        if hoisted:
            for k in keys:
                if k is not None:
                    k.prepare_hoisted()
        return RnsHybridKeySet(keys, alpha)

    @staticmethod
    def rotate_hoisted_hybrid(ct: Ciphertext, keyset: RnsHybridKeySet) -> Ciphertext:
        """Every ciphertext of the batch rotated by each of the key set's
        steps with one ModUp: a batch of ``n_steps * B``, rotation t of
        ciphertext b at ``t * B + b``."""
        return rotate_ciphertext_hybrid_hoisted(ct, keyset)

    def generate_rotsum_key_sets(self, sk: RnsPoly, plan, rng, alpha: int) -> list:
        """One ORDINARY hybrid key set per stage of a ``rotsum_plan`` (its
        steps, the leading 0 without a key), for ``inner_sum_hybrid``.  The
        caller's trade-off is the plan's radix: radix 2 needs ``log2 n`` keys
        and ``log2 n`` ModUps, radix r ``(r - 1) log_r n`` keys and ``log_r n``
        ModUps; a key is ``2 beta (Lv + K)`` planes (72 MiB at 2^16 x (16 + 2)
        limbs, alpha = 2, 32-bit words)."""
        if plan.stages[-1][-1] >= self.degree // 2:
            raise ValueError("generate_rotsum_key_sets: a step of the plan reaches the ring's N/2 slots")
        return [self.generate_hybrid_rotation_key_set(sk, st, rng, alpha) for st in plan.stages]

    @staticmethod
    def inner_sum_hybrid(ct: Ciphertext, plan, keysets) -> Ciphertext:
        """``sum_{t < plan.n} rotate(ct, t plan.stride)``: slot j of the result
        holds the sum of slots ``j, j + stride, ..., j + (n - 1) stride`` of
        ``ct`` (indices mod N/2).  One ``rotsum_ciphertext_hybrid`` per stage of
        the plan, the stages after the first in place on one output
        ciphertext.  Scale and level are unchanged: no plaintext, no
        rescale."""
        if len(keysets) != len(plan.stages):
            raise ValueError(f"inner_sum_hybrid: {len(keysets)} key sets for {len(plan.stages)} stages")
        for u, (ks, st) in enumerate(zip(keysets, plan.stages)):
            if list(ks.steps) != list(st):
                raise ValueError(f"inner_sum_hybrid: the key set of stage {u} is not for the plan's steps")
        out = None
        for ks in keysets:
            out = rotsum_ciphertext_hybrid(ct if out is None else out, ks, out=out)
        return out

    @staticmethod
    def linear_transform_hybrid(ct: Ciphertext, diag_plaintexts: Plaintext, keyset: RnsHybridKeySet) -> Ciphertext:
        """``sum_k diag_k * rotate(ct, k)`` over the (hoisting-form) key set's
        steps on hybrid keys; logp grows by the diagonals' scale."""
        out = linear_transform_hybrid(ct, diag_plaintexts.poly, keyset)
        out.logp = ct.logp + diag_plaintexts.scale_bits
        return out

    @staticmethod
    def linear_transform_bsgs_hybrid(ct: Ciphertext, diag_plaintexts: Plaintext, baby_keyset: RnsHybridKeySet,
                                     giant_keyset: RnsHybridKeySet) -> Ciphertext:
        """``linear_transform_bsgs`` on hybrid keys (baby keys in hoisting
        form, giant keys ordinary; ``encode_diagonals_bsgs`` gives the
        plaintexts): one ModUp for all the babies, one ModDown for all the
        giants; logp grows by the diagonals' scale."""
        out = linear_transform_bsgs_hybrid(ct, diag_plaintexts.poly, baby_keyset, giant_keyset)
        out.logp = ct.logp + diag_plaintexts.scale_bits
        return out

    @staticmethod
    def linear_transform_bsgs_hybrid_rescale(ct: Ciphertext, diag_plaintexts: Plaintext,
                                             baby_keyset: RnsHybridKeySet,
                                             giant_keyset: RnsHybridKeySet,
                                             out_basis: Optional[RnsBasis] = None) -> Ciphertext:
        """``linear_transform_bsgs_hybrid`` then ``rescale_ciphertext`` as one
        op, word for word: logp grows by the diagonals' scale and drops, with
        logq, by the bits of the limb rescaled away.  ``out_basis`` (a
        ``drop_last(1)`` of the input's basis) receives the result where a
        circuit keeps one basis object per level."""
        out = linear_transform_bsgs_hybrid_rescale(ct, diag_plaintexts.poly, baby_keyset, giant_keyset,
                                                   out_basis=out_basis)
        out.logp += diag_plaintexts.scale_bits
        return out

    # -- CoeffToSlot / SlotToCoeff (rns_ntt/homdft.py) ---------------------------
    @staticmethod
    def encode_diagonal_rows_bsgs(diags, baby_steps, giant_steps, encoder: CkksEncoder, basis: RnsBasis) -> Plaintext:
        """The sparse twin of ``encode_diagonals_bsgs``: ``diags`` maps a step
        in ``[0, slots)`` to that diagonal of the matrix (``d_k[s] = M[s][(s +
        k) mod slots]``).  Row ``(j, i)`` is diagonal ``g_j + b_i`` rotated
        back by ``g_j`` -- ``bsgs_diagonal_rows``' rule -- and a diagonal that
        is absent a zero plaintext.  One batch on ``basis``, poly ``j n1 + i``,
        NTT domain."""
        slots = encoder.max_slots()
        baby, giant = [int(b) for b in baby_steps], [int(g) for g in giant_steps]
        if not baby or not giant:
            raise ValueError("encode_diagonal_rows_bsgs: no steps")
        if any(not 0 <= k < slots for k in baby + giant):
            raise ValueError("encode_diagonal_rows_bsgs: every step must be in [0, slots) (slots - k for a rotation "
                             "by -k)")
        rows = np.zeros((len(giant), len(baby), slots), dtype=np.complex128)
        seen = {}
        for j, g in enumerate(giant):
            for i, b in enumerate(baby):
                d = (g + b) % slots
                if d in seen:
                    raise ValueError(f"encode_diagonal_rows_bsgs: pairs {seen[d]} and {(j, i)} both give diagonal {d}")
                seen[d] = (j, i)
                if d in diags:
                    v = np.asarray(diags[d])
                    if v.shape != (slots,):
                        raise ValueError(f"encode_diagonal_rows_bsgs: diagonal {d} must hold {slots} values")
                    rows[j, i] = np.roll(v, g)  # rows[j][i][s] = d[(s - g_j) mod slots]
        missing = [d for d in diags if int(d) % slots not in seen and np.any(np.asarray(diags[d]) != 0)]
        if missing:
            raise ValueError(f"encode_diagonal_rows_bsgs: the grid does not name the nonzero diagonals {sorted(missing)}")
        pt = encoder.encode_complex(rows.reshape(-1, slots), basis)
        pt.poly.to_ntt_domain()
        return pt

    def prepare_homdft(self, plan, top_basis: RnsBasis) -> PreparedHomDft:
        """Encode every group of ``plan`` on the level basis it runs on: group
        s on ``top_basis`` less s limbs, ONE basis object per level, all kept.
        Group s is encoded at ``scale_bits`` = the bit length of the prime q its
        rescale removes, so logp leaves every group as it came; its diagonals
        are first multiplied by ``q / 2^scale_bits``, which makes the encoding
        scale q itself: the rescale divides by q, not by 2^scale_bits, and
        without the factor every group would scale the whole plaintext -- the
        large ``Q0 I`` of a raised ciphertext included -- by ``2^scale_bits / q``."""
        return self._prepare_homdft("prepare_homdft", plan, top_basis, lambda s, bases: bases[s])

    def _prepare_homdft(self, name: str, plan, top_basis: RnsBasis, plain_basis) -> PreparedHomDft:
        """The level bases of ``plan`` under ``top_basis`` and every group's
        diagonals, group s encoded on ``plain_basis(s, bases)``."""
        mods = top_basis.moduli()
        if len(mods) - plan.depth < 1:
            raise ValueError(f"{name}: the plan consumes {plan.depth} levels, the basis has {len(mods)} limbs")
        if top_basis.degree != plan.degree:
            raise ValueError(f"{name}: the plan is for degree {plan.degree}, the basis has {top_basis.degree}")
        bases = [top_basis] + [top_basis.drop_last(s) for s in range(1, plan.depth + 1)]
        pts = []
        for s, g in enumerate(plan.groups):
            q = mods[len(mods) - 1 - s]
            enc = CkksEncoder(plan.degree, q.bit_length())
            drift = q / 2.0 ** q.bit_length()
            diags = {k: v * drift for k, v in g.diags.items()}
            pts.append(self.encode_diagonal_rows_bsgs(diags, g.baby_steps, g.giant_steps, enc, plain_basis(s, bases)))
        return PreparedHomDft(plan, bases, pts)

    def generate_homdft_key_sets(self, sk: RnsPoly, plan, rng, alpha: int) -> list:
        """Per group ``(baby_keyset, giant_keyset)`` for the plan's steps: baby
        keys in hoisting form, giant keys ordinary."""
        return [(self.generate_hybrid_rotation_key_set(sk, g.baby_steps, rng, alpha, hoisted=True),
                 self.generate_hybrid_rotation_key_set(sk, g.giant_steps, rng, alpha)) for g in plan.groups]

    @staticmethod
    def _homdft_hybrid(ct: Ciphertext, prepared: PreparedHomDft, keysets, direction: str, name: str,
                       group_call=None) -> Ciphertext:
        """Every group of the plan as one ``group_call`` (by default
        ``linear_transform_bsgs_hybrid_rescale``; the double-hoisted one for
        the ``_dh`` transforms)."""
        group_call = group_call or CkksEngine.linear_transform_bsgs_hybrid_rescale
        plan = prepared.plan
        if plan.direction != direction:
            raise ValueError(f"{name}: the plan's direction is {plan.direction!r}")
        if len(keysets) != len(plan.groups):
            raise ValueError(f"{name}: {len(keysets)} key set pairs for {len(plan.groups)} groups")
        if ct.c0.basis is not prepared.bases[0]:
            raise ValueError(f"{name}: the ciphertext is not on the basis object the plan was prepared for")
        for s, (pt, (bk, gk)) in enumerate(zip(prepared.plaintexts, keysets)):
            if list(bk.steps) != list(plan.groups[s].baby_steps) or list(gk.steps) != list(plan.groups[s].giant_steps):
                raise ValueError(f"{name}: the key sets of group {s} are not for the plan's steps")
            ct = group_call(ct, pt, bk, gk, out_basis=prepared.bases[s + 1])
        return ct

    @staticmethod
    def coeff_to_slot_hybrid(ct: Ciphertext, prepared: PreparedHomDft, keysets) -> Ciphertext:
        """CoeffToSlot: the slots of the result hold ``a_j + i a_{j+n}`` over
        ``2^logp`` (bit-reversed in j with ``order="bitrev"``) for the
        polynomial ``a`` that ``ct`` decrypts to.  One
        ``linear_transform_bsgs_hybrid_rescale`` per group; ``plan.depth``
        levels down, logp unchanged."""
        return CkksEngine._homdft_hybrid(ct, prepared, keysets, "coeff_to_slot", "coeff_to_slot_hybrid")

    @staticmethod
    def slot_to_coeff_hybrid(ct: Ciphertext, prepared: PreparedHomDft, keysets) -> Ciphertext:
        """SlotToCoeff, the inverse: a ciphertext whose slots hold ``(a_j + i
        a_{j+n}) / 2^logp`` becomes one that decrypts to ``a``."""
        return CkksEngine._homdft_hybrid(ct, prepared, keysets, "slot_to_coeff", "slot_to_coeff_hybrid")

    # -- the double-hoisted transform (rnt_ct_linear_bsgs_hybrid_dh) --------------
    def dh_plain_basis(self, level: Optional[int] = None) -> RnsBasis:
        """The basis the double-hoisted transform's plaintexts are encoded on
        for a ciphertext of ``level`` limbs: ``q_0..q_{level-1}`` followed by
        the special primes.  At the top level it is ``ext_basis``; below it a
        root basis over those moduli (``hybrid_level_moduli``), one object per
        level, kept.  Such a root is a full context -- its own transform tables
        for every limb and its own stream -- made only to hold plaintexts: a
        level context cannot hold them (it carries key views alone).  The
        library orders a call after the plaintexts' stream."""
        if self.ext_basis is None:
            raise ValueError("dh_plain_basis: the engine has no special_moduli")
        top = self.basis.channel_count()
        level = top if level is None else int(level)
        if level == top:
            return self.ext_basis
        cache = self._dh_bases
        if level not in cache:
            cache[level] = RnsBasis(hybrid_level_moduli(self.ext_basis, len(self.special_moduli), level), self.degree,
                                    device=self.ext_basis.device)
        return cache[level]

    @staticmethod
    def linear_transform_bsgs_hybrid_dh(ct: Ciphertext, diag_plaintexts: Plaintext, baby_keyset: RnsHybridKeySet,
                                        giant_keyset: RnsHybridKeySet) -> Ciphertext:
        """``linear_transform_bsgs_hybrid`` double-hoisted: the same key sets,
        the plaintexts encoded on ``dh_plain_basis(level of ct)``
        (``encode_diagonal_rows_bsgs(..., basis=that)``); logp grows by the
        diagonals' scale."""
        out = linear_bsgs_hybrid_dh(ct, diag_plaintexts.poly, baby_keyset, giant_keyset)
        out.logp = ct.logp + diag_plaintexts.scale_bits
        return out

    @staticmethod
    def linear_transform_bsgs_hybrid_dh_rescale(ct: Ciphertext, diag_plaintexts: Plaintext,
                                                baby_keyset: RnsHybridKeySet, giant_keyset: RnsHybridKeySet,
                                                out_basis: Optional[RnsBasis] = None) -> Ciphertext:
        """``linear_transform_bsgs_hybrid_dh`` then ``rescale_ciphertext`` as
        one op, word for word; logp, logq and ``out_basis`` as
        ``linear_transform_bsgs_hybrid_rescale``."""
        out = linear_bsgs_hybrid_dh(ct, diag_plaintexts.poly, baby_keyset, giant_keyset, rescale=True,
                                    out_basis=out_basis)
        out.logp += diag_plaintexts.scale_bits
        return out

    def prepare_homdft_dh(self, plan, top_basis: RnsBasis) -> PreparedHomDft:
        """``prepare_homdft`` for the double-hoisted path: the same level bases
        and the same diagonals, group s encoded over ``Q_l u P`` at its level
        (``plaintexts[s]`` on ``dh_plain_basis(l)``, l = the top basis' limbs
        less s).  ``top_basis`` holds a prefix of the engine's moduli."""
        mods = top_basis.moduli()
        if mods != self.basis.moduli()[: len(mods)]:
            raise ValueError("prepare_homdft_dh: the top basis does not hold a prefix of the engine's moduli")
        return self._prepare_homdft("prepare_homdft_dh", plan, top_basis,
                                    lambda s, bases: self.dh_plain_basis(len(mods) - s))

    @staticmethod
    def coeff_to_slot_hybrid_dh(ct: Ciphertext, prepared: PreparedHomDft, keysets) -> Ciphertext:
        """``coeff_to_slot_hybrid`` with every group one
        ``linear_transform_bsgs_hybrid_dh_rescale`` call: ``prepared`` from
        ``prepare_homdft_dh``, the SAME key sets."""
        return CkksEngine._homdft_hybrid(ct, prepared, keysets, "coeff_to_slot", "coeff_to_slot_hybrid_dh",
                                         CkksEngine.linear_transform_bsgs_hybrid_dh_rescale)

    @staticmethod
    def slot_to_coeff_hybrid_dh(ct: Ciphertext, prepared: PreparedHomDft, keysets) -> Ciphertext:
        """``slot_to_coeff_hybrid`` on the double-hoisted calls."""
        return CkksEngine._homdft_hybrid(ct, prepared, keysets, "slot_to_coeff", "slot_to_coeff_hybrid_dh",
                                         CkksEngine.linear_transform_bsgs_hybrid_dh_rescale)

    # -- polynomial evaluation -------------------------------------------------
    ct_lincomb = staticmethod(ct_lincomb)

    @staticmethod
    def evaluate_polynomial_hybrid(ct: Ciphertext, coeffs, rlk: RnsHybridKey, basis: str = "monomial") -> Ciphertext:
        """``p(ct)`` for every ciphertext of the batch, ``p = sum_k coeffs[k]
        Phi_k`` with ``Phi_k = x^k`` (``basis="monomial"``) or the Chebyshev
        ``T_k`` (``"chebyshev"``), degree >= 1: the Paterson-Stockmeyer
        schedule of ``poly_eval_plan`` on ``mul_ciphertexts_hybrid_rescale``,
        ``ct_lincomb`` and additions.  ``rlk`` is one full-level hybrid
        relinearisation key with ``n_special``: it picks each multiply's level
        by itself.  Every ciphertext prime the circuit consumes (the last
        ``plan.depth`` of ``ct``'s basis) must have bit length ``ct.logp``, so
        the scale stays 2^logp (up to the drift of q != 2^logp, which the
        integer logp does not track); the result is ``plan.depth`` levels
        down."""
        plan = poly_eval_plan(coeffs, basis, int(ct.logp))
        _check_levels("evaluate_polynomial_hybrid", ct, plan.depth, f"degree {plan.degree}")
        return CkksEngine._run_poly_plan(ct, plan, rlk)[0]

    @staticmethod
    def evaluate_polynomial_hybrid_fused(ct: Ciphertext, coeffs, rlk: RnsHybridKey,
                                         basis: str = "monomial") -> Ciphertext:
        """:meth:`evaluate_polynomial_hybrid` on ``poly_eval_plan_fused``: the
        same arguments, rules, depth and leaves, with every affine step after
        a product riding in the product's own call
        (``mul_ciphertexts_hybrid_rescale_affine``) -- the same values from
        fewer launches and less traffic; in the Chebyshev basis the very words
        of the unfused evaluation."""
        plan = poly_eval_plan_fused(coeffs, basis, int(ct.logp))
        _check_levels("evaluate_polynomial_hybrid_fused", ct, plan.depth, f"degree {plan.degree}")
        return CkksEngine._run_poly_plan(ct, plan, rlk)[0]

    @staticmethod
    def _run_poly_plan(ct: Ciphertext, plan, rlk: RnsHybridKey):
        """The ops of a ``PolyEvalPlan`` on the device: the result and the one
        basis object per level it was computed on (a later call that joins the
        result with another operand needs the same object)."""
        p = int(ct.logp)
        top = ct.c0.basis
        mods = top.moduli()
        B = ct.c0.n_polys
        level_basis = {0: top}  # one basis object per level: operands of a call share it

        def lb(level):
            if level not in level_basis:
                level_basis[level] = top.drop_last(level)
            return level_basis[level]

        def drop(poly, basis_to):
            out = poly._like(basis_to)
            check(load().rnt_mod_drop_last(out.handle, poly.handle))
            return out

        v = {"x": ct}
        for op in plan.ops:
            if op[0] == "drop":
                _, dst, src, level = op
                s = v[src]
                bits = sum(q.bit_length() for q in mods[len(mods) - level:len(mods) - plan.levels[src]])
                v[dst] = Ciphertext(drop(s.c0, lb(level)), drop(s.c1, lb(level)), s.logp, s.logq - bits)
            elif op[0] == "mul":
                _, dst, a, b = op
                v[dst] = mul_ciphertexts_hybrid_rescale(v[a], v[b], rlk, out_basis=lb(plan.levels[dst]))
            elif op[0] == "add":
                _, dst, a, b = op
                v[dst] = CkksEngine.add_ciphertexts(v[a], v[b])
            elif op[0] == "fma":
                _, dst, a, b, w, z, u, bias, _ = op
                v[dst] = mul_ciphertexts_hybrid_rescale_affine(v[a], v[b], rlk, w, None if z is None else v[z], u,
                                                               bias, out_basis=lb(plan.levels[dst]))
            else:
                _, dsts, srcs, weights, bias, rescale, _, _ = op
                if len(srcs) == 1:
                    packed = v[srcs[0]]
                else:
                    here = lb(plan.levels[srcs[0]])
                    c0, c1 = RnsPoly(here, len(srcs) * B, _uninit=True), RnsPoly(here, len(srcs) * B, _uninit=True)
                    for i, s in enumerate(srcs):
                        c0.copy_polys(v[s].c0, i * B, 0, B)
                        c1.copy_polys(v[s].c1, i * B, 0, B)
                    packed = Ciphertext(c0, c1, v[srcs[0]].logp, v[srcs[0]].logq)
                out = ct_lincomb(packed, len(srcs), weights, bias, rescale=rescale, out_basis=lb(plan.levels[dsts[0]]))
                if rescale:
                    out.logp += p  # the weights' scale
                for j, d in enumerate(dsts):
                    if len(dsts) == 1:
                        v[d] = out
                        break
                    c0, c1 = RnsPoly(out.c0.basis, B, _uninit=True), RnsPoly(out.c0.basis, B, _uninit=True)
                    c0.copy_polys(out.c0, 0, j * B, B)
                    c1.copy_polys(out.c1, 0, j * B, B)
                    v[d] = Ciphertext(c0, c1, out.logp, out.logq)
        return v[plan.result], lb

    @staticmethod
    def eval_mod_hybrid(ct: Ciphertext, plan, rlk: RnsHybridKey) -> Ciphertext:
        """The homomorphic modular reduction of bootstrapping (EvalMod) on
        every ciphertext of the batch -- the real and imaginary halves of a
        split ciphertext go through as one batch of 2 B.  ``plan`` is an
        ``evalmod_plan(K, degree, r, ct.logp)``: real slots u = (I + eps) / K
        with an integer |I| < K come back as sin(2 pi eps) / (2 pi), close to
        eps.  The fused Chebyshev evaluation of the scaled cosine, then r
        double angles y <- 2 y^2 - a^(2^(j+1)), each ONE
        ``mul_ciphertexts_hybrid_rescale_affine``.  The result is
        ``plan.depth`` levels down with logp unchanged; every consumed prime
        must have ``ct.logp`` bits, as ``evaluate_polynomial_hybrid`` demands."""
        if int(ct.logp) != plan.logp:
            raise ValueError(f"eval_mod_hybrid: the plan was made for logp {plan.logp}, the ciphertext's is {ct.logp}")
        _check_levels("eval_mod_hybrid", ct, plan.depth, f"EvalMod (K = {plan.K}, degree {plan.degree}, "
                                                         f"{plan.double_angles} double angles)")
        y, lb = CkksEngine._run_poly_plan(ct, plan.poly, rlk)
        for j, c in enumerate(plan.constants):
            y = mul_ciphertexts_hybrid_rescale_affine(y, y, rlk, 2, None, 0, -c, out_basis=lb(plan.poly.depth + j + 1))
        return y

    # -- encryption (engine.rs:84-127) -----------------------------------------
    def encrypt(self, plaintext, pk: PublicKey, rng, logp: int = 0,
                logq: Optional[int] = None) -> Ciphertext:
        """``plaintext`` is an RnsPoly (with ``logp``) or a Plaintext, whose
        scale_bits become the ciphertext's logp (engine.rs:84-112)."""
        if isinstance(plaintext, Plaintext):
            logp, plaintext = plaintext.scale_bits, plaintext.poly
        u = self._tern_poly(rng)
        e0 = self._gauss_poly(rng)
        e1 = self._gauss_poly(rng)
        c0 = pk.b * u + e0 + plaintext
        c1 = pk.a * u + e1
        return Ciphertext(c0, c1, logp, self.basis.total_bits() if logq is None else logq)

    @staticmethod
    def decrypt(ct: Ciphertext, sk: RnsPoly) -> RnsPoly:
        """m = c0 + c1 * s (engine.rs:114-127); sk must share ct's basis."""
        return ct.c1 * sk + ct.c0

    @staticmethod
    def decrypt_plaintext(ct: Ciphertext, sk: RnsPoly) -> Plaintext:
        """engine.rs:114-128: the decryption as a Plaintext with
        scale_bits = logp and all N/2 slots, ready for CkksEncoder.decode."""
        return Plaintext(CkksEngine.decrypt(ct, sk), ct.logp, ct.c0.basis.degree // 2)

    @staticmethod
    def add_ciphertexts(ct1: Ciphertext, ct2: Ciphertext) -> Ciphertext:
        assert ct1.logp == ct2.logp, "logp mismatch in addition"
        assert ct1.logq == ct2.logq, "logq mismatch in addition"
        return Ciphertext(ct1.c0 + ct2.c0, ct1.c1 + ct2.c1, ct1.logp, ct1.logq)

    # -- ciphertext x plaintext (rnt_ct_plain_mac) -----------------------------
    @staticmethod
    def prepare_plaintext(pt: Plaintext) -> Plaintext:
        """A copy of ``pt`` in the NTT domain, the form ``mul_plaintext`` and
        ``plain_mac`` read: made once per weight, used by every call."""
        poly = pt.poly.clone()
        if not poly.is_ntt_domain():
            poly.to_ntt_domain()
        return Plaintext(poly, pt.scale_bits, pt.slots)

    @staticmethod
    def plain_mac(ct: Ciphertext, n_terms: int, pt: Plaintext, bias: Optional[Plaintext] = None,
                  rescale: bool = True) -> Ciphertext:
        """``sum_i ct_i (.) pt_i + bias`` slot by slot over the ``n_terms``
        ciphertexts packed in ``ct`` (term i of ciphertext b at ``i * B + b``,
        as ``rotate_hoisted_hybrid`` writes them): ``pt`` holds ``n_terms``
        plaintexts for the whole batch or ``n_terms * B``, ``bias`` one or
        ``B``.  A coefficient-domain plaintext is converted on the fly
        (``prepare_plaintext`` does it once).  logp grows by the plaintexts'
        scale, which a bias must carry too, and with ``rescale`` drops, with
        logq, by the bits of the limb rescaled away."""
        if bias is not None and bias.scale_bits != ct.logp + pt.scale_bits:
            raise ValueError(f"plain_mac: a bias at scale 2^{bias.scale_bits} for products at scale "
                             f"2^{ct.logp + pt.scale_bits}")
        if not pt.poly.is_ntt_domain():
            pt = CkksEngine.prepare_plaintext(pt)
        if bias is not None and not bias.poly.is_ntt_domain():
            bias = CkksEngine.prepare_plaintext(bias)
        out = ct_plain_mac(ct, n_terms, pt.poly, None if bias is None else bias.poly, rescale)
        out.logp += pt.scale_bits
        return out

    @staticmethod
    def mul_plaintext(ct: Ciphertext, pt: Plaintext, rescale: bool = True) -> Ciphertext:
        """``ct (.) pt`` slot by slot: ``plain_mac`` with one term."""
        return CkksEngine.plain_mac(ct, 1, pt, None, rescale)

    @staticmethod
    def add_plaintext(ct: Ciphertext, pt: Plaintext) -> Ciphertext:
        """``ct + pt`` slot by slot: the plaintext, in the coefficient domain
        and at the ciphertext's scale, is added to c0."""
        assert ct.logp == pt.scale_bits, "logp mismatch in plaintext addition"
        poly = pt.poly
        if poly.is_ntt_domain():
            poly = poly.clone()
            poly.to_coeff_domain()
        return Ciphertext(ct.c0 + poly, ct.c1.clone(), ct.logp, ct.logq)

    # the gadget multiply / rotate / rescale are the library calls
    mul_ciphertexts_gadget = staticmethod(mul_ciphertexts_gadget)
    rotate_ciphertext = staticmethod(rotate_ciphertext)
    rescale_ciphertext = staticmethod(rescale_ciphertext)

    # -- linear transforms (the diagonal method) -----------------------------
    def generate_rotation_key_set(self, sk: RnsPoly, steps, rng, hoisted: bool = False) -> RnsGadgetKeySet:
        """One gadget rotation key per step, packed for ``linear_transform``
        (no key for a step of 0); with ``hoisted`` every key in its hoisting
        form, for ``rotate_hoisted`` and the baby keys of
        ``linear_transform_bsgs_hoisted``."""
        keys = [None if int(s) == 0 else self.generate_gadget_rotation_key(sk, int(s), rng) for s in steps]
        if hoisted:
            for k in keys:
                if k is not None:
                    k.prepare_hoisted()
        return RnsGadgetKeySet(keys, self.basis)

    @staticmethod
    def rotate_hoisted(ct: Ciphertext, keyset: RnsGadgetKeySet) -> Ciphertext:
        """Every ciphertext of the batch rotated by each of the key set's
        steps with one gadget decomposition: a batch of ``n_steps * B``,
        rotation t of ciphertext b at ``t * B + b``."""
        return rotate_ciphertext_hoisted(ct, keyset)

    def encode_diagonals(self, matrix, steps, encoder: CkksEncoder) -> Plaintext:
        """The diagonal plaintexts of a slots x slots matrix for the steps of
        a key set: ``diag_k[i] = M[i][(i + k) mod slots]`` (slot i of a
        rotation by k holds old slot i + k), encoded as one batch, one poly
        per step, and moved to the NTT domain."""
        m = np.asarray(matrix)
        slots = m.shape[0]
        if m.ndim != 2 or m.shape[1] != slots or slots != encoder.max_slots():
            raise ValueError("encode_diagonals: the matrix must be slots x slots with slots = N / 2")
        i = np.arange(slots)
        rows = np.stack([m[i, (i + int(k)) % slots] for k in steps])
        pt = encoder.encode_complex(rows, self.basis)
        pt.poly.to_ntt_domain()
        return pt

    @staticmethod
    def linear_transform(ct: Ciphertext, diag_plaintexts: Plaintext, keyset: RnsGadgetKeySet) -> Ciphertext:
        """``sum_k diag_k * rotate(ct, k)`` over the key set's steps as one
        library call; the scales multiply, so logp grows by the diagonals'."""
        out = linear_transform(ct, diag_plaintexts.poly, keyset)
        out.logp = ct.logp + diag_plaintexts.scale_bits
        return out

    def encode_diagonals_bsgs(self, matrix, baby_steps, giant_steps, encoder: CkksEncoder) -> Plaintext:
        """The n2 n1 plaintexts of a slots x slots matrix for
        ``linear_transform_bsgs`` (``bsgs_diagonal_rows``: diagonal
        ``g_j + b_i`` rotated back by ``g_j``), encoded as one batch, poly
        ``j n1 + i`` for (giant j, baby i), and moved to the NTT domain."""
        m = np.asarray(matrix)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] != encoder.max_slots():
            raise ValueError("encode_diagonals_bsgs: the matrix must be slots x slots with slots = N / 2")
        rows = bsgs_diagonal_rows(m, baby_steps, giant_steps)
        pt = encoder.encode_complex(rows.reshape(-1, rows.shape[-1]), self.basis)
        pt.poly.to_ntt_domain()
        return pt

    @staticmethod
    def linear_transform_bsgs(ct: Ciphertext, diag_plaintexts: Plaintext, baby_keyset: RnsGadgetKeySet,
                              giant_keyset: RnsGadgetKeySet) -> Ciphertext:
        """``sum_j rotate(sum_i diag_ji * rotate(ct, b_i), g_j)`` over the two
        key sets' steps as one library call: n1 + n2 key-switches for n1 n2
        diagonals; logp grows by the diagonals' scale."""
        out = linear_transform_bsgs(ct, diag_plaintexts.poly, baby_keyset, giant_keyset)
        out.logp = ct.logp + diag_plaintexts.scale_bits
        return out

    @staticmethod
    def linear_transform_bsgs_hoisted(ct: Ciphertext, diag_plaintexts: Plaintext, baby_keyset: RnsGadgetKeySet,
                                      giant_keyset: RnsGadgetKeySet) -> Ciphertext:
        """``linear_transform_bsgs`` with hoisted baby rotations (baby keys
        in hoisting form, giant keys ordinary): one decomposition for all the
        babies; logp grows by the diagonals' scale."""
        out = linear_transform_bsgs_hoisted(ct, diag_plaintexts.poly, baby_keyset, giant_keyset)
        out.logp = ct.logp + diag_plaintexts.scale_bits
        return out

    @staticmethod
    def secret_on(sk: RnsPoly, basis: RnsBasis) -> RnsPoly:
        """The secret key restricted to a prefix basis (after rescale), built
        on that basis object (same basis = same context, as Arc::ptr_eq)."""
        ch = sk.channels()
        return RnsPoly.from_channels(ch[: basis.channel_count()], basis)
