"""Host-side mirror of oiwn/toy-heaan-ckks's RNS-NTT ring interface over the
MI355X C-ABI (include/rnsntt.h).

Names, argument meaning and error behaviour follow the reference:

* :class:`RnsBasis`  -- ``RnsBasis<N>`` (src/rings/backends/rns_ntt/basis.rs:90-180)
* :class:`RnsPoly`   -- ``RnsPoly<N>`` (src/rings/backends/rns_ntt/poly.rs:25-570);
  one object holds a *batch* of ``n_polys`` polynomials that every op
  processes together (``n_polys=1`` is the reference's single polynomial).
* :func:`mul_ciphertexts_gadget`, :func:`rotate_ciphertext`,
  :func:`rescale_ciphertext` -- ``CkksEngine`` (src/crypto/engine.rs:263-539).
* :class:`RnsNttError` -- ``RnsNttError`` (errors.rs:4-20), raised with the
  same variant name.

All arithmetic runs in librnsntt.so on the GPU.  Host code here only moves
data across the boundary (``from_channels`` / ``channels``) and does the
reference's decode-side u128 CRT in :meth:`RnsPoly.to_coeffs`.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import RnsNttError, check, load
from .homdft import HomDftPlan, homdft_plan
from .poly_eval import PolyEvalPlan, poly_eval_plan, poly_eval_plan_fused
from .evalmod import EvalModPlan, evalmod_plan
from .rotsum import RotsumPlan, rotsum_plan

__all__ = [
    "device_count",
    "RnsNttError",
    "RnsBasis",
    "RnsPoly",
    "RnsGadgetKey",
    "RnsHybridKey",
    "keyswitch_hybrid",
    "rotate_ciphertext_hybrid",
    "mul_ciphertexts_hybrid",
    "RnsHybridKeySet",
    "rotate_ciphertext_hybrid_hoisted",
    "rotsum_ciphertext_hybrid",
    "automorphism_ntt",
    "rotsum_plan",
    "RotsumPlan",
    "linear_transform_hybrid",
    "linear_transform_bsgs_hybrid",
    "mul_ciphertexts_hybrid_rescale",
    "mul_ciphertexts_hybrid_rescale_affine",
    "evalmod_plan",
    "EvalModPlan",
    "linear_transform_bsgs_hybrid_rescale",
    "linear_bsgs_hybrid_dh",
    "hybrid_level_moduli",
    "dot_ciphertexts_hybrid",
    "conjugate_hybrid",
    "mul_i",
    "split_real_imag_hybrid",
    "merge_real_imag",
    "homdft_plan",
    "HomDftPlan",
    "Ciphertext",
    "generate_primes",
    "is_ntt_friendly_prime",
    "find_psi",
    "keyswitch",
    "mul_ciphertexts_gadget",
    "mul_ciphertexts_gadget_rescale",
    "rotate_ciphertext",
    "RnsGadgetKeySet",
    "linear_transform",
    "linear_transform_bsgs",
    "linear_transform_bsgs_hoisted",
    "rotate_ciphertext_hoisted",
    "bsgs_diagonal_rows",
    "rescale_ciphertext",
    "ct_lincomb",
    "ct_plain_mac",
    "mul_plain",
    "poly_eval_plan",
    "poly_eval_plan_fused",
    "PolyEvalPlan",
    "Plaintext",
    "CkksEncoder",
    "DeviceRng",
    "pool_trim",
    "Graph",
]


def _u64p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _i64p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


# ---------------------------------------------------------------------------
# host-side number theory (setup)
# ---------------------------------------------------------------------------


def device_count() -> int:
    """Visible HIP devices (0 on a CPU-only host)."""
    r = ctypes.c_int(0)
    check(load().rnt_device_count(ctypes.byref(r)))
    return int(r.value)


def pool_trim(device: int = -1) -> int:
    """Release the device block cache's idle blocks (of one device, or all
    with -1) back to HIP; returns the bytes released.  Call it when another
    allocator (torch's) runs out of memory before retrying."""
    freed = ctypes.c_size_t(0)
    check(load().rnt_pool_trim(int(device), ctypes.byref(freed)))
    return int(freed.value)


def generate_primes(bit_size: int, count: int, degree: int) -> list[int]:
    """src/math/utils.rs:47-80."""
    out = np.zeros(max(count, 1), dtype=np.uint64)
    check(load().rnt_generate_primes(bit_size, count, degree, _u64p(out)))
    return [int(x) for x in out[:count]]


def is_ntt_friendly_prime(p: int, n: int) -> bool:
    """src/math/primes.rs:125-131."""
    r = ctypes.c_int(0)
    check(load().rnt_is_ntt_friendly_prime(p, n, ctypes.byref(r)))
    return bool(r.value)


def find_psi(modulus: int, degree: int) -> int:
    """psi of NttTable::new (basis.rs:39-40, 217-237)."""
    r = ctypes.c_uint64(0)
    check(load().rnt_find_psi(modulus, degree, ctypes.byref(r)))
    return int(r.value)


class DeviceRng:
    """The seeded generator passed where the reference passes ``&mut rng``
    to a PolySampler (traits.rs:74-127).  Every sampler call takes the next
    stream of the device's counter-based Philox4x32-10 generator
    (rnt_sample_*), so a seed fixes every later sample, as a seeded
    ChaCha20Rng does in the reference (whose streams are not reproduced)."""

    def __init__(self, seed: int):
        self.seed = int(seed) & ((1 << 64) - 1)
        self.stream = 0

    def next_stream(self) -> int:
        s = self.stream
        self.stream += 1
        return s


# ---------------------------------------------------------------------------
# RnsBasis
# ---------------------------------------------------------------------------


class RnsBasis:
    """``Arc<RnsBasis<N>>``: an immutable RNS basis with device NTT tables.

    ``RnsBasis(moduli, degree)`` validates like ``RnsBasis::new``
    (basis.rs:97-106): ``EmptyBasis`` for no moduli, ``InvalidDegree`` for a
    non power-of-two degree, ``NonNttFriendlyModulus`` otherwise; a valid
    degree above 2^17 raises ``Unsupported`` (this backend's capacity).
    """

    def __init__(self, moduli: Sequence[int], degree: int, device: int = 0):
        lib = load()
        # basis.rs:97-106 order: EmptyBasis first (rnt_ctx_create checks it),
        # then per modulus NttTable::new's InvalidDegree (basis.rs:22-24: not a
        # power of two) and NonNttFriendlyModulus.  A power-of-two degree
        # above this backend's 2^17 is Unsupported (status 12), never
        # InvalidDegree.
        if len(moduli) and (degree <= 0 or degree & (degree - 1)):
            raise RnsNttError(_lib.INVALID_DEGREE, f"ring degree must be a power of two, got {degree}",
                              {"degree": degree})
        log_n = degree.bit_length() - 1 if degree > 0 and not degree & (degree - 1) else 0
        arr = np.ascontiguousarray(np.array(list(moduli), dtype=np.uint64)) if len(moduli) else np.zeros(1, np.uint64)
        h = ctypes.c_void_p()
        check(lib.rnt_ctx_create(log_n, _u64p(arr), len(moduli), device, ctypes.byref(h)))
        self._h = h
        self._parent = None
        self.degree = degree
        self.device = device

    @classmethod
    def _from_handle(cls, h, parent: "RnsBasis") -> "RnsBasis":
        self = cls.__new__(cls)
        self._h = h
        self._parent = parent  # keeps the shared tables' owner reachable
        self.degree = parent.degree
        self.device = parent.device
        return self

    @property
    def handle(self):
        return self._h

    def moduli(self) -> list[int]:
        out = np.zeros(self.channel_count(), dtype=np.uint64)
        check(load().rnt_ctx_moduli(self._h, _u64p(out)))
        return [int(x) for x in out]

    def channel_count(self) -> int:
        r = ctypes.c_size_t(0)
        check(load().rnt_ctx_channel_count(self._h, ctypes.byref(r)))
        return int(r.value)

    def drop_last(self, drop_count: int) -> "RnsBasis":
        """basis.rs:121-134 (a view sharing the device tables)."""
        h = ctypes.c_void_p()
        check(load().rnt_ctx_drop_last(self._h, drop_count, ctypes.byref(h)))
        return RnsBasis._from_handle(h, self)

    def hybrid_level(self, n_special: int, level: int) -> "RnsBasis":
        """The level basis ``q_0..q_{level-1}, p_0..p_{K-1}`` of this hybrid
        key basis (its last ``K = n_special`` limbs the special primes), on
        this basis' own tables (rnt_ctx_hybrid_level).  It holds key level
        views alone (:meth:`RnsHybridKey.at_level`).  One object per
        ``(n_special, level)``: the hybrid calls compare the handles of the
        key halves and sets, so every key at a level must share it."""
        cache = self.__dict__.setdefault("_levels", {})
        at = (int(n_special), int(level))
        if at not in cache:
            h = ctypes.c_void_p()
            check(load().rnt_ctx_hybrid_level(self._h, at[0], at[1], ctypes.byref(h)))
            cache[at] = RnsBasis._from_handle(h, self)
        return cache[at]

    def total_bits(self) -> int:
        r = ctypes.c_uint32(0)
        check(load().rnt_ctx_total_bits(self._h, ctypes.byref(r)))
        return int(r.value)

    def psi(self, limb: int) -> int:
        r = ctypes.c_uint64(0)
        check(load().rnt_ctx_psi(self._h, limb, ctypes.byref(r)))
        return int(r.value)

    def stream(self) -> int:
        r = ctypes.c_void_p()
        check(load().rnt_ctx_stream(self._h, ctypes.byref(r)))
        return int(r.value or 0)

    def set_stream(self, stream=None) -> None:
        """Queue later ops on ``stream`` (a raw hipStream_t address or a
        ``torch.cuda.Stream``; None: the basis' own stream), after everything
        queued so far.  Shared with every drop_last view of this basis."""
        if stream is not None and not isinstance(stream, int):
            stream = int(stream.cuda_stream)
        check(load().rnt_ctx_set_stream(self._h, ctypes.c_void_p(stream or None)))

    def sync(self) -> None:
        check(load().rnt_sync(self._h))

    def capture(self) -> "Graph":
        """Record the device ops this thread queues on the basis' stream
        inside ``with basis.capture() as g:`` into a HIP graph instead of
        running them; ``g.replay()`` then re-runs the whole sequence (same
        buffers) as one launch (rnt_capture_begin / rnt_graph_launch).  Run
        the sequence once before recording it, so its workspaces are cached;
        only device ops may be recorded (no from_channels / channels / sync)."""
        return Graph(self)

    def profile_enable(self, enable: bool = True) -> None:
        """Bracket every kernel launched on this basis' stream with HIP events."""
        check(load().rnt_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self, kernel: str) -> tuple[int, float]:
        """(launches, summed device ms) for one kernel since profile_enable."""
        n = ctypes.c_uint64(0)
        ms = ctypes.c_double(0)
        check(load().rnt_profile_read(self._h, kernel.encode(), ctypes.byref(n), ctypes.byref(ms)))
        return int(n.value), float(ms.value)

    def reconstruct_centered_coeff(self, residues: Sequence[int]) -> int:
        """basis.rs:158-180 (host-side decode; the reference needs Q < 2^128)."""
        mods = self.moduli()
        Q = 1
        for m in mods:
            Q *= m
        if Q >= 1 << 128:
            raise OverflowError("reconstruct_centered_coeff requires Q < 2^128 (basis.rs:152-157)")
        acc = 0
        for r, m in zip(residues, mods):
            qi = Q // m
            acc = (acc + (int(r) * pow(qi % m, -1, m) % m) * qi) % Q
        return acc - Q if acc > Q // 2 else acc

    def __del__(self, _lib=_lib):  # module globals may be gone at interpreter exit
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None and _lib._lib is not None:
            _lib._lib.rnt_ctx_destroy(h)
            self._h = None


class Graph:
    """A recorded op sequence (see RnsBasis.capture)."""

    def __init__(self, basis: "RnsBasis"):
        self.basis = basis
        self._h = None

    def __enter__(self) -> "Graph":
        check(load().rnt_capture_begin(self.basis.handle))
        return self

    def __exit__(self, exc_type, exc, tb) -> None:
        h = ctypes.c_void_p()
        rc = load().rnt_capture_end(self.basis.handle, ctypes.byref(h))
        if exc_type is None:
            check(rc)
            self._h = h
        elif rc == 0 and h.value:
            # the body raised: the graph (and the workspace it holds) is never replayed
            load().rnt_graph_destroy(h)

    def workspace(self) -> tuple[int, int]:
        """(blocks, bytes) of device workspace the recorded graph holds."""
        if self._h is None:
            raise RuntimeError("graph was not recorded")
        blocks, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
        check(load().rnt_graph_workspace(self._h, ctypes.byref(blocks), ctypes.byref(nbytes)))
        return int(blocks.value), int(nbytes.value)

    def replay(self) -> None:
        if self._h is None:
            raise RuntimeError("graph was not recorded")
        check(load().rnt_graph_launch(self._h))

    def __del__(self, _lib=_lib):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None and _lib._lib is not None:
            _lib._lib.rnt_graph_destroy(h)
            self._h = None


# ---------------------------------------------------------------------------
# RnsPoly
# ---------------------------------------------------------------------------


class RnsPoly:
    """A batch of ``n_polys`` polynomials in Z_{q_0} x ... x Z_{q_{L-1}}[X]/(X^N+1).

    Mirrors ``RnsPoly<N>`` (poly.rs:25-570).  Operators follow the Rust ones:
    ``a *= b`` (MulAssign), ``a += b`` (AddAssign), ``-a`` (Neg).

    An object is either the reference's single polynomial (built without a
    batch count: ``RnsPoly(basis)``, ``from_channels([L][N])``,
    ``from_coeffs([N])``, ``sample_*(...)`` without ``n_polys``) or a batch
    (``RnsPoly(basis, B)``, ``from_channels([B][L][N])`` ...), and every
    result of an op is of the same kind as its input.  Host views follow the
    kind, never the batch size: ``channels()`` is [L][N] for a single
    polynomial and [B][L][N] for a batch (also when B == 1);
    ``channels_batch()`` is always [B][L][N].
    """

    def __init__(self, basis: RnsBasis, n_polys: Optional[int] = None, _uninit: bool = False):
        lib = load()
        h = ctypes.c_void_p()
        count = 1 if n_polys is None else int(n_polys)
        alloc = lib.rnt_buf_alloc_uninit if _uninit else lib.rnt_buf_alloc
        check(alloc(basis.handle, count, ctypes.byref(h)))
        self._h = h
        self.basis = basis
        self.n_polys = count
        self.batched = n_polys is not None

    def _like(self, basis: Optional[RnsBasis] = None) -> "RnsPoly":
        """An op output of this object's kind and batch on ``basis``: its
        contents are unspecified until the op (which writes every word)
        fills it, so no zero fill is queued (rnt_buf_alloc_uninit)."""
        return RnsPoly(basis or self.basis, self.n_polys if self.batched else None, _uninit=True)

    @classmethod
    def _key_level_view(cls, key_polys: "RnsPoly", level_basis: RnsBasis, alpha: int) -> "RnsPoly":
        """A read-only view of a prepared hybrid key's (or key set's) polys at
        the level of ``level_basis`` (rnt_key_level_view): no copy; it keeps
        ``key_polys`` alive and serves as a hybrid key argument alone."""
        h = ctypes.c_void_p()
        check(load().rnt_key_level_view(key_polys.handle, level_basis.handle, int(alpha), ctypes.byref(h)))
        self = cls.__new__(cls)
        self._h = h
        self.basis = level_basis
        self._view_of = key_polys
        n = ctypes.c_size_t(0)
        check(load().rnt_buf_n_polys(h, ctypes.byref(n)))
        self.n_polys = int(n.value)
        self.batched = True
        return self

    # -- constructors (poly.rs:34-114) --------------------------------------
    @classmethod
    def zero(cls, basis: RnsBasis, n_polys: Optional[int] = None) -> "RnsPoly":
        return cls(basis, n_polys)

    @classmethod
    def from_coeffs(cls, coeffs, basis: RnsBasis) -> "RnsPoly":
        """poly.rs:49-67; ``coeffs`` is [N] or [B][N] signed integers."""
        c = np.asarray(coeffs, dtype=np.int64)
        single = c.ndim == 1
        if single:
            c = c[None, :]
        if c.shape[1] < basis.degree:
            raise ValueError(f"from_coeffs: need at least {basis.degree} coefficients, got {c.shape[1]}")
        c = np.ascontiguousarray(c[:, : basis.degree])
        p = cls(basis, None if single else c.shape[0])
        check(load().rnt_upload_coeffs(p._h, _i64p(c), c.shape[0]))
        return p

    @classmethod
    def from_channels(cls, channels, basis: RnsBasis, in_ntt_domain: bool = False) -> "RnsPoly":
        """poly.rs:73-99; ``channels`` is [L][N] or [B][L][N] residues.

        Raises ChannelCountMismatch / NonReducedCoefficient like the reference.
        """
        ch = np.asarray(channels, dtype=np.uint64)
        single = ch.ndim == 2
        if single:
            ch = ch[None, :, :]
        if ch.ndim != 3 or ch.shape[2] != basis.degree:
            raise ValueError("from_channels: expected [L][N] or [B][L][N] with N == degree")
        ch = np.ascontiguousarray(ch)
        p = cls(basis, None if single else ch.shape[0])
        check(load().rnt_upload(p._h, _u64p(ch), ch.shape[0], ch.shape[1], 1 if in_ntt_domain else 0))
        return p

    @classmethod
    def wrap(cls, basis: RnsBasis, device_ptr: int, n_polys: int, in_ntt_domain: bool = False,
             owner=None) -> "RnsPoly":
        """A non-owning view of caller device memory laid out [L][n_polys][N]
        in the basis' device word width (``word_bytes``); ``owner`` (e.g. the
        torch tensor holding the memory) is kept alive with the view.  Used
        by the limb-sharded pipeline to hand buffers to RCCL collectives."""
        p = cls.__new__(cls)
        h = ctypes.c_void_p()
        check(load().rnt_buf_wrap(basis.handle, ctypes.c_void_p(device_ptr), n_polys,
                                  1 if in_ntt_domain else 0, ctypes.byref(h)))
        p._h = h
        p.basis = basis
        p.n_polys = n_polys
        p.batched = True
        p._owner = owner
        return p

    # -- PolySampler (traits.rs:74-127; poly.rs:438-477), on the device -----
    @classmethod
    def sample_uniform(cls, basis: RnsBasis, rng: DeviceRng, n_polys: Optional[int] = None) -> "RnsPoly":
        p = cls(basis, n_polys)
        check(load().rnt_sample_uniform(p._h, rng.seed, rng.next_stream()))
        return p

    @classmethod
    def sample_gaussian(cls, std_dev: float, basis: RnsBasis, rng: DeviceRng, n_polys: Optional[int] = None) -> "RnsPoly":
        p = cls(basis, n_polys)
        check(load().rnt_sample_gaussian(p._h, float(std_dev), rng.seed, rng.next_stream()))
        return p

    @classmethod
    def sample_tribits(cls, hamming_weight: int, basis: RnsBasis, rng: DeviceRng, n_polys: Optional[int] = None) -> "RnsPoly":
        p = cls(basis, n_polys)
        check(load().rnt_sample_ternary(p._h, int(hamming_weight), rng.seed, rng.next_stream()))
        return p

    @classmethod
    def sample_noise(cls, variance: float, basis: RnsBasis, rng: DeviceRng, n_polys: Optional[int] = None) -> "RnsPoly":
        """poly.rs:471-477: Gaussian with std_dev = sqrt(variance)."""
        return cls.sample_gaussian(float(np.sqrt(variance)), basis, rng, n_polys)

    def device_ptr(self) -> tuple[int, int]:
        """(device address of the [L][B][N] storage, word bytes)."""
        ptr = ctypes.c_void_p()
        wb = ctypes.c_size_t()
        check(load().rnt_buf_device_ptr(self._h, ctypes.byref(ptr), ctypes.byref(wb)))
        return int(ptr.value or 0), int(wb.value)

    # -- accessors (poly.rs:118-129) ----------------------------------------
    @property
    def handle(self):
        return self._h

    def channels(self) -> np.ndarray:
        """poly.rs:119-121: [L][N] for a single polynomial, [B][L][N] for a
        batch object (whatever its size; see the class docstring)."""
        out = self.channels_batch()
        return out if self.batched else out[0]

    def channels_batch(self) -> np.ndarray:
        """[B][L][N] always (B = 1 for a single polynomial)."""
        out = np.zeros((self.n_polys, self.basis.channel_count(), self.basis.degree), dtype=np.uint64)
        check(load().rnt_download(self._h, _u64p(out), self.n_polys))
        return out

    def channels_of(self, first: int, count: int = 1) -> np.ndarray:
        """[count][L][N]: channels of polys first .. first+count-1 of the batch."""
        out = np.zeros((count, self.basis.channel_count(), self.basis.degree), dtype=np.uint64)
        check(load().rnt_download_polys(self._h, _u64p(out), int(first), int(count)))
        return out

    def is_ntt_domain(self) -> bool:
        r = ctypes.c_int(0)
        check(load().rnt_buf_is_ntt(self._h, ctypes.byref(r)))
        return bool(r.value)

    def clone(self) -> "RnsPoly":
        p = self._like()
        check(load().rnt_copy(p._h, self._h))
        return p

    def copy_polys(self, src: "RnsPoly", dst_first: int = 0, src_first: int = 0,
                   count: Optional[int] = None) -> "RnsPoly":
        """Polys ``src_first .. src_first+count-1`` of ``src`` into this batch
        from ``dst_first`` on, device to device (rnt_copy_polys); ``count``
        defaults to the rest of ``src``."""
        n = src.n_polys - int(src_first) if count is None else int(count)
        check(load().rnt_copy_polys(self._h, int(dst_first), src._h, int(src_first), n))
        return self

    # -- domain conversion (poly.rs:136-166) --------------------------------
    def to_ntt_domain(self) -> None:
        check(load().rnt_ntt_fwd(self._h))

    def to_coeff_domain(self) -> None:
        check(load().rnt_ntt_inv(self._h))

    # -- arithmetic (poly.rs:254-385) ---------------------------------------
    def __imul__(self, rhs: "RnsPoly") -> "RnsPoly":
        check(load().rnt_mul(self._h, self._h, rhs._h))
        return self

    def __iadd__(self, rhs: "RnsPoly") -> "RnsPoly":
        check(load().rnt_add(self._h, self._h, rhs._h))
        return self

    def __isub__(self, rhs: "RnsPoly") -> "RnsPoly":
        check(load().rnt_sub(self._h, self._h, rhs._h))
        return self

    def __mul__(self, rhs: "RnsPoly") -> "RnsPoly":
        out = self._like()
        check(load().rnt_mul(out._h, self._h, rhs._h))
        return out

    def __add__(self, rhs: "RnsPoly") -> "RnsPoly":
        out = self._like()
        check(load().rnt_add(out._h, self._h, rhs._h))
        return out

    def __sub__(self, rhs: "RnsPoly") -> "RnsPoly":
        out = self._like()
        check(load().rnt_sub(out._h, self._h, rhs._h))
        return out

    def __neg__(self) -> "RnsPoly":
        out = self._like()
        check(load().rnt_neg(out._h, self._h))
        return out

    # -- rescale / mod-drop (poly.rs:168-249) -------------------------------
    def rescale_into(self, new_basis: RnsBasis) -> "RnsPoly":
        out = self._like(new_basis)
        check(load().rnt_rescale(out._h, self._h))
        return out

    def rescale(self) -> "RnsPoly":
        if self.basis.channel_count() < 2:
            raise RnsNttError(_lib.INVALID_MOD_DROP,
                              f"invalid mod-drop count 1 for {self.basis.channel_count()} channels",
                              {"drop_count": 1, "channel_count": self.basis.channel_count()})
        return self.rescale_into(self.basis.drop_last(1))

    def mod_drop_last(self, drop_count: int) -> "RnsPoly":
        nb = self.basis.drop_last(drop_count)
        out = self._like(nb)
        check(load().rnt_mod_drop_last(out._h, self._h))
        return out

    def mod_raise(self, basis: RnsBasis) -> "RnsPoly":
        """ModRaise (rnt_mod_raise): this polynomial, on 1..4 limbs in the
        coefficient domain, as the same centred integers on ``basis`` -- a
        longer basis whose first moduli are this one's, by value."""
        out = self._like(basis)
        check(load().rnt_mod_raise(out._h, self._h))
        return out

    def mul_monomial(self, k: int) -> "RnsPoly":
        """``self * X^k`` in Z_q[X]/(X^N + 1) (rnt_mul_monomial), k mod 2N:
        an exact negacyclic shift; coefficient domain."""
        out = self._like()
        check(load().rnt_mul_monomial(out._h, self._h, int(k)))
        return out

    # -- automorphisms (poly.rs:482-570) ------------------------------------
    def automorphism(self, exponent: int) -> "RnsPoly":
        out = self._like()
        check(load().rnt_automorphism(out._h, self._h, exponent))
        return out

    def rotate_slots(self, k: int) -> "RnsPoly":
        out = self._like()
        check(load().rnt_rotate_slots(out._h, self._h, k))
        return out

    def automorphism_ntt(self, exponent: int, out: Optional["RnsPoly"] = None) -> "RnsPoly":
        """:func:`automorphism_ntt` of this NTT-domain polynomial."""
        return automorphism_ntt(self, exponent, out)

    # -- PolyRing::to_coeffs (poly.rs:404-427) ------------------------------
    def to_coeffs(self) -> np.ndarray:
        """PolyRing::to_coeffs (poly.rs:404-427): the centred CRT value of each
        coefficient as i64 (its low 64 bits, like the reference), computed on
        the device (rnt_to_coeffs)."""
        out = np.zeros((self.n_polys, self.basis.degree), dtype=np.int64)
        check(load().rnt_to_coeffs(self._h, out.ctypes.data_as(ctypes.c_void_p), self.n_polys))
        return out if self.batched else out[0]

    def to_coeffs_exact(self) -> list:
        """The centred CRT values as Python ints for any Q (rnt_crt_centered):
        [N] for a single polynomial, [B][N] nested lists for a batch object."""
        bits = sum(int(q).bit_length() for q in self.basis.moduli())
        words = max(1, (bits + 1 + 63) // 64)
        raw = np.zeros((self.n_polys, self.basis.degree, words), dtype=np.uint64)
        check(load().rnt_crt_centered(self._h, raw.ctypes.data_as(ctypes.c_void_p), self.n_polys, words))
        out = []
        for b in range(self.n_polys):
            row = []
            for i in range(self.basis.degree):
                v = 0
                for w in range(words - 1, -1, -1):
                    v = (v << 64) | int(raw[b, i, w])
                if v >> (64 * words - 1):  # two's complement sign
                    v -= 1 << (64 * words)
                row.append(v)
            out.append(row)
        return out if self.batched else out[0]

    def __del__(self, _lib=_lib):  # module globals may be gone at interpreter exit
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None and _lib._lib is not None:
            _lib._lib.rnt_buf_free(h)
            self._h = None


# ---------------------------------------------------------------------------
# engine-level ops (src/crypto/engine.rs)
# ---------------------------------------------------------------------------


class RnsGadgetKey:
    """RnsGadgetRelinKey / RnsGadgetRotationKey (engine.rs:224-253).

    ``a`` and ``b`` are RnsPoly batches holding the L key polynomials; they
    are made NTT-resident once by :meth:`prepare`.  ``hoisted`` says which
    form the key is in: the ordinary prepared one, or (after
    :meth:`prepare_hoisted`) the hoisting form of the hoisted rotations.
    """

    def __init__(self, a: RnsPoly, b: RnsPoly, rotation: Optional[int] = None):
        self.a = a
        self.b = b
        self.rotation = rotation
        self.hoisted = False
        check(load().rnt_key_prepare(a.handle, b.handle))

    def prepare_hoisted(self) -> "RnsGadgetKey":
        """Turn this rotation key into its hoisting form
        ``NTT(sigma_k^-1(key))``, k the key's ``rotation``
        (rnt_key_prepare_hoisted), in place.  The ordinary form is gone: a
        caller that needs both keeps a second key."""
        if self.rotation is None:
            raise ValueError("prepare_hoisted: not a rotation key (no rotation step)")
        if self.hoisted:
            raise ValueError("prepare_hoisted: the key is in hoisting form already")
        check(load().rnt_key_prepare_hoisted(self.a.handle, self.b.handle, int(self.rotation)))
        self.hoisted = True
        return self

    @classmethod
    def from_channels(cls, a_channels, b_channels, basis: RnsBasis, rotation: Optional[int] = None):
        """a_channels / b_channels: [L][L][N] coefficient-domain residues."""
        return cls(RnsPoly.from_channels(a_channels, basis), RnsPoly.from_channels(b_channels, basis), rotation)


@dataclass
class Ciphertext:
    """types.rs:27-35."""

    c0: RnsPoly
    c1: RnsPoly
    logp: int = 0
    logq: int = 0


def _require_class(key, cls, what: str) -> None:
    """``key`` must be of the class the call reads (RnsGadgetKey for the
    gadget calls, RnsHybridKey for the hybrid ones): the library sees only
    buffers and would at best report a poly count."""
    if not isinstance(key, cls):
        raise TypeError(f"{what}: needs an {cls.__name__}, got {type(key).__name__}")


def keyswitch(d: RnsPoly, key: RnsGadgetKey) -> tuple[RnsPoly, RnsPoly]:
    """Gadget sum (engine.rs:505-528 / 429-452) on a coefficient-domain batch."""
    _require_class(key, RnsGadgetKey, "keyswitch")
    acc0, acc1 = d._like(), d._like()
    check(load().rnt_keyswitch(acc0.handle, acc1.handle, d.handle, key.a.handle, key.b.handle))
    return acc0, acc1


def mul_ciphertexts_gadget(ct1: Ciphertext, ct2: Ciphertext, rlk: RnsGadgetKey) -> Ciphertext:
    """engine.rs:473-539."""
    _require_class(rlk, RnsGadgetKey, "mul_ciphertexts_gadget")
    assert ct1.logq == ct2.logq, "logq mismatch in gadget multiplication"
    basis = ct1.c0.basis
    out0, out1 = ct1.c0._like(basis), ct1.c0._like(basis)
    check(load().rnt_ct_mul_relin(out0.handle, out1.handle, ct1.c0.handle, ct1.c1.handle,
                                  ct2.c0.handle, ct2.c1.handle, rlk.a.handle, rlk.b.handle))
    return Ciphertext(out0, out1, ct1.logp + ct2.logp, ct1.logq)


def _require_form(keys, hoisted: bool, what: str) -> None:
    """``keys`` (an RnsGadgetKey or RnsGadgetKeySet) must be in the form the
    call reads: the library cannot tell the two apart and would compute a
    wrong result from the wrong one."""
    if bool(getattr(keys, "hoisted", False)) != hoisted:
        raise ValueError(f"{what}: needs {'hoisting-form' if hoisted else 'ordinary prepared'} keys, got "
                         f"{'ordinary prepared' if hoisted else 'hoisting-form'} ones")


def rotate_ciphertext(ct: Ciphertext, rotk: RnsGadgetKey) -> Ciphertext:
    """engine.rs:412-463."""
    _require_class(rotk, RnsGadgetKey, "rotate_ciphertext")
    _require_form(rotk, False, "rotate_ciphertext")
    basis = ct.c0.basis
    out0, out1 = ct.c0._like(basis), ct.c0._like(basis)
    check(load().rnt_ct_rotate(out0.handle, out1.handle, ct.c0.handle, ct.c1.handle,
                               int(rotk.rotation or 0), rotk.a.handle, rotk.b.handle))
    return Ciphertext(out0, out1, ct.logp, ct.logq)


class RnsHybridKey:
    """A hybrid (special-prime) relinearisation or rotation key: ``a`` and
    ``b`` are RnsPoly batches of ``beta = ceil(L / alpha)`` polys on the
    EXTENDED basis ``q_0..q_{L-1}, p_0..p_{K-1}``, made NTT-resident here
    (rnt_key_prepare).  ``alpha`` is the digit size the key was generated
    for and ``rotation`` the step of a rotation key.  ``hoisted`` says which
    form the key is in: the ordinary prepared one, or (after
    :meth:`prepare_hoisted`) the hoisting form of the hoisted hybrid
    rotations."""

    def __init__(self, a: RnsPoly, b: RnsPoly, alpha: int, rotation: Optional[int] = None,
                 n_special: Optional[int] = None):
        if int(alpha) < 1:
            raise ValueError("RnsHybridKey: alpha must be at least 1")
        if a.basis is not b.basis and a.basis.moduli() != b.basis.moduli():
            raise ValueError("RnsHybridKey: the key halves are on different bases")
        if n_special is not None and not 1 <= int(n_special) < a.basis.channel_count():
            raise ValueError("RnsHybridKey: n_special must be at least 1 and below the basis' limb count")
        self.a = a
        self.b = b
        self.alpha = int(alpha)
        self.rotation = rotation
        self.hoisted = False
        # the count K of special primes (the basis' last limbs): with it the
        # hybrid wrappers pick the key's view at a lower-level ciphertext's
        # level by themselves (at_level); None: the caller restricts, as before
        self.n_special = None if n_special is None else int(n_special)
        self.level = None  # a view's level (at_level)
        self._views = {}
        check(load().rnt_key_prepare(a.handle, b.handle))

    def at_level(self, level: int, n_special: Optional[int] = None) -> "RnsHybridKey":
        """This key at a lower level, as a VIEW of its device planes
        (rnt_key_level_view): the key of ``q_0..q_{level-1}`` and the special
        primes, with no copy and no host trip; it keeps ``alpha``, ``rotation``
        and ``hoisted`` and holds this key alive.  Cached per level; every key
        of one extended basis shares the level's basis object
        (:meth:`RnsBasis.hybrid_level`).  ``n_special`` defaults to the
        key's."""
        if self.level is not None:
            raise ValueError("at_level: the key is a level view already")
        ns = self.n_special if n_special is None else int(n_special)
        if ns is None:
            raise ValueError("at_level: the key carries no n_special; pass it")
        at = (ns, int(level))
        if at not in self._views:
            lb = self.a.basis.hybrid_level(ns, int(level))
            if self.b.basis is not self.a.basis:
                raise ValueError("at_level: the key halves must share one basis object")
            v = RnsHybridKey.__new__(RnsHybridKey)
            v.a = RnsPoly._key_level_view(self.a, lb, self.alpha)
            v.b = RnsPoly._key_level_view(self.b, lb, self.alpha)
            v.alpha, v.rotation, v.hoisted, v.n_special = self.alpha, self.rotation, self.hoisted, ns
            v.level = int(level)
            v._views = {}
            v._parent = self
            self._views[at] = v
        return self._views[at]

    def prepare_hoisted(self) -> "RnsHybridKey":
        """Turn this rotation key into its hoisting form
        ``NTT(sigma_k^-1(key))`` over the extended basis, k the key's
        ``rotation`` (rnt_key_prepare_hoisted), in place.  The ordinary form
        is gone: a caller that needs both keeps a second key."""
        if self.rotation is None:
            raise ValueError("prepare_hoisted: not a rotation key (no rotation step)")
        if self.hoisted:
            raise ValueError("prepare_hoisted: the key is in hoisting form already")
        check(load().rnt_key_prepare_hoisted(self.a.handle, self.b.handle, int(self.rotation)))
        self.hoisted = True
        self._views = {}  # (views made before read the new words but carry the old form)
        return self

    @classmethod
    def from_channels(cls, a_channels, b_channels, ext_basis: RnsBasis, alpha: int,
                      rotation: Optional[int] = None, n_special: Optional[int] = None) -> "RnsHybridKey":
        """a_channels / b_channels: [beta][L + K][N] coefficient-domain residues."""
        return cls(RnsPoly.from_channels(np.asarray(a_channels, dtype=np.uint64), ext_basis),
                   RnsPoly.from_channels(np.asarray(b_channels, dtype=np.uint64), ext_basis), alpha, rotation,
                   n_special)

    def restrict(self, ext_basis_lv: RnsBasis) -> "RnsHybridKey":
        """The key of a lower level: ``ext_basis_lv`` is a root basis over
        ``q_0..q_{L'-1}, p_0..p_{K-1}``; the result holds the first
        ``ceil(L'/alpha)`` polys on the kept limbs (the digit boundaries do not
        move).  Set-up: the polys make one host round trip, in the NTT domain
        (a limb's transform does not depend on the others; the hoisting form
        is computed per limb too, so the result keeps the key's form)."""
        full = self.a.basis.moduli()
        low = ext_basis_lv.moduli()
        lv = 0
        while lv < min(len(full), len(low)) and full[lv] == low[lv]:
            lv += 1
        if lv == len(full) == len(low):
            keep, n_polys = list(range(len(full))), self.a.n_polys
        else:
            k = len(low) - lv
            if k < 1 or lv < 1 or low[lv:] != full[len(full) - k:]:
                raise ValueError("restrict: the basis is not a prefix of the key's ciphertext moduli followed by "
                                 "its special primes")
            keep = list(range(lv)) + list(range(len(full) - k, len(full)))
            n_polys = -(-lv // self.alpha)
        if ext_basis_lv.degree != self.a.basis.degree:
            raise ValueError("restrict: ring degrees differ")
        halves = []
        for p in (self.a, self.b):
            ch = p.channels_of(0, n_polys)[:, keep, :]
            halves.append(RnsPoly.from_channels(ch, ext_basis_lv, in_ntt_domain=True))
        out = RnsHybridKey(halves[0], halves[1], self.alpha, self.rotation)
        out.hoisted = self.hoisted
        return out


def _at_ct_level(key, ct_basis: RnsBasis):
    """The key (an RnsHybridKey or RnsHybridKeySet) the call reads for a
    ciphertext on ``ct_basis``: where it carries ``n_special`` and the
    ciphertext has fewer limbs than the key's level, its view at that level
    (at_level); else the key as it is."""
    ns = getattr(key, "n_special", None)
    if ns is None or getattr(key, "level", None) is not None or key.a is None:
        return key
    lv = ct_basis.channel_count()
    if lv < key.a.basis.channel_count() - ns:
        return key.at_level(lv)
    return key


def keyswitch_hybrid(d: RnsPoly, key: RnsHybridKey) -> tuple[RnsPoly, RnsPoly]:
    """The hybrid key-switch sums of a coefficient-domain batch
    (rnt_keyswitch_hybrid): ``acc0 + acc1 s = d s' + small``."""
    _require_class(key, RnsHybridKey, "keyswitch_hybrid")
    _require_form(key, False, "keyswitch_hybrid")
    key = _at_ct_level(key, d.basis)
    acc0, acc1 = d._like(), d._like()
    check(load().rnt_keyswitch_hybrid(acc0.handle, acc1.handle, d.handle, key.a.handle, key.b.handle, key.alpha))
    return acc0, acc1


def rotate_ciphertext_hybrid(ct: Ciphertext, rotk: RnsHybridKey) -> Ciphertext:
    """rotate_ciphertext with the hybrid key-switch (rnt_ct_rotate_hybrid):
    the same rotation with less noise, not the gadget call's words."""
    _require_class(rotk, RnsHybridKey, "rotate_ciphertext_hybrid")
    _require_form(rotk, False, "rotate_ciphertext_hybrid")
    rotk = _at_ct_level(rotk, ct.c0.basis)
    out0, out1 = ct.c0._like(), ct.c0._like()
    check(load().rnt_ct_rotate_hybrid(out0.handle, out1.handle, ct.c0.handle, ct.c1.handle,
                                      int(rotk.rotation or 0), rotk.a.handle, rotk.b.handle, rotk.alpha))
    return Ciphertext(out0, out1, ct.logp, ct.logq)


def mul_ciphertexts_hybrid(ct1: Ciphertext, ct2: Ciphertext, rlk: RnsHybridKey) -> Ciphertext:
    """mul_ciphertexts_gadget with the hybrid key-switch (rnt_ct_mul_relin_hybrid)."""
    _require_class(rlk, RnsHybridKey, "mul_ciphertexts_hybrid")
    assert ct1.logq == ct2.logq, "logq mismatch in hybrid multiplication"
    rlk = _at_ct_level(rlk, ct1.c0.basis)
    out0, out1 = ct1.c0._like(), ct1.c0._like()
    check(load().rnt_ct_mul_relin_hybrid(out0.handle, out1.handle, ct1.c0.handle, ct1.c1.handle,
                                         ct2.c0.handle, ct2.c1.handle, rlk.a.handle, rlk.b.handle, rlk.alpha))
    return Ciphertext(out0, out1, ct1.logp + ct2.logp, ct1.logq)


def conjugate_hybrid(ct: Ciphertext, conj_key: RnsHybridKey) -> Ciphertext:
    """The complex conjugate of every slot: :func:`rotate_ciphertext_hybrid`
    with the hybrid rotation key of step ``-N/2``.  ``rotation_exponent(-N/2)``
    is ``5^(N/2) (2N - 1) = 2N - 1 mod 2N`` (5 has order N/2), the conjugation
    ``X -> X^-1``, so that key IS a conjugation key
    (``CkksEngine.generate_hybrid_conjugation_key``)."""
    _require_class(conj_key, RnsHybridKey, "conjugate_hybrid")
    if conj_key.rotation != -(ct.c0.basis.degree // 2):
        raise ValueError(f"conjugate_hybrid: needs the rotation key of step -N/2 = {-(ct.c0.basis.degree // 2)}, "
                         f"got step {conj_key.rotation}")
    return rotate_ciphertext_hybrid(ct, conj_key)


def mul_i(ct: Ciphertext, sign: int = 1) -> Ciphertext:
    """Every slot times ``i`` (``sign = +1``) or ``-i`` (``-1``): both
    components times ``X^(N/2)`` or ``X^(3N/2)`` (rnt_mul_monomial).  X^(N/2)
    evaluates to i in every slot (5^k = 1 mod 4), so this is an exact
    negacyclic shift: no level, no noise, logp and logq unchanged."""
    if sign not in (1, -1):
        raise ValueError("mul_i: sign is +1 or -1")
    n = ct.c0.basis.degree
    k = n // 2 if sign == 1 else 3 * n // 2
    return Ciphertext(ct.c0.mul_monomial(k), ct.c1.mul_monomial(k), ct.logp, ct.logq)


def split_real_imag_hybrid(ct: Ciphertext, conj_key: RnsHybridKey) -> tuple[Ciphertext, Ciphertext]:
    """``(ct_re, ct_im)`` with ``ct_re = ct + conj(ct)`` and ``ct_im = (ct -
    conj(ct)) X^(3N/2)``: ``2 Re`` and ``2 Im`` of the slots, carried as ``logp
    = ct.logp + 1`` so that they decode to ``Re`` and ``Im`` -- the factor 2 is
    exact and costs no level.  One key-switch."""
    cj = conjugate_hybrid(ct, conj_key)
    re = Ciphertext(ct.c0 + cj.c0, ct.c1 + cj.c1, ct.logp + 1, ct.logq)
    im = mul_i(Ciphertext(ct.c0 - cj.c0, ct.c1 - cj.c1, ct.logp + 1, ct.logq), -1)
    return re, im


def merge_real_imag(ct_re: Ciphertext, ct_im: Ciphertext) -> Ciphertext:
    """``ct_re + X^(N/2) ct_im``: slots ``re + i im``.  No key."""
    if ct_re.logp != ct_im.logp or ct_re.logq != ct_im.logq:
        raise ValueError("merge_real_imag: the two parts differ in logp or logq")
    t = mul_i(ct_im, 1)
    return Ciphertext(ct_re.c0 + t.c0, ct_re.c1 + t.c1, ct_re.logp, ct_re.logq)


class RnsHybridKeySet:
    """The hybrid rotation keys of several steps, packed on the device as
    rnt_ct_rotate_hybrid_hoisted and rnt_ct_linear_bsgs_hybrid read them:
    step t's ``beta`` key polys at ``[t beta, (t + 1) beta)`` of ``a`` / ``b``
    on the extended basis (rnt_copy_polys, no host round trip).  ``keys[t]``
    is an :class:`RnsHybridKey` whose ``rotation`` is the step, or None for a
    step of 0 (its slot stays zero and is never read).  The keys share one
    extended basis, one ``alpha`` and one form (``hoisted``); a set without
    any key serves both forms and needs ``alpha``."""

    def __init__(self, keys: Sequence[Optional[RnsHybridKey]], alpha: Optional[int] = None):
        keys = list(keys)
        if not keys:
            raise ValueError("RnsHybridKeySet: no steps")
        real = [k for k in keys if k is not None]
        for k in real:
            if not isinstance(k, RnsHybridKey):
                raise ValueError(f"RnsHybridKeySet: needs RnsHybridKey entries, got {type(k).__name__}")
        if len({bool(k.hoisted) for k in real}) > 1:
            raise ValueError("RnsHybridKeySet: a mix of hoisting-form and ordinary keys")
        if len({k.alpha for k in real} | ({int(alpha)} if alpha is not None else set())) > 1:
            raise ValueError("RnsHybridKeySet: the keys were generated for different alpha")
        if not real and alpha is None:
            raise ValueError("RnsHybridKeySet: a set of step-0 terms needs alpha")
        self.hoisted = bool(real[0].hoisted) if real else False
        self.alpha = real[0].alpha if real else int(alpha)
        self.steps = [0 if k is None else int(k.rotation or 0) for k in keys]
        self.basis = real[0].a.basis if real else None
        self.a = self.b = None
        if any(k.level is not None for k in real):
            raise ValueError("RnsHybridKeySet: pack full keys and take the set's view (at_level)")
        if len({k.n_special for k in real}) > 1:
            raise ValueError("RnsHybridKeySet: the keys carry different n_special")
        self.n_special = real[0].n_special if real else None
        self.level = None  # a view's level (at_level)
        self._views = {}
        if real:
            beta = real[0].a.n_polys
            for k in real:
                if k.a.basis is not self.basis and k.a.basis.moduli() != self.basis.moduli():
                    raise ValueError("RnsHybridKeySet: the keys are on different extended bases")
                if k.a.n_polys != beta:
                    raise ValueError("RnsHybridKeySet: the keys hold different digit counts")
            self.a = RnsPoly(self.basis, len(keys) * beta)
            self.b = RnsPoly(self.basis, len(keys) * beta)
            # (zero-filled: a zero poly is zero in both domains)
            self.a.to_ntt_domain()
            self.b.to_ntt_domain()
            for t, k in enumerate(keys):
                if k is not None:
                    self.a.copy_polys(k.a, t * beta, 0, beta)
                    self.b.copy_polys(k.b, t * beta, 0, beta)

    def at_level(self, level: int) -> "RnsHybridKeySet":
        """This set at a lower level, as a view of its packed planes
        (rnt_key_level_view; step t's key at ``[t beta', (t + 1) beta')`` of
        the view): no copy; it keeps ``alpha``, the steps and ``hoisted`` and
        holds this set alive.  Cached per level.  The keys must carry
        ``n_special``; a set without any key is its own view."""
        if self.level is not None:
            raise ValueError("at_level: the set is a level view already")
        if self.a is None:
            return self
        if self.n_special is None:
            raise ValueError("at_level: the set's keys carry no n_special")
        level = int(level)
        if level not in self._views:
            lb = self.basis.hybrid_level(self.n_special, level)
            v = RnsHybridKeySet.__new__(RnsHybridKeySet)
            v.hoisted, v.alpha, v.steps, v.basis = self.hoisted, self.alpha, list(self.steps), lb
            v.a = RnsPoly._key_level_view(self.a, lb, self.alpha)
            v.b = RnsPoly._key_level_view(self.b, lb, self.alpha)
            v.n_special, v.level, v._views, v._parent = self.n_special, level, {}, self
            self._views[level] = v
        return self._views[level]

    def __len__(self) -> int:
        return len(self.steps)


def _require_hybrid_set(keyset, hoisted: bool, what: str) -> None:
    if not isinstance(keyset, RnsHybridKeySet):
        raise ValueError(f"{what}: needs an RnsHybridKeySet, got {type(keyset).__name__}")
    if keyset.a is not None:
        _require_form(keyset, hoisted, what)


def rotate_ciphertext_hybrid_hoisted(ct: Ciphertext, keyset: RnsHybridKeySet,
                                     out: Optional[Ciphertext] = None) -> Ciphertext:
    """The hoisted hybrid rotations of every ciphertext of the batch by each
    of ``keyset.steps`` with one ModUp and one forward transform
    (rnt_ct_rotate_hybrid_hoisted): a batch of ``n_steps * B``, rotation t of
    ciphertext b at poly ``t * B + b``.  ``keyset`` is in hoisting form.
    Valid rotations with ``rotate_ciphertext_hybrid``'s noise, not its
    words."""
    _require_hybrid_set(keyset, True, "rotate_ciphertext_hybrid_hoisted")
    keyset = _at_ct_level(keyset, ct.c0.basis)
    basis = ct.c0.basis
    n_out = len(keyset.steps) * ct.c0.n_polys
    if out is None:
        out = Ciphertext(RnsPoly(basis, n_out, _uninit=True), RnsPoly(basis, n_out, _uninit=True), ct.logp, ct.logq)
    steps = (ctypes.c_int32 * len(keyset.steps))(*keyset.steps)
    check(load().rnt_ct_rotate_hybrid_hoisted(out.c0.handle, out.c1.handle, ct.c0.handle, ct.c1.handle, steps,
                                              len(keyset.steps), keyset.a.handle if keyset.a is not None else None,
                                              keyset.b.handle if keyset.b is not None else None, keyset.alpha))
    return out


def automorphism_ntt(poly: RnsPoly, g: int, out: Optional[RnsPoly] = None) -> RnsPoly:
    """``X -> X^g`` (g odd) on an NTT-domain polynomial without leaving the
    domain (rnt_automorphism_ntt): the words of
    ``to_ntt(automorphism(to_coeff(poly), g))``, word for word, by one gather.
    ``out`` must not be ``poly``."""
    if out is None:
        out = poly._like()
    check(load().rnt_automorphism_ntt(out.handle, poly.handle, int(g)))
    return out


def rotsum_ciphertext_hybrid(ct: Ciphertext, keyset: RnsHybridKeySet, out: Optional[Ciphertext] = None) -> Ciphertext:
    """``sum_t rotate(ct, keyset.steps[t])`` for every ciphertext of the batch
    (rnt_ct_rotsum_hybrid): one ModUp and one forward transform for every step,
    the key products of all steps summed over the extended basis and divided
    by P once.  A step of 0 adds the ciphertext itself.  ``keyset`` holds
    ORDINARY prepared keys.  It spends no level and no scale; ``out`` may be
    ``ct`` (a chain of stages runs in place).  The same decryption as a chain
    of ``rotate_ciphertext_hybrid`` and additions with less ModDown error, not
    its words."""
    _require_hybrid_set(keyset, False, "rotsum_ciphertext_hybrid")
    keyset = _at_ct_level(keyset, ct.c0.basis)
    if out is None:
        out = Ciphertext(ct.c0._like(), ct.c0._like(), ct.logp, ct.logq)
    steps = (ctypes.c_int32 * len(keyset.steps))(*keyset.steps)
    check(load().rnt_ct_rotsum_hybrid(out.c0.handle, out.c1.handle, ct.c0.handle, ct.c1.handle, steps,
                                      len(keyset.steps), keyset.a.handle if keyset.a is not None else None,
                                      keyset.b.handle if keyset.b is not None else None, keyset.alpha))
    return out


def linear_transform_bsgs_hybrid(ct: Ciphertext, diag: RnsPoly, baby_keyset: RnsHybridKeySet,
                                 giant_keyset: RnsHybridKeySet, out: Optional[Ciphertext] = None) -> Ciphertext:
    """:func:`linear_transform_bsgs` on hybrid keys
    (rnt_ct_linear_bsgs_hybrid): the baby rotations hoisted (``baby_keyset``
    in hoisting form), the giant rotations (``giant_keyset`` ordinary) summed
    over the extended basis and divided by P once.  ``diag`` as
    :func:`linear_transform_bsgs` takes it; ``out`` may be ``ct``."""
    _require_hybrid_set(baby_keyset, True, "linear_transform_bsgs_hybrid (baby keys)")
    _require_hybrid_set(giant_keyset, False, "linear_transform_bsgs_hybrid (giant keys)")
    if baby_keyset.alpha != giant_keyset.alpha:
        raise ValueError("linear_transform_bsgs_hybrid: the two key sets were generated for different alpha")
    baby_keyset = _at_ct_level(baby_keyset, ct.c0.basis)
    giant_keyset = _at_ct_level(giant_keyset, ct.c0.basis)
    basis = ct.c0.basis
    if out is None:
        out = Ciphertext(ct.c0._like(basis), ct.c0._like(basis), ct.logp, ct.logq)
    baby = (ctypes.c_int32 * len(baby_keyset.steps))(*baby_keyset.steps)
    giant = (ctypes.c_int32 * len(giant_keyset.steps))(*giant_keyset.steps)

    def h(p):
        return p.handle if p is not None else None

    check(load().rnt_ct_linear_bsgs_hybrid(out.c0.handle, out.c1.handle, ct.c0.handle, ct.c1.handle, baby,
                                           len(baby_keyset.steps), giant, len(giant_keyset.steps), diag.handle,
                                           h(baby_keyset.a), h(baby_keyset.b), h(giant_keyset.a), h(giant_keyset.b),
                                           baby_keyset.alpha))
    return out


def linear_transform_hybrid(ct: Ciphertext, diag: RnsPoly, keyset: RnsHybridKeySet,
                            out: Optional[Ciphertext] = None) -> Ciphertext:
    """``sum_t diag[t] * R_t`` over the hoisted hybrid rotations ``R_t`` of
    ``ct`` by ``keyset.steps``: :func:`linear_transform_bsgs_hybrid` with the
    single giant step 0."""
    _require_hybrid_set(keyset, True, "linear_transform_hybrid")
    return linear_transform_bsgs_hybrid(ct, diag, keyset, RnsHybridKeySet([None], keyset.alpha), out)


class RnsGadgetKeySet:
    """The gadget keys of a linear transform's terms, packed on the device as
    rnt_ct_linear reads them: term t's L key polys at ``[t L, (t + 1) L)`` of
    ``a`` / ``b`` (rnt_copy_polys, no host round trip).  ``keys[t]`` is a
    prepared :class:`RnsGadgetKey` whose ``rotation`` is the term's step, or
    None for a step-0 term (its slot stays zero and is never read).  The keys
    are all ordinary or all in hoisting form (``hoisted``); a set without any
    key serves both."""

    def __init__(self, keys: Sequence[Optional[RnsGadgetKey]], basis: Optional[RnsBasis] = None):
        keys = list(keys)
        if not keys:
            raise ValueError("RnsGadgetKeySet: no terms")
        forms = {bool(getattr(k, "hoisted", False)) for k in keys if k is not None}
        if len(forms) > 1:
            raise ValueError("RnsGadgetKeySet: a mix of hoisting-form and ordinary keys")
        self.hoisted = forms.pop() if forms else False
        first = next((k for k in keys if k is not None), None)
        if first is None and basis is None:
            raise ValueError("RnsGadgetKeySet: a set of step-0 terms needs the basis")
        self.basis = basis if basis is not None else first.a.basis
        self.steps = [0 if k is None else int(k.rotation or 0) for k in keys]
        L = self.basis.channel_count()
        self.a = self.b = None
        if first is not None:
            self.a = RnsPoly(self.basis, len(keys) * L)
            self.b = RnsPoly(self.basis, len(keys) * L)
            # (zero-filled coefficient-domain buffers; a zero poly is zero in
            # both domains, so the slots written below decide nothing else)
            self.a.to_ntt_domain()
            self.b.to_ntt_domain()
            for t, k in enumerate(keys):
                if k is not None:
                    self.a.copy_polys(k.a, t * L, 0, L)
                    self.b.copy_polys(k.b, t * L, 0, L)

    def __len__(self) -> int:
        return len(self.steps)


def linear_transform(ct: Ciphertext, diag: RnsPoly, keyset: RnsGadgetKeySet,
                     out: Optional[Ciphertext] = None) -> Ciphertext:
    """``sum_t diag[t] * rotate_ciphertext(ct, keyset.steps[t])`` for every
    ciphertext of the batch (rnt_ct_linear): ``diag`` holds one NTT-domain
    plaintext poly per term.  ``out`` may be ``ct`` itself (in place)."""
    if keyset.a is not None:
        _require_form(keyset, False, "linear_transform")
    basis = ct.c0.basis
    if out is None:
        out = Ciphertext(ct.c0._like(basis), ct.c0._like(basis), ct.logp, ct.logq)
    steps = (ctypes.c_int32 * len(keyset.steps))(*keyset.steps)
    check(load().rnt_ct_linear(out.c0.handle, out.c1.handle, ct.c0.handle, ct.c1.handle, steps,
                               len(keyset.steps), diag.handle,
                               keyset.a.handle if keyset.a is not None else None,
                               keyset.b.handle if keyset.b is not None else None))
    return out


def linear_transform_bsgs(ct: Ciphertext, diag: RnsPoly, baby_keyset: RnsGadgetKeySet,
                          giant_keyset: RnsGadgetKeySet, out: Optional[Ciphertext] = None) -> Ciphertext:
    """The baby-step giant-step form of :func:`linear_transform`
    (rnt_ct_linear_bsgs): with ``b = baby_keyset.steps`` (n1 of them) and
    ``g = giant_keyset.steps`` (n2),

        ``sum_j rotate(sum_i diag[j n1 + i] * rotate(ct, b[i]), g[j])``

    for every ciphertext of the batch -- at most n1 + n2 key-switches for the
    n1 n2 diagonals ``g[j] + b[i]``.  ``diag`` holds the n2 n1 NTT-domain
    plaintext polys (:func:`bsgs_diagonal_rows` gives their slots).  ``out``
    may be ``ct`` itself (in place)."""
    return _linear_bsgs(ct, diag, baby_keyset, giant_keyset, out, False)


def linear_transform_bsgs_hoisted(ct: Ciphertext, diag: RnsPoly, baby_keyset: RnsGadgetKeySet,
                                  giant_keyset: RnsGadgetKeySet, out: Optional[Ciphertext] = None) -> Ciphertext:
    """:func:`linear_transform_bsgs` with the baby rotations hoisted
    (rnt_ct_linear_bsgs_hoisted): one gadget decomposition of ``ct`` serves
    every baby step.  ``baby_keyset`` is in hoisting form, ``giant_keyset``
    ordinary.  A valid transform with the same noise, but not
    ``linear_transform_bsgs``' words."""
    return _linear_bsgs(ct, diag, baby_keyset, giant_keyset, out, True)


def _linear_bsgs(ct, diag, baby_keyset, giant_keyset, out, hoisted: bool):
    name = "linear_transform_bsgs_hoisted" if hoisted else "linear_transform_bsgs"
    if baby_keyset.a is not None:
        _require_form(baby_keyset, hoisted, f"{name} (baby keys)")
    if giant_keyset.a is not None:
        _require_form(giant_keyset, False, f"{name} (giant keys)")
    basis = ct.c0.basis
    if out is None:
        out = Ciphertext(ct.c0._like(basis), ct.c0._like(basis), ct.logp, ct.logq)
    baby = (ctypes.c_int32 * len(baby_keyset.steps))(*baby_keyset.steps)
    giant = (ctypes.c_int32 * len(giant_keyset.steps))(*giant_keyset.steps)

    def h(p):
        return p.handle if p is not None else None

    fn = load().rnt_ct_linear_bsgs_hoisted if hoisted else load().rnt_ct_linear_bsgs
    check(fn(out.c0.handle, out.c1.handle, ct.c0.handle, ct.c1.handle, baby, len(baby_keyset.steps), giant,
             len(giant_keyset.steps), diag.handle, h(baby_keyset.a), h(baby_keyset.b), h(giant_keyset.a),
             h(giant_keyset.b)))
    return out


def rotate_ciphertext_hoisted(ct: Ciphertext, keyset: RnsGadgetKeySet,
                              out: Optional[Ciphertext] = None) -> Ciphertext:
    """The hoisted rotations of every ciphertext of the batch by each of
    ``keyset.steps`` with one gadget decomposition (rnt_ct_rotate_hoisted):
    a batch of ``n_steps * B``, rotation t of ciphertext b at poly
    ``t * B + b``.  ``keyset`` is in hoisting form
    (``generate_rotation_key_set(..., hoisted=True)``).  Valid rotations with
    ``rotate_ciphertext``'s noise, not its words."""
    if keyset.a is not None:
        _require_form(keyset, True, "rotate_ciphertext_hoisted")
    basis = ct.c0.basis
    n_out = len(keyset.steps) * ct.c0.n_polys
    if out is None:
        out = Ciphertext(RnsPoly(basis, n_out, _uninit=True), RnsPoly(basis, n_out, _uninit=True), ct.logp, ct.logq)
    steps = (ctypes.c_int32 * len(keyset.steps))(*keyset.steps)
    check(load().rnt_ct_rotate_hoisted(out.c0.handle, out.c1.handle, ct.c0.handle, ct.c1.handle, steps,
                                       len(keyset.steps), keyset.a.handle if keyset.a is not None else None,
                                       keyset.b.handle if keyset.b is not None else None))
    return out


def bsgs_diagonal_rows(matrix, baby_steps, giant_steps) -> np.ndarray:
    """The plaintext slot vectors of a slots x slots matrix for
    :func:`linear_transform_bsgs`, ``[n2][n1][slots]``:

        ``rows[j][i][s] = M[(s - g_j) mod slots][(s + b_i) mod slots]``

    -- diagonal ``g_j + b_i`` of the matrix, rotated back by its giant step
    (slot s of a rotation by k holds old slot s + k), so that
    ``sum_j rot_{g_j}(sum_i rows[j][i] * rot_{b_i}(x)) = M_banded x`` with
    M_banded the matrix restricted to those diagonals.  Pure numpy.  Steps
    are slot rotations in ``[0, slots)``: a negative step raises ValueError
    (pass ``slots - k``), and so do two pairs that name one diagonal."""
    m = np.asarray(matrix)
    if m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError("bsgs_diagonal_rows: the matrix must be square")
    slots = m.shape[0]
    baby = [int(b) for b in baby_steps]
    giant = [int(g) for g in giant_steps]
    if not baby or not giant:
        raise ValueError("bsgs_diagonal_rows: no steps")
    if any(k < 0 for k in baby + giant):
        raise ValueError("bsgs_diagonal_rows: negative step (pass slots - k for a rotation by -k)")
    seen = {}
    for j, g in enumerate(giant):
        for i, b in enumerate(baby):
            d = (g + b) % slots
            if d in seen:
                raise ValueError(f"bsgs_diagonal_rows: pairs {seen[d]} and {(j, i)} both give diagonal {d}")
            seen[d] = (j, i)
    s = np.arange(slots)
    return np.stack([np.stack([m[(s - g) % slots, (s + b) % slots] for b in baby]) for g in giant])


def mul_ciphertexts_gadget_rescale(ct1: Ciphertext, ct2: Ciphertext, rlk: RnsGadgetKey) -> Ciphertext:
    """mul_ciphertexts_gadget then rescale_ciphertext (engine.rs:473-539,
    :263-282) as one op (rnt_ct_mul_relin_rescale): equal word for word to
    the two calls, with the rescale fused into the key-switch inverse."""
    assert ct1.logq == ct2.logq, "logq mismatch in gadget multiplication"
    q_last = ct1.c0.basis.moduli()[-1]
    bits_dropped = q_last.bit_length()
    new_basis = ct1.c0.basis.drop_last(1)
    out0, out1 = ct1.c0._like(new_basis), ct1.c0._like(new_basis)
    check(load().rnt_ct_mul_relin_rescale(out0.handle, out1.handle, ct1.c0.handle, ct1.c1.handle,
                                          ct2.c0.handle, ct2.c1.handle, rlk.a.handle, rlk.b.handle))
    return Ciphertext(out0, out1, ct1.logp + ct2.logp - bits_dropped, ct1.logq - bits_dropped)


def mul_ciphertexts_hybrid_rescale(ct1: Ciphertext, ct2: Ciphertext, rlk: RnsHybridKey,
                                   out_basis: Optional[RnsBasis] = None) -> Ciphertext:
    """mul_ciphertexts_hybrid then rescale_ciphertext as one op
    (rnt_ct_mul_relin_rescale_hybrid): equal word for word to the two calls;
    the un-rescaled product never reaches memory.  ``out_basis`` (a
    ``drop_last(1)`` of the inputs' basis) receives the result where a circuit
    keeps one basis object per level; by default a fresh one is made."""
    _require_class(rlk, RnsHybridKey, "mul_ciphertexts_hybrid_rescale")
    assert ct1.logq == ct2.logq, "logq mismatch in hybrid multiplication"
    rlk = _at_ct_level(rlk, ct1.c0.basis)
    q_last = ct1.c0.basis.moduli()[-1]
    bits_dropped = q_last.bit_length()
    new_basis = out_basis if out_basis is not None else ct1.c0.basis.drop_last(1)
    out0, out1 = ct1.c0._like(new_basis), ct1.c0._like(new_basis)
    check(load().rnt_ct_mul_relin_rescale_hybrid(out0.handle, out1.handle, ct1.c0.handle, ct1.c1.handle,
                                                 ct2.c0.handle, ct2.c1.handle, rlk.a.handle, rlk.b.handle,
                                                 rlk.alpha))
    return Ciphertext(out0, out1, ct1.logp + ct2.logp - bits_dropped, ct1.logq - bits_dropped)


def mul_ciphertexts_hybrid_rescale_affine(ct1: Ciphertext, ct2: Ciphertext, rlk: RnsHybridKey, weight: int = 1,
                                         addend: Optional[Ciphertext] = None, addend_weight: int = 1, bias: int = 0,
                                         out_basis: Optional[RnsBasis] = None) -> Ciphertext:
    """``weight * (ct1 * ct2) + addend_weight * addend + bias`` with the
    product relinearised and rescaled, as one op
    (rnt_ct_mul_relin_rescale_affine_hybrid): word for word
    :func:`mul_ciphertexts_hybrid_rescale` followed by an un-rescaled
    :func:`ct_lincomb` on the product and the addend, the affine step in the
    epilogue of the kernels that close the multiply -- no launch and no pass
    over the ciphertext of its own, and nothing copied from the host, so the
    call can be recorded.  ``weight``, ``addend_weight`` (below 2^31 in
    magnitude) and ``bias`` (below 2^62) are signed Python ints; the bias is
    the constant in every slot at the result's scale (it is added after the
    rescale), and the weights do not change logp.  ``addend`` lives at the result's level, on the result's basis
    object (``out_basis``, by default the addend's own), with the result's logp
    and logq: anything else raises ValueError.  logp / logq are the
    multiply's."""
    _require_class(rlk, RnsHybridKey, "mul_ciphertexts_hybrid_rescale_affine")
    assert ct1.logq == ct2.logq, "logq mismatch in hybrid multiplication"
    rlk = _at_ct_level(rlk, ct1.c0.basis)
    bits_dropped = ct1.c0.basis.moduli()[-1].bit_length()
    logp, logq = ct1.logp + ct2.logp - bits_dropped, ct1.logq - bits_dropped
    if addend is not None:
        if addend.logp != logp or addend.logq != logq:
            raise ValueError(f"mul_ciphertexts_hybrid_rescale_affine: the addend's (logp, logq) = ({addend.logp}, "
                             f"{addend.logq}) is not the result's ({logp}, {logq})")
        if out_basis is None:
            out_basis = addend.c0.basis
    new_basis = out_basis if out_basis is not None else ct1.c0.basis.drop_last(1)
    out0, out1 = ct1.c0._like(new_basis), ct1.c0._like(new_basis)
    check(load().rnt_ct_mul_relin_rescale_affine_hybrid(
        out0.handle, out1.handle, ct1.c0.handle, ct1.c1.handle, ct2.c0.handle, ct2.c1.handle, rlk.a.handle,
        rlk.b.handle, rlk.alpha, int(weight), None if addend is None else addend.c0.handle,
        None if addend is None else addend.c1.handle, int(addend_weight), int(bias)))
    return Ciphertext(out0, out1, logp, logq)


def linear_transform_bsgs_hybrid_rescale(ct: Ciphertext, diag: RnsPoly, baby_keyset: RnsHybridKeySet,
                                         giant_keyset: RnsHybridKeySet,
                                         out_basis: Optional[RnsBasis] = None) -> Ciphertext:
    """:func:`linear_transform_bsgs_hybrid` then rescale_ciphertext as one op
    (rnt_ct_linear_bsgs_hybrid_rescale): equal word for word to the two
    calls, the closing ModDowns and the rescale in one kernel each.
    ``out_basis`` as in :func:`mul_ciphertexts_hybrid_rescale`."""
    _require_hybrid_set(baby_keyset, True, "linear_transform_bsgs_hybrid_rescale (baby keys)")
    _require_hybrid_set(giant_keyset, False, "linear_transform_bsgs_hybrid_rescale (giant keys)")
    if baby_keyset.alpha != giant_keyset.alpha:
        raise ValueError("linear_transform_bsgs_hybrid_rescale: the two key sets were generated for different alpha")
    baby_keyset = _at_ct_level(baby_keyset, ct.c0.basis)
    giant_keyset = _at_ct_level(giant_keyset, ct.c0.basis)
    q_last = ct.c0.basis.moduli()[-1]
    bits_dropped = q_last.bit_length()
    new_basis = out_basis if out_basis is not None else ct.c0.basis.drop_last(1)
    out0, out1 = ct.c0._like(new_basis), ct.c0._like(new_basis)
    baby = (ctypes.c_int32 * len(baby_keyset.steps))(*baby_keyset.steps)
    giant = (ctypes.c_int32 * len(giant_keyset.steps))(*giant_keyset.steps)

    def h(p):
        return p.handle if p is not None else None

    check(load().rnt_ct_linear_bsgs_hybrid_rescale(out0.handle, out1.handle, ct.c0.handle, ct.c1.handle, baby,
                                                   len(baby_keyset.steps), giant, len(giant_keyset.steps),
                                                   diag.handle, h(baby_keyset.a), h(baby_keyset.b),
                                                   h(giant_keyset.a), h(giant_keyset.b), baby_keyset.alpha))
    return Ciphertext(out0, out1, ct.logp - bits_dropped, ct.logq - bits_dropped)


def hybrid_level_moduli(ext_basis: RnsBasis, n_special: int, level: int) -> list:
    """The moduli ``q_0..q_{level-1}, p_0..p_{K-1}`` of a hybrid key basis at a
    level: what the plaintexts of :func:`linear_bsgs_hybrid_dh` are encoded
    over.  A level basis (``hybrid_level``) holds key views alone, so below the
    top level the plaintexts live on a root basis over these moduli; at the top
    level ``ext_basis`` itself serves."""
    mods = ext_basis.moduli()
    K, level = int(n_special), int(level)
    if not 0 < K < len(mods) or not 0 < level <= len(mods) - K:
        raise ValueError(f"hybrid_level_moduli: level {level} with {K} special primes of {len(mods)} moduli")
    return mods[:level] + mods[len(mods) - K:]


def linear_bsgs_hybrid_dh(ct: Ciphertext, diagE: RnsPoly, baby_keyset: RnsHybridKeySet,
                          giant_keyset: RnsHybridKeySet, rescale: bool = False, out: Optional[Ciphertext] = None,
                          out_basis: Optional[RnsBasis] = None) -> Ciphertext:
    """The double-hoisted form of :func:`linear_transform_bsgs_hybrid`
    (rnt_ct_linear_bsgs_hybrid_dh): the baby rotations stay over ``Q u P`` in
    the NTT domain, the inner sums are formed there against ``diagE`` -- the
    same plaintexts encoded over the key basis at the ciphertext's level
    (:func:`hybrid_level_moduli`), NTT domain -- and only one component per
    rotating giant and the two final sums are divided by P.  The SAME key sets
    as :func:`linear_transform_bsgs_hybrid` (baby keys in hoisting form, giant
    keys ordinary); the same decryption with less ModDown error, not its
    words.  ``rescale``: followed by rescale_ciphertext, word for word, as one
    op (``out_basis`` as in :func:`mul_ciphertexts_hybrid_rescale`); without it
    ``out`` may be ``ct``."""
    name = "linear_bsgs_hybrid_dh"
    _require_hybrid_set(baby_keyset, True, f"{name} (baby keys)")
    _require_hybrid_set(giant_keyset, False, f"{name} (giant keys)")
    if baby_keyset.alpha != giant_keyset.alpha:
        raise ValueError(f"{name}: the two key sets were generated for different alpha")
    baby_keyset = _at_ct_level(baby_keyset, ct.c0.basis)
    giant_keyset = _at_ct_level(giant_keyset, ct.c0.basis)
    logp, logq = ct.logp, ct.logq
    if rescale:
        bits_dropped = ct.c0.basis.moduli()[-1].bit_length()
        logp, logq = logp - bits_dropped, logq - bits_dropped
        if out is None:
            new_basis = out_basis if out_basis is not None else ct.c0.basis.drop_last(1)
            out = Ciphertext(ct.c0._like(new_basis), ct.c0._like(new_basis), logp, logq)
    elif out is None:
        out = Ciphertext(ct.c0._like(), ct.c0._like(), logp, logq)
    baby = (ctypes.c_int32 * len(baby_keyset.steps))(*baby_keyset.steps)
    giant = (ctypes.c_int32 * len(giant_keyset.steps))(*giant_keyset.steps)

    def h(p):
        return p.handle if p is not None else None

    fn = load().rnt_ct_linear_bsgs_hybrid_dh_rescale if rescale else load().rnt_ct_linear_bsgs_hybrid_dh
    check(fn(out.c0.handle, out.c1.handle, ct.c0.handle, ct.c1.handle, baby, len(baby_keyset.steps), giant,
             len(giant_keyset.steps), diagE.handle, h(baby_keyset.a), h(baby_keyset.b), h(giant_keyset.a),
             h(giant_keyset.b), baby_keyset.alpha))
    out.logp, out.logq = logp, logq
    return out


def ct_lincomb(ct: Ciphertext, n_in: int, weights, bias=None, rescale: bool = True,
               out_basis: Optional[RnsBasis] = None) -> Ciphertext:
    """``n_out`` scalar linear combinations of the ``n_in`` ciphertexts packed
    in ``ct`` (a batch of ``n_in * B``, term i of ciphertext b at ``i * B + b``,
    the layout ``rotate_ciphertext_hybrid_hoisted`` writes) in one launch
    (rnt_ct_lincomb / rnt_ct_lincomb_rescale): output j is ``sum_i
    weights[j][i] * ct_i + bias[j]``, a batch of ``n_out * B`` with output j of
    ciphertext b at ``j * B + b``.  ``weights`` ([n_out][n_in]) and ``bias``
    ([n_out] or None) are signed Python ints, reduced mod every q_t here; a
    bias is the constant in every slot, at the scale the caller means (the
    products' scale).  With ``rescale`` the result is rescaled in the same
    kernel, word for word ``rescale_ciphertext`` of the un-rescaled call, and
    logp / logq drop by the bit length of the limb rescaled away.  logp does
    not grow by the weights' scale: the caller adds it.  ``out_basis`` as in
    :func:`mul_ciphertexts_hybrid_rescale`."""
    n_in = int(n_in)
    rows = [[int(v) for v in row] for row in weights]
    if n_in < 1 or not rows or any(len(r) != n_in for r in rows):
        raise ValueError("ct_lincomb: weights must be [n_out][n_in] with n_out, n_in >= 1")
    if ct.c0.n_polys % n_in != 0:
        raise ValueError(f"ct_lincomb: a batch of {ct.c0.n_polys} polys is no {n_in} terms of ciphertexts")
    if bias is not None and len(bias) != len(rows):
        raise ValueError("ct_lincomb: bias must have one entry per output")
    basis = ct.c0.basis
    mods = basis.moduli()
    n_out, B = len(rows), ct.c0.n_polys // n_in
    w = np.array([[[v % q for q in mods] for v in row] for row in rows], dtype=np.uint64)
    b = None if bias is None else np.array([[int(v) % q for q in mods] for v in bias], dtype=np.uint64)
    bits_dropped = 0
    if rescale:
        if len(mods) < 2:
            raise RnsNttError(_lib.INVALID_MOD_DROP, f"invalid mod-drop count 1 for {len(mods)} channels",
                              {"drop_count": 1, "channel_count": len(mods)})
        bits_dropped = mods[-1].bit_length()
        new_basis = out_basis if out_basis is not None else basis.drop_last(1)
    else:
        new_basis = out_basis if out_basis is not None else basis
    out0 = RnsPoly(new_basis, n_out * B, _uninit=True)
    out1 = RnsPoly(new_basis, n_out * B, _uninit=True)
    call = load().rnt_ct_lincomb_rescale if rescale else load().rnt_ct_lincomb
    check(call(out0.handle, out1.handle, ct.c0.handle, ct.c1.handle, n_in, n_out, _u64p(w),
               None if b is None else _u64p(b)))
    return Ciphertext(out0, out1, ct.logp - bits_dropped, ct.logq - bits_dropped)


def dot_ciphertexts_hybrid(ctx: Ciphertext, cty: Ciphertext, n_terms: int, rlk: RnsHybridKey,
                           rescale: bool = True, out_basis: Optional[RnsBasis] = None) -> Ciphertext:
    """``sum_i ctx_i * cty_i`` over the ``n_terms`` ciphertexts packed in each
    operand (a batch of ``n_terms * B``, term i of ciphertext b at ``i * B +
    b``, the layout ``ct_lincomb`` reads) with ONE relinearisation
    (rnt_ct_dot_relin_hybrid / rnt_ct_dot_relin_rescale_hybrid): the three
    tensor components are summed first, the key-switch runs on their d2, and
    with ``rescale`` the result is rescaled in the closing kernels.  ``cty``
    may be ``ctx`` itself (a sum of squares).  A batch of ``B`` comes back; its
    words are those of the coefficient-domain composition, not of ``n_terms``
    hybrid multiplies added up (the same message, the key-switch error once).
    logp / logq as in :func:`mul_ciphertexts_hybrid_rescale`; ``out_basis``
    likewise (``drop_last(1)`` of the inputs' with ``rescale``, else theirs)."""
    _require_class(rlk, RnsHybridKey, "dot_ciphertexts_hybrid")
    assert ctx.logq == cty.logq, "logq mismatch in hybrid inner product"
    n_terms = int(n_terms)
    if n_terms < 1 or ctx.c0.n_polys % n_terms != 0:
        raise ValueError(f"dot_ciphertexts_hybrid: a batch of {ctx.c0.n_polys} polys is no {n_terms} terms of "
                         "ciphertexts")
    basis = ctx.c0.basis
    rlk = _at_ct_level(rlk, basis)
    bits_dropped = 0
    if rescale:
        bits_dropped = basis.moduli()[-1].bit_length()
        new_basis = out_basis if out_basis is not None else basis.drop_last(1)
    else:
        new_basis = out_basis if out_basis is not None else basis
    B = ctx.c0.n_polys // n_terms
    out0 = RnsPoly(new_basis, B, _uninit=True)
    out1 = RnsPoly(new_basis, B, _uninit=True)
    call = load().rnt_ct_dot_relin_rescale_hybrid if rescale else load().rnt_ct_dot_relin_hybrid
    check(call(out0.handle, out1.handle, ctx.c0.handle, ctx.c1.handle, cty.c0.handle, cty.c1.handle, n_terms,
               rlk.a.handle, rlk.b.handle, rlk.alpha))
    return Ciphertext(out0, out1, ctx.logp + cty.logp - bits_dropped, ctx.logq - bits_dropped)


def ct_plain_mac(ct: Ciphertext, n_terms: int, pt: RnsPoly, bias: Optional[RnsPoly] = None, rescale: bool = True,
                 out_basis: Optional[RnsBasis] = None) -> Ciphertext:
    """``sum_i ct_i * pt_i + bias`` over the ``n_terms`` ciphertexts packed in
    ``ct`` (a batch of ``n_terms * B``, term i of ciphertext b at ``i * B + b``,
    the layout ``ct_lincomb`` reads and ``rotate_ciphertext_hybrid_hoisted``
    writes) with encoded plaintexts (rnt_ct_plain_mac /
    rnt_ct_plain_mac_rescale).  ``pt`` is an NTT-domain ``RnsPoly`` on the
    ciphertexts' basis: ``n_terms`` polys, plaintext i for every ciphertext, or
    ``n_terms * B``, term i of ciphertext b at ``i * B + b``.  ``bias`` is None
    or an NTT-domain ``RnsPoly`` of 1 or ``B`` polys, added to ``c0``, at the
    scale the caller means (the products' scale).  A batch of ``B`` comes back;
    its words are those of the coefficient-domain composition.  With
    ``rescale`` the result is ``rescale_ciphertext`` of the un-rescaled call,
    word for word, and logp / logq drop by the bit length of the limb rescaled
    away.  logp does not grow by the plaintexts' scale: the caller adds it.
    ``out_basis`` as in :func:`mul_ciphertexts_hybrid_rescale`."""
    n_terms = int(n_terms)
    if n_terms < 1 or ct.c0.n_polys % n_terms != 0 or ct.c1.n_polys != ct.c0.n_polys:
        raise ValueError(f"ct_plain_mac: a batch of {ct.c0.n_polys} polys is no {n_terms} terms of ciphertexts")
    B = ct.c0.n_polys // n_terms
    if not isinstance(pt, RnsPoly) or (bias is not None and not isinstance(bias, RnsPoly)):
        raise ValueError("ct_plain_mac: the plaintexts and the bias are RnsPoly batches in the NTT domain")
    if pt.n_polys not in (n_terms, n_terms * B):
        raise ValueError(f"ct_plain_mac: {pt.n_polys} plaintexts for {n_terms} terms of a batch of {B}")
    if bias is not None and bias.n_polys not in (1, B):
        raise ValueError(f"ct_plain_mac: a bias of {bias.n_polys} polys for a batch of {B}")
    if not pt.is_ntt_domain() or (bias is not None and not bias.is_ntt_domain()):
        raise ValueError("ct_plain_mac: the plaintexts and the bias must be in the NTT domain")
    basis = ct.c0.basis
    bits_dropped = 0
    if rescale:
        mods = basis.moduli()
        if len(mods) < 2:
            raise RnsNttError(_lib.INVALID_MOD_DROP, f"invalid mod-drop count 1 for {len(mods)} channels",
                              {"drop_count": 1, "channel_count": len(mods)})
        bits_dropped = mods[-1].bit_length()
        new_basis = out_basis if out_basis is not None else basis.drop_last(1)
    else:
        new_basis = out_basis if out_basis is not None else basis
    out0 = RnsPoly(new_basis, B, _uninit=True)
    out1 = RnsPoly(new_basis, B, _uninit=True)
    call = load().rnt_ct_plain_mac_rescale if rescale else load().rnt_ct_plain_mac
    check(call(out0.handle, out1.handle, ct.c0.handle, ct.c1.handle, pt.handle,
               None if bias is None else bias.handle, n_terms))
    return Ciphertext(out0, out1, ct.logp - bits_dropped, ct.logq - bits_dropped)


def mul_plain(ct: Ciphertext, pt: RnsPoly, rescale: bool = True) -> Ciphertext:
    """``ct * pt`` for an NTT-domain plaintext (one poly for the whole batch,
    or one per ciphertext): :func:`ct_plain_mac` with one term."""
    return ct_plain_mac(ct, 1, pt, None, rescale)


def rescale_ciphertext(ct: Ciphertext) -> Ciphertext:
    """engine.rs:263-282: both components onto one shared dropped basis."""
    q_last = ct.c0.basis.moduli()[-1]
    bits_dropped = q_last.bit_length()
    new_basis = ct.c0.basis.drop_last(1)
    out0, out1 = ct.c0._like(new_basis), ct.c0._like(new_basis)
    check(load().rnt_ct_rescale(out0.handle, out1.handle, ct.c0.handle, ct.c1.handle))
    return Ciphertext(out0, out1, ct.logp - bits_dropped, ct.logq - bits_dropped)


# ---------------------------------------------------------------------------
# CKKS encoder (src/encoding/ckks_encoder.rs)
# ---------------------------------------------------------------------------


@dataclass
class Plaintext:
    """types.rs Plaintext: an encoded RnsPoly batch (one row of slots per
    poly), its scale and slot count."""

    poly: RnsPoly
    scale_bits: int
    slots: int


class CkksEncoder:
    """``CkksEncoder<DEGREE>`` (ckks_encoder.rs:32-157).  The canonical
    embedding runs on the device as an O(N log N) special FFT
    (rnt_encode / rnt_decode) instead of the reference's O(N^2) Vandermonde
    evaluation; a 2-D ``values`` encodes one poly per row."""

    def __init__(self, degree: int, scale_bits: int):
        if degree <= 0 or degree & (degree - 1):
            raise ValueError("CkksEncoder: DEGREE must be a power of two")
        if scale_bits <= 0:
            raise ValueError("CkksEncoder: scale_bits must be positive")
        self.degree = degree
        self.scale_bits = scale_bits

    def scale_factor(self) -> float:
        return 2.0 ** self.scale_bits

    def max_slots(self) -> int:
        return self.degree // 2

    def encode(self, values, basis: RnsBasis) -> Plaintext:
        """ckks_encoder.rs:65-82: real values, imaginary parts zero."""
        return self.encode_complex(np.asarray(values, dtype=np.float64), basis, _name="encode")

    def encode_complex(self, values, basis: RnsBasis, _name: str = "encode_complex") -> Plaintext:
        """ckks_encoder.rs:85-99."""
        if basis.degree != self.degree:
            raise ValueError(f"{_name}: basis degree {basis.degree} != encoder degree {self.degree}")
        v = np.asarray(values, dtype=np.complex128)
        rows = v.reshape(1, -1) if v.ndim <= 1 else v
        if rows.ndim != 2:
            raise ValueError(f"{_name}: values must be 1-D (one poly) or 2-D (one row per poly)")
        n_values = rows.shape[1]
        if n_values > self.degree // 2:
            raise ValueError(f"{_name}: {n_values} values exceed max slots {self.degree // 2}")
        buf = np.ascontiguousarray(rows)
        poly = RnsPoly(basis, None if v.ndim <= 1 else rows.shape[0])
        check(load().rnt_encode(poly.handle, buf.ctypes.data_as(ctypes.c_void_p), n_values, self.scale_bits))
        return Plaintext(poly, self.scale_bits, n_values)

    def decode(self, pt: Plaintext) -> np.ndarray:
        """ckks_encoder.rs:129-131."""
        return self.decode_complex(pt).real

    def decode_complex(self, pt: Plaintext) -> np.ndarray:
        """ckks_encoder.rs:134-156 (one row per poly of a batch object)."""
        B = pt.poly.n_polys
        out = np.zeros((B, pt.slots), dtype=np.complex128)
        check(load().rnt_decode(pt.poly.handle, out.ctypes.data_as(ctypes.c_void_p), pt.slots, pt.scale_bits))
        return out if pt.poly.batched else out[0]


# ---------------------------------------------------------------------------
# limb-sharded building blocks (include/rnsntt.h)
# ---------------------------------------------------------------------------


def ct_tensor(c0: RnsPoly, c1: RnsPoly, c0p: RnsPoly, c1p: RnsPoly,
              d2_out: Optional[RnsPoly] = None) -> tuple[RnsPoly, RnsPoly, RnsPoly]:
    """Tensor product (engine.rs:480-493) on this basis' limbs: d0, d1 in the
    NTT domain (key-switch seeds), d2 in the coefficient domain (written into
    ``d2_out`` when given, e.g. a wrapped collective buffer)."""
    d0, d1 = c0._like(), c0._like()
    d2 = d2_out if d2_out is not None else c0._like()
    check(load().rnt_ct_tensor(d0.handle, d1.handle, d2.handle, c0.handle, c1.handle,
                               c0p.handle, c1p.handle))
    return d0, d1, d2


def keyswitch_ext(src_ptr: int, src_limbs: int, key: RnsGadgetKey, basis: RnsBasis, n_polys: int,
                  init0: Optional[RnsPoly] = None, init1: Optional[RnsPoly] = None,
                  out0: Optional[RnsPoly] = None, out1: Optional[RnsPoly] = None
                  ) -> tuple[RnsPoly, RnsPoly]:
    """Gadget sum (engine.rs:505-528) for this basis' (target) limbs over
    ``src_limbs`` coefficient-domain source limbs at device address
    ``src_ptr`` ([src_limbs][n_polys][N] words); seeds in the NTT domain."""
    acc0 = out0 if out0 is not None else RnsPoly(basis, n_polys)
    acc1 = out1 if out1 is not None else RnsPoly(basis, n_polys)
    check(load().rnt_keyswitch_ext(acc0.handle, acc1.handle, ctypes.c_void_p(src_ptr), src_limbs,
                                   key.a.handle, key.b.handle,
                                   init0.handle if init0 is not None else None,
                                   init1.handle if init1 is not None else None))
    return acc0, acc1


def rescale_ext(x: RnsPoly, last_ptr: int, q_last: int, out_basis: RnsBasis,
                out: Optional[RnsPoly] = None) -> RnsPoly:
    """rescale_into (poly.rs:187-228) by an external last limb: residues mod
    ``q_last`` ([n_polys][N] words, coefficient domain) at ``last_ptr``."""
    o = out if out is not None else x._like(out_basis)
    check(load().rnt_rescale_ext(o.handle, x.handle, ctypes.c_void_p(last_ptr), int(q_last)))
    return o
