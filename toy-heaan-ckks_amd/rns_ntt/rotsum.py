"""The plan of an inner sum over slots (rotate-and-sum): a pure host function
(DESIGN.md §4 "Rotate-and-sum").

``sum_{t < n} rot(ct, t stride)`` with ``n = r_0 r_1 ... r_{s-1}`` factors into
``s`` stages: stage ``u`` replaces the ciphertext by the sum of its rotations by

    0, m_u stride, 2 m_u stride, ..., (r_u - 1) m_u stride,    m_u = r_0 ... r_{u-1}

because every ``t < n`` is ``t_0 + t_1 m_1 + ... `` with ``t_u < r_u`` exactly
once (mixed radix).  Each stage is one ``rotsum_ciphertext_hybrid`` call
(rnt_ct_rotsum_hybrid): one ModUp, ``r_u - 1`` key streams, two ModDowns.

The trade-off the caller controls with the radix: radix 2 needs ``log2 n`` keys
and ``log2 n`` ModUps; radix ``r`` needs ``(r - 1) log_r n`` keys and ``log_r n``
ModUps.  A key is ``2 beta (Lv + K)`` planes -- 72 MiB at 2^16 x (16 + 2) limbs,
alpha = 2, 32-bit words -- and every rotating step of a stage streams one.
Measured at that ring (profiles/rotsum_bench.jsonl): radix
4 is ahead of radix 2 at every batch size and every n measured (1.25 to 1.48 x),
radix 8 is the fastest at n = 8 and at one ciphertext, radix 4 from n = 64 on at
8 and 64 ciphertexts; radix 16 is never the best.  Hence the default radix 4,
at 1.5 x the keys of radix 2.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Sequence

__all__ = ["RotsumPlan", "rotsum_plan"]


@dataclass
class RotsumPlan:
    n: int                                        # the slots summed
    stride: int                                   # the distance between them
    radices: list = field(default_factory=list)   # r_u, their product is n
    stages: list = field(default_factory=list)    # per stage its steps, the leading 0 included
    all_steps: list = field(default_factory=list) # the nonzero steps: the keys the plan needs

    def offsets(self) -> list:
        """Every slot offset the stages reach, with multiplicity: the sums of
        one step per stage.  It is ``[t stride for t < n]`` up to order."""
        out = [0]
        for st in self.stages:
            out = [o + s for o in out for s in st]
        return out


def rotsum_plan(n: int, stride: int = 1, radix: int = 4, radices: Optional[Sequence[int]] = None,
                n_slots: Optional[int] = None) -> RotsumPlan:
    """The stages of ``sum_{t < n} rot(., t stride)``.  ``radices`` gives the
    factors of ``n`` in stage order; without it ``n`` must be a power of two
    and is split into factors of ``radix`` (a power of two), the smallest
    factor last.  ``n_slots`` (N/2 of the ring): no step may reach it."""
    n, stride = int(n), int(stride)
    if n < 2:
        raise ValueError("rotsum_plan: n must be at least 2")
    if stride < 1:
        raise ValueError("rotsum_plan: the stride must be at least 1")
    if radices is None:
        radix = int(radix)
        if radix < 2 or radix & (radix - 1):
            raise ValueError("rotsum_plan: the radix must be a power of two, at least 2")
        if n & (n - 1):
            raise ValueError("rotsum_plan: n is no power of two; give its factors in `radices`")
        radices, left = [], n
        while left > 1:
            radices.append(min(radix, left))
            left //= radices[-1]
    else:
        radices = [int(r) for r in radices]
        if not radices or any(r < 2 for r in radices):
            raise ValueError("rotsum_plan: every radix must be at least 2")
        prod = 1
        for r in radices:
            prod *= r
        if prod != n:
            raise ValueError(f"rotsum_plan: the radices multiply to {prod}, not n = {n}")
    stages, m = [], 1
    for r in radices:
        stages.append([t * m * stride for t in range(r)])
        m *= r
    if n_slots is not None and stages[-1][-1] >= int(n_slots):
        raise ValueError(f"rotsum_plan: a step of {stages[-1][-1]} reaches the ring's {int(n_slots)} slots")
    all_steps = sorted({s for st in stages for s in st if s != 0})
    return RotsumPlan(n, stride, list(radices), stages, all_steps)
