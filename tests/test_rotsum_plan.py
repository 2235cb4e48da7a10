"""rotsum_plan (rns_ntt/rotsum.py): the stages of an inner sum over slots, a
pure host function."""
from __future__ import annotations

import pytest

from rns_ntt.rotsum import rotsum_plan


def test_radix_two():
    p = rotsum_plan(64, 1, 2)
    assert p.n == 64 and p.stride == 1 and p.radices == [2] * 6
    assert p.stages == [[0, 1], [0, 2], [0, 4], [0, 8], [0, 16], [0, 32]]
    assert p.all_steps == [1, 2, 4, 8, 16, 32]
    assert rotsum_plan(64).stages == rotsum_plan(64, 1, 4).stages  # the default radix is the measured 4


def test_radix_eight():
    p = rotsum_plan(64, 1, 8)
    assert p.radices == [8, 8]
    assert p.stages == [list(range(8)), [8 * t for t in range(8)]]
    assert p.all_steps == list(range(1, 8)) + [8 * t for t in range(1, 8)]


def test_stride():
    p = rotsum_plan(64, 4, 4)
    assert p.radices == [4, 4, 4]
    assert p.stages == [[0, 4, 8, 12], [0, 16, 32, 48], [0, 64, 128, 192]]
    assert p.stride == 4


def test_mixed_last_factor():
    p = rotsum_plan(32, 1, 8)
    assert p.radices == [8, 4]  # the smallest factor last
    assert p.stages == [list(range(8)), [0, 8, 16, 24]]
    assert rotsum_plan(8, 1, 16).stages == [list(range(8))]  # a radix above n: one stage


def test_given_radices():
    p = rotsum_plan(12, radices=(4, 3))
    assert p.n == 12 and p.radices == [4, 3]
    assert p.stages == [[0, 1, 2, 3], [0, 4, 8]]
    assert p.all_steps == [1, 2, 3, 4, 8]
    q = rotsum_plan(12, 2, radices=(3, 4))
    assert q.stages == [[0, 2, 4], [0, 6, 12, 18]]


@pytest.mark.parametrize("args,kw", [((64, 1, 2), {}), ((64, 1, 8), {}), ((64, 4, 4), {}), ((32, 1, 8), {}),
                                     ((12,), {"radices": (4, 3)}), ((12, 5), {"radices": (3, 2, 2)}),
                                     ((16, 4, 16), {})])
def test_every_offset_is_reached_exactly_once(args, kw):
    p = rotsum_plan(*args, **kw)
    assert sorted(p.offsets()) == [t * p.stride for t in range(p.n)]
    assert all(st[0] == 0 for st in p.stages)
    assert p.all_steps == sorted({s for st in p.stages for s in st if s})


def test_rejections():
    for bad in ((1,), (0,), (-4,)):
        with pytest.raises(ValueError, match="at least 2"):
            rotsum_plan(*bad)
    with pytest.raises(ValueError, match="radix"):
        rotsum_plan(8, 1, 1)
    with pytest.raises(ValueError, match="radix"):
        rotsum_plan(8, 1, 3)  # no power of two
    with pytest.raises(ValueError, match="radices"):
        rotsum_plan(12)  # no power of two and no factors given
    with pytest.raises(ValueError, match="at least 2"):
        rotsum_plan(4, radices=(4, 1))
    with pytest.raises(ValueError, match="multiply"):
        rotsum_plan(12, radices=(4, 4))
    with pytest.raises(ValueError, match="stride"):
        rotsum_plan(4, 0)
    # steps of N/2 or more: N = 1024 has 512 slots
    assert rotsum_plan(512, 1, 2, n_slots=512).stages[-1] == [0, 256]
    with pytest.raises(ValueError, match="slots"):
        rotsum_plan(1024, 1, 2, n_slots=512)
    with pytest.raises(ValueError, match="slots"):
        rotsum_plan(16, 64, 4, n_slots=512)
