"""Idle blocks of the device block cache outlive the context whose stream they
were last used on.  When that context goes, its stream is destroyed; a block
must then carry no event recorded on it, because the next taker waits for the
block's event -- on its stream, or on the host while a graph is being recorded
-- and the runtime consults the event's stream for that (pool_forget_stream in
rnt_api.cpp drops those events once the stream is synchronised)."""
from __future__ import annotations

import gc

import numpy as np
import pytest

import pyoracle as orc

pytestmark = pytest.mark.gpu


def test_blocks_of_a_destroyed_context_serve_another_one_and_its_recording(gpu):
    rn = gpu
    rn.pool_trim()  # the cache holds only what this test leaves in it
    n, L, B = 1 << 12, 3, 2
    mod = rn.generate_primes(31, L, n)
    x_h = orc.uniform_poly(mod, n, np.random.default_rng(71), batch=B)
    gone = rn.RnsBasis(mod, n)
    for _ in range(4):  # data blocks of [L][B][N] words, freed behind events on gone's stream
        p = rn.RnsPoly.from_channels(x_h, gone)
        p.to_ntt_domain()
        del p
    del gone
    gc.collect()  # the context and its stream are destroyed; the blocks stay idle in the cache
    live = rn.RnsBasis(mod, n)
    x = rn.RnsPoly.from_channels(x_h, live)  # takes such a block on another stream
    y = x.clone()
    assert np.array_equal(y.channels(), x_h)
    out = rn.RnsPoly(live, B)
    with live.capture() as g:  # a buffer allocated while recording takes one too: the wait is a host wait
        t = x.clone()
        rn.check(rn.load().rnt_add(out.handle, t.handle, x.handle))
    g.replay()
    live.sync()
    Bo = orc.Basis(mod, n)
    assert np.array_equal(out.channels(), np.stack([orc.add(Bo, x_h[b], x_h[b]) for b in range(B)]))
