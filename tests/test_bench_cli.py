"""bench.py's command line: a plain run leaves out what --full adds, and
--dump-outputs writes a bounded, reproducible sample of the timed output.
The option handling and the sampling run on the CPU; one GPU test runs the
benchmark itself at a tiny shape and checks the dumped product against the
oracle."""
from __future__ import annotations

import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402  (conftest puts the repository root on sys.path)


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_switches_the_extras_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_cpu_baseline and a.no_power and a.no_live_pmc
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_cpu_baseline or a.no_power or a.no_live_pmc)
    a = _parse(monkeypatch, "--full", "--no-power")
    assert a.no_power and not a.no_cpu_baseline and not a.no_live_pmc


def _dump(tmp_path, name, outputs, world=1, rank=0, wide=False):
    d = tmp_path / name
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=str(d)), rank, world, outputs, wide=wide)
    return {f: np.load(d / f) for f in sorted(os.listdir(d))}


def test_dump_outputs_sample_is_bounded_and_reproducible(tmp_path, monkeypatch):
    rng = np.random.default_rng(1)
    L, n, count = 3, 64, 37
    data = rng.integers(0, 1 << 31, size=(count, L, n), dtype=np.uint64)
    one = L * n * 8
    monkeypatch.setattr(bench, "DUMP_BUDGET", 5 * one + 17)  # room for five polys, not six
    got = _dump(tmp_path, "a", [("c", count, lambda i: data[i])])
    again = _dump(tmp_path, "b", [("c", count, lambda i: data[i])])
    assert list(got) == ["c.npy"] and got["c.npy"].dtype == np.float64
    assert got["c.npy"].shape == (5, L, n) and np.array_equal(got["c.npy"], again["c.npy"])
    # the sample holds the first and the last poly, in batch order, exactly
    rows = [int(np.flatnonzero((data == got["c.npy"][k].astype(np.uint64)).all(axis=(1, 2)))[0]) for k in range(5)]
    assert rows == sorted(rows) and rows[0] == 0 and rows[-1] == count - 1
    # two outputs share the budget and take the same polys; a batch of one
    two = _dump(tmp_path, "c", [("c0", count, lambda i: data[i]), ("c1", count, lambda i: data[i])])
    assert two["c0.npy"].shape == (2, L, n) and np.array_equal(two["c0.npy"], two["c1.npy"])
    assert _dump(tmp_path, "d", [("c", 1, lambda i: data[i])])["c.npy"].shape == (1, L, n)
    # one poly larger than the budget: its leading limbs only
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * n * 8 + 5)
    assert np.array_equal(_dump(tmp_path, "e", [("c", count, lambda i: data[i])])["c.npy"], data[:1, :2])


def test_dump_outputs_wide_complex_and_ranks(tmp_path):
    rng = np.random.default_rng(2)
    wide = rng.integers(1 << 61, 1 << 62, size=(2, 2, 16), dtype=np.uint64)
    got = _dump(tmp_path, "w", [("c", 2, lambda i: wide[i])], wide=True)
    assert sorted(got) == ["c_hi.npy", "c_lo.npy"]
    back = (got["c_hi.npy"].astype(np.uint64) << np.uint64(31)) | got["c_lo.npy"].astype(np.uint64)
    assert np.array_equal(back, wide)
    z = rng.normal(size=(3, 8)) + 1j * rng.normal(size=(3, 8))
    got = _dump(tmp_path, "z", [("slots", 3, lambda i: z[i])], world=2, rank=1)
    assert sorted(got) == ["slots_im_rank1.npy", "slots_re_rank1.npy"]
    assert np.array_equal(got["slots_re_rank1.npy"] + 1j * got["slots_im_rank1.npy"], z)
    # no directory given: nothing is written
    bench.dump_outputs(types.SimpleNamespace(dump_outputs=None), 0, 1, [("c", 2, lambda i: wide[i])])
    assert sorted(os.listdir(tmp_path)) == ["w", "z"]


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_timed_product(gpu, tmp_path):
    """A plain run at a tiny ring with seeded host operands: the line's
    headline fields, the extras' fields null, and c.npy (the whole batch
    here) bit-exact against the oracle's product of the same operands."""
    import pyoracle as orc

    rn = gpu
    log_n, L, batch, steps, warmup = 12, 3, 5, 3, 1
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--log-n", str(log_n), "--limbs", str(L), "--batch", str(batch),
                        "--inputs", "host", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert (line["steps"], line["warmup"], line["unit"], line["dtype"]) == (steps, warmup, "poly-muls/s", "u32")
    assert line["higher_is_better"] is True and line["metric"] == bench.METRIC
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(batch / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None and line["power"] is None
    assert line["config"]["parity_spot_check"] is None and line["roofline"]["stream_copy_GBs"] is None
    assert line["roofline"]["traffic_live"] is None
    launches = sum(k["launches"] for k in line["roofline"]["kernels"].values())
    assert launches % steps == 0 and launches >= steps  # the timed region ran `steps` products
    n = 1 << log_n
    mod = rn.generate_primes(31, L, n)
    rng = np.random.default_rng(1234)
    a, b = bench.uniform(rng, mod, batch, n), bench.uniform(rng, mod, batch, n)
    Bo = orc.Basis(mod, n)
    got = np.load(tmp_path / "out" / "c.npy")
    assert got.dtype == np.float64 and got.shape == (batch, L, n)
    for i in range(batch):
        assert np.array_equal(got[i].astype(np.uint64), orc.mul(Bo, a[i], b[i])), i
