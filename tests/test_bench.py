"""bench.py's plain run and --dump-outputs.  CPU part: the dump's size cap.  GPU part: a plain run times exactly --steps steps, leaves
the --full figures out and writes the same samples from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT


def test_dump_outputs_caps_size_with_a_fixed_sample_subset(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(3)
    pos, logits = torch.randn(40, 7, 3, generator=g), torch.randn(40, 7, 21, generator=g, dtype=torch.float64)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 10 * 7 * 24 * 4)          # room for 10 of the 40 samples
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), positions=pos, logits=logits)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("positions", "logits")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("positions", "logits")}
    assert a["positions"].dtype == np.float32 and a["logits"].dtype == np.float32
    assert a["positions"].shape == (10, 7, 3) and a["logits"].shape == (10, 7, 21)
    assert all(np.array_equal(a[n], b[n]) for n in a)
    # the same samples in both arrays, in their original order
    rows = [int(np.flatnonzero((pos.float().numpy() == r).all(axis=(1, 2)))[0]) for r in a["positions"]]
    assert rows == sorted(rows)
    assert np.array_equal(a["logits"], logits.float().numpy()[rows])
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 64 << 20)
    bench.dump_outputs(str(tmp_path / "c"), positions=pos, logits=logits)
    assert np.array_equal(np.load(tmp_path / "c" / "positions.npy"), pos.numpy())


def _plain_run(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(out_dir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    return json.loads([ln for ln in out.stdout.decode().splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_bench_dumps_reproducible_outputs(tmp_path):
    lines = [_plain_run(tmp_path / d) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["roofline"] is None and line["cpu_baseline"] is None and line["config"]["outputs_finite"] is True
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("positions", "logits")}
    assert a["positions"].shape == (1, 320, 3) and a["logits"].shape == (1, 320, 21)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy")), n
