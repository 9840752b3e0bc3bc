"""bench.py --dump-outputs: the arrays of the last timed call as DIR/<name>.npy in float32 / float64, at most 64 MB in all, and
the same file for the same arguments (a larger output keeps a fixed seeded subset of its rows).  No GPU: CPU tensors stand in
for what the timed path returns."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_output_is_written_whole_in_float32(tmp_path):
    bench = _bench()
    x = torch.randn(8, 3, 4, 4, dtype=torch.float32)
    info = bench.dump_outputs(str(tmp_path / "d"), {"samples": x.to(torch.bfloat16)})
    got = np.load(tmp_path / "d" / "samples.npy")
    assert got.dtype == np.float32 and got.shape == (8, 3, 4, 4)
    assert np.array_equal(got, x.to(torch.bfloat16).float().numpy())
    assert info["samples"] == {"shape": [8, 3, 4, 4], "dtype": "float32", "rows": 8, "of_rows": 8}


def test_large_output_keeps_the_same_seeded_rows_within_the_limit(tmp_path):
    bench = _bench()
    x = torch.randn(512, 3, 32, 32)
    loss = torch.tensor([0.25], dtype=torch.float64)
    limit = 2 * 2 ** 20
    bench.dump_outputs(str(tmp_path / "a"), {"samples": x, "loss": loss}, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), {"samples": x, "loss": loss}, limit=limit)
    a, b = np.load(tmp_path / "a" / "samples.npy"), np.load(tmp_path / "b" / "samples.npy")
    assert np.array_equal(a, b) and 0 < a.shape[0] < 512 and a.shape[1:] == (3, 32, 32)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
    rows = {r.tobytes() for r in x.numpy()}
    assert all(r.tobytes() in rows for r in a), "the subset holds whole rows of the output"
    assert np.load(tmp_path / "a" / "loss.npy").dtype == np.float64


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode != 0 and b"--steps" in r.stderr
