"""CPU-only: bench.py --dump-outputs writes float32 .npy files; an array larger than DUMP_MAX_ELEMS is written as a fixed
sample of its elements (the same positions in every run, so two builds can be compared array by array)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def test_dump_outputs_small_whole_large_sampled(tmp_path):
    n = bench.DUMP_MAX_ELEMS
    small = torch.arange(6, dtype=torch.float64).view(2, 3)
    big = torch.arange(n + 1000, dtype=torch.float32)          # element value = its flat position
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (2, 3) and (s == small.numpy()).all()
    g = np.load(tmp_path / "a" / "big.npy")
    assert g.dtype == np.float32 and g.shape == (n,)
    assert (np.diff(g) >= 0).all() and g[0] >= 0 and g[-1] < n + 1000     # sorted positions inside the array
    assert len(np.unique(g)) > n // 2                                      # spread over it, not one position repeated
    assert (g == np.load(tmp_path / "b" / "big.npy")).all()
