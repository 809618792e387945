"""bench.dump_outputs (--dump-outputs) on host tensors: dtypes, the shared
byte budget and the fixed sample of an array over its share."""
import os

import numpy as np
import torch


def test_dump_outputs_dtypes_budget_and_fixed_sample(tmp_path, monkeypatch):
    # bench.py sets process-wide defaults for its own runs when imported: pin
    # both variables first, so the session's environment is as before afterwards
    for k in ("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "EXO_BURST_PREFETCH"):
        monkeypatch.setenv(k, os.environ.get(k, "0"))
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4000)  # 4,000 bytes per array
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    t = {"big": big, "f64": torch.linspace(0, 1, 7, dtype=torch.float64), "u8": torch.tensor([0, 1, 1], dtype=torch.uint8)}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), t)
    bench.dump_outputs(str(b), t)
    assert sorted(os.listdir(a)) == ["big.npy", "f64.npy", "u8.npy"]
    f64, u8, s = np.load(a / "f64.npy"), np.load(a / "u8.npy"), np.load(a / "big.npy")
    assert f64.dtype == np.float64 and np.array_equal(f64, t["f64"].numpy())
    assert u8.dtype == np.float32 and u8.tolist() == [0.0, 1.0, 1.0]
    # over its share: 1,000 distinct elements of the flattened array, in index order, the same every time
    assert s.dtype == np.float32 and s.shape == (1000,)
    assert np.all(np.diff(s) > 0) and set(s.tolist()) <= set(range(5000))
    assert np.array_equal(s, np.load(b / "big.npy"))
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 3 * 4000 + 3 * 128  # + the .npy headers
