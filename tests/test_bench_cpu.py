"""bench.py --dump-outputs, the writer alone (no GPU): what the last timed step computed goes to <name>.npy in float32 / float64, and past
the size limit every array keeps the same seeded sample of its elements on every run."""
import numpy as np
import torch

import bench


def test_dump_outputs_writes_float32_and_float64(tmp_path):
    bench.dump_outputs(str(tmp_path), {"segs": torch.arange(6, dtype=torch.bfloat16).reshape(2, 3),
                                       "ids": np.arange(4, dtype=np.int64), "pose": torch.ones(3, 4, dtype=torch.float64)})
    segs, ids, pose = (np.load(tmp_path / f"{k}.npy") for k in ("segs", "ids", "pose"))
    assert segs.dtype == np.float32 and np.array_equal(segs, np.arange(6, dtype=np.float32).reshape(2, 3))
    assert ids.dtype == np.float64 and np.array_equal(ids, np.arange(4))
    assert pose.dtype == np.float64 and pose.shape == (3, 4)


def test_dump_outputs_past_the_limit_is_the_same_seeded_sample_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    arrays = {"a": np.arange(3000, dtype=np.float32).reshape(30, 100), "b": np.arange(1000, dtype=np.float64)}
    for run in ("one", "two"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    got = {run: {k: np.load(tmp_path / run / f"{k}.npy") for k in arrays} for run in ("one", "two")}
    assert sum(v.nbytes for v in got["one"].values()) <= 4000
    for k, full in arrays.items():
        a = got["one"][k]
        assert a.size == full.size // 5 and np.array_equal(a, got["two"][k])
        assert np.isin(a, full).all() and (np.diff(a) > 0).all()          # distinct elements, in their original order
