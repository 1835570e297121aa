"""bench.py's command line on a box WITHOUT a GPU: the self-launching N-rank form must refuse, with a message and a non-zero
exit code, before it starts a single rank."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_2_without_two_devices_fails_loudly():
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this node has two GPUs: the refusal cannot be provoked")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PC_FORCE_DEVICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert "--gpus 2 needs 2 visible GPUs" in r.stderr and not r.stdout.strip()


def test_dump_outputs_writes_float_arrays_and_samples_past_the_cap(tmp_path):
    """--dump-outputs' writer: one <name>.npy per array, float32 / float64 by source dtype; past the byte cap an array over
    its share becomes a fixed seeded sample (the same elements in every run)."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    outs = {"loss": torch.tensor(0.25), "w": torch.arange(12.0).reshape(3, 4), "n": torch.tensor(7), "d": torch.ones(2, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), outs)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in outs}
    assert got["loss"].dtype == np.float32 and got["loss"].tolist() == [0.25]
    assert got["w"].dtype == np.float32 and np.array_equal(got["w"], np.arange(12.0).reshape(3, 4))
    assert got["n"].dtype == np.float64 and got["n"].tolist() == [7.0] and got["d"].dtype == np.float64
    big = {"a": torch.arange(1000.0), "b": torch.arange(10.0)}
    for sub in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / sub), big, cap=2000)
    a1, a2 = np.load(tmp_path / "s1" / "a.npy"), np.load(tmp_path / "s2" / "a.npy")
    assert a1.size == 250 and np.array_equal(a1, a2) and np.all(np.diff(a1) > 0)
    assert np.array_equal(np.load(tmp_path / "s1" / "b.npy"), np.arange(10.0, dtype=np.float32))
