"""bench.py --dump-outputs DIR: what the timed path returned in its last step, as DIR/<name>.npy, so that two builds run with the same
arguments can be compared output for output."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_stays_under_the_limit_with_a_fixed_sample(tmp_path):
    import bench
    big = np.arange(12 << 20, dtype=np.float64)                     # 96 MB: more than the whole limit
    small = np.arange(12, dtype=np.float32).reshape(4, 3)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert a.nbytes == bench.DUMP_LIMIT_BYTES // 2 and np.all(np.diff(a) > 0)           # a sorted sample of distinct elements
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_LIMIT_BYTES + 2 * 128


@pytest.mark.gpu
@pytest.mark.parametrize("config, names", [("c2", ("renderC_image", "renderD_image", "renderD_grad_albedo")),
                                           ("c4", ("renderC_image", "grad_vertex_positions", "grad_albedo"))], ids=["c2", "c4"])
def test_bench_dumps_the_same_outputs_in_two_runs(tmp_path, config, names):
    from helpers import rel_l2
    res = 64
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--gpus", "1", "--steps", "2", "--warmup", "1", "--res", str(res),
                            "--spp", "4", "--no-pmc", "--no-cpu-baseline", "--no-tree-scenes", "--no-c4-strong", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in names)
    for name in names:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape[-1] == 3 and np.isfinite(a).all() and np.abs(a).max() > 0, name
        assert rel_l2(b, a) < 1e-5, (name, rel_l2(b, a))
    assert np.load(tmp_path / "a" / "renderC_image.npy").shape == (res * res, 3)
