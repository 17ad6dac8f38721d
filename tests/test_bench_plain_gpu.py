"""bench.py without --full prints the headline alone; --full adds the blocks measured beside it, after the timed steps."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")
SIDE = ("surface", "kernel_only", "roofline", "cpu_baseline", "grad_rel_l2", "tree_scenes", "c4_strong", "c4_strong_one_integrator")


def run_bench(*extra):
    res, spp = 64, 4
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--res", str(res), "--spp", str(spp)]
                       + list(extra), capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "Mpath-samples/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["ms_per_step"] > 0 and d["config"]["global_spp"] == spp and d["config"]["triangles"] > 0
    # value = the camera sample slots of the two passes per step over the step time
    assert d["value"] == pytest.approx(2.0 * res * res * spp / (d["ms_per_step"] * 1e-3) / 1e6, rel=2e-3)          # both rounded in the line
    return d


@pytest.mark.gpu
def test_plain_run_reports_the_headline_alone():
    d = run_bench()
    assert tuple(d) == HEADLINE, list(d)


@pytest.mark.gpu
def test_full_run_adds_the_side_blocks():
    d = run_bench("--full", "--no-pmc", "--no-cpu-baseline", "--no-tree-scenes", "--no-c4-strong")
    assert tuple(d) == HEADLINE + SIDE, list(d)
    assert d["surface"]["ms_per_step"] == d["ms_per_step"] and d["surface"]["reverse_step_ms"] > 0
    assert d["kernel_only"]["render_c_ms"] > 0 and d["kernel_only"]["render_d_rev_all_ms"] > 0 and d["roofline"]["kernel_ms"] > 0
    assert all(d[k] is None for k in ("cpu_baseline", "grad_rel_l2", "tree_scenes", "c4_strong", "c4_strong_one_integrator"))
