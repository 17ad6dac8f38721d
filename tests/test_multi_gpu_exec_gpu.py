"""The multi-GPU code path EXECUTED on hardware: two processes share the one GPU of the test box (backend gloo,
CUDA tensors), each renders its half of the sample slots through the PUBLIC surface -- renderC, renderD +
enoki.forward, renderD + enoki.backward, preprocess_secondary_edges -- and the collectives inside
psdr_cuda/integrator.py (one all-reduce of [image || derivative images] or of the flat gradient buffer per render call,
one of the guiding mass) must reproduce the single-process result up to the order of the fp32 sums.

(8-GPU runs over RCCL are the driver's; on one GPU `nccl` cannot host two ranks, gloo moves the same buffers.)
"""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_sequence():
    """The call sequence under test; returns a dict of numpy arrays.  Runs in every rank and in the single process."""
    import torch
    import enoki as ek
    import psdr_cuda
    from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD, Matrix4f as Matrix4fD
    from psdr_cuda.fixtures import scene_path
    out = {}

    def scene(name, spp, sppe, sppse, res=48):
        sc = psdr_cuda.Scene()
        sc.load_file(scene_path(name), False)
        sc.opts.width = sc.opts.height = res
        sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
        return sc
    # renderC, PathTracer (odd spp: the shards are 4 + 3 samples)
    sc = scene("cbox", 7, 0, 0)
    sc.configure()
    out["c_path"] = psdr_cuda.PathTracer(3).renderC(sc).numpy()
    out["c_direct_second_pass"] = psdr_cuda.DirectIntegrator(2, 1).renderC(sc).numpy()       # RNG offsets advanced on every rank alike
    # renderD + forward, all three terms
    sc = scene("cbox_occluder", 6, 5, 7)
    P = FloatD(0.)
    ek.set_requires_gradient(P)
    sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD([1.0, 0.5, 0.0]) * P))
    sc.configure()
    integ = psdr_cuda.DirectIntegrator(1, 1)
    img = integ.renderD(sc, 0)
    ek.forward(P, free_graph=True)
    out["d_fwd_img"], out["d_fwd_grad"] = img.numpy(), ek.gradient(img).numpy()
    # guiding grid, then a guided renderD
    w = integ.preprocess_secondary_edges(sc, 0, np.array([64, 4, 4, 2]), 2)
    out["guide_cmf"] = w.m_distrb.m_cmf.cpu().numpy()
    # renderD + backward: albedo texels and vertex positions
    sc = scene("cbox", 6, 4, 4)
    refl = sc.param_map["BSDF[0]"].reflectance
    ek.set_requires_gradient(refl.data)
    mesh = sc.param_map["Mesh[0]"]
    v = Vector3fD(ek.detach(mesh.vertex_positions))
    ek.set_requires_gradient(v)
    mesh.vertex_positions = v
    sc.configure()
    img = psdr_cuda.DirectIntegrator(1, 1).renderD(sc, 0)
    wgt = torch.linspace(0.5, 1.5, img.t.numel(), device=img.t.device).reshape(img.t.shape)
    ek.backward(FloatD._wrap((wgt * (img.t - 0.3) ** 2).sum().reshape(1)))
    out["d_rev_img"] = img.numpy()
    out["g_refl"], out["g_vert"] = ek.gradient(refl.data).numpy(), ek.gradient(v).numpy()
    # round 5, PathTracer on a two-level scene at a size where the library picks its wavefront launches by itself (2^20 slots per rank at two ranks):
    # geometry tangents through the traced wavefront with dual-number stages, then renderD + backward whose reverse call reuses the primal render's records
    sc = scene("cbox_bunny", 32, 0, 0, res=256)
    P = FloatD(0.)
    ek.set_requires_gradient(P)
    sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD([0.5, 1.0, 0.0]) * P))
    sc.configure()
    pt = psdr_cuda.PathTracer(3)
    img = pt.renderD(sc, 0)
    ek.forward(P, free_graph=True)
    out["pt_fwd_img"], out["pt_fwd_grad"] = img.numpy(), ek.gradient(img).numpy()
    sc = scene("cbox_bunny", 32, 0, 0, res=256)
    mesh = sc.param_map["Mesh[1]"]
    v = Vector3fD(ek.detach(mesh.vertex_positions))
    ek.set_requires_gradient(v)
    mesh.vertex_positions = v
    sc.configure()
    img = pt.renderD(sc, 0)
    ek.backward(FloatD._wrap((img.t * img.t).sum().reshape(1)))
    out["pt_rev_img"], out["pt_g_vert"] = img.numpy(), ek.gradient(v).numpy()
    out["pt_rev_rays"] = np.array([pt.last_counters[0]])               # 0: the reverse call ran its adjoint kernel only (PSDR_FLAG_KEEP_RECORDS)
    return out


def main():
    """Entry point of one rank (python tests/test_multi_gpu_exec_gpu.py <out.npz>, started by run_ranks)."""
    for p in ("psdr-cuda_amd", "tests"):
        sys.path.insert(0, os.path.join(ROOT, p))
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)                       # both ranks on the one GPU
    dist.init_process_group("gloo")
    out = run_sequence()
    out["world"] = np.array([dist.get_world_size()])
    if dist.get_rank() == 0:
        np.savez(sys.argv[1], **out)
    dist.barrier()
    dist.destroy_process_group()


def run_ranks(world, argv, env, tmp_path, timeout):
    """`world` processes of `python argv` sharing the one GPU, started with the environment torch.distributed.run gives its workers (RANK, WORLD_SIZE,
    MASTER_ADDR / MASTER_PORT, ...) but without the launcher's agent process, which opens the GPU as well.  No test of this suite keeps the GPU open in
    more than six processes at once, the pytest process being one of them: five ranks at most.  A rank that fails ends the others.  Returns (exit codes,
    every rank's stdout, the tails of the ranks' stderr)."""
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs, logs = [], []
    for rank in range(world):
        e = dict(env, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), GROUP_RANK="0", WORLD_SIZE=str(world),
                 LOCAL_WORLD_SIZE=str(world))
        out, err = open(tmp_path / ("rank%d.out" % rank), "w+"), open(tmp_path / ("rank%d.err" % rank), "w+")
        logs.append((out, err))
        procs.append(subprocess.Popen([sys.executable] + argv, env=e, stdout=out, stderr=err, cwd=ROOT))
    deadline = time.time() + timeout
    while any(p.poll() is None for p in procs):
        if time.time() > deadline or any(p.returncode not in (None, 0) for p in procs):
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(1)
    codes = [p.wait() for p in procs]
    text = []
    for out, err in logs:
        out.seek(0); err.seek(0)
        text.append((out.read(), err.read()))
        out.close(); err.close()
    return codes, [o for o, _ in text], "".join("--- rank %d\n%s" % (i, e[-2000:]) for i, (_, e) in enumerate(text))


@pytest.mark.parametrize("world", [2, 5])
def test_two_ranks_on_one_gpu_reproduce_the_single_process_results(tmp_path, world):
    """world = 5: the most ranks one GPU hosts in this suite (run_ranks); with 7 / 6 / 5 / 4 samples per pixel most ranks hold ONE sample and one holds NONE (an empty shard must launch nothing and still enter every collective)."""
    from helpers import rel_l2
    path = str(tmp_path / "ranks.npz")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    codes, stdout, stderr = run_ranks(world, [os.path.abspath(__file__), path], env, tmp_path, timeout=900)
    assert codes == [0] * world, (codes, stdout[0][-2000:], stderr)
    got = np.load(path)
    assert int(got["world"][0]) == world
    ref = run_sequence()
    for k, v in ref.items():
        assert got[k].shape == v.shape, k
        if k == "pt_rev_rays":
            continue
        tol = 1e-4 if k.startswith("g_") or k in ("pt_fwd_grad", "pt_g_vert") else 2e-5          # same samples, different grouping of the fp32 sums / atomics (3e-7 between two runs of one process since the table chain is reproducible: tests/test_tables_native_gpu.py)
        if world > 2 and k == "pt_g_vert":
            # beyond two ranks a rank's shard can fall below the size from which the library runs the PathTracer's value sweep as the traced wavefront: the ranks run the
            # fused kernels, the single process the wavefront -- separately compiled fp32 tree walks, a handful of samples resolve an epsilon tie the other way and ONE
            # such sample moves a bunny vertex' gradient by per cents (tests/test_gpu_parity.py test_wavefront_and_fused_agree_on_tree_scenes...): 5.7e-3 measured at
            # eight ranks (2^18 slots per shard)
            tol = 2e-2
        assert rel_l2(got[k], v) < tol, (k, rel_l2(got[k], v))
    assert np.abs(ref["d_fwd_grad"]).max() > 0 and np.abs(ref["g_vert"]).max() > 0 and np.abs(ref["g_refl"]).min() > 0
    assert np.abs(ref["pt_fwd_grad"]).max() > 0 and np.abs(ref["pt_g_vert"]).max() > 0
    # one process and each of two ranks: the reverse call reused the primal render's records (at eight ranks a shard is 2^18 slots: below the size from which the
    # library splits the reverse launch, nothing is kept -- and nothing needs to be)
    assert int(ref["pt_rev_rays"][0]) == 0 and (world != 2 or int(got["pt_rev_rays"][0]) == 0)


if __name__ == "__main__":
    main()


def test_bench_multi_rank_path_executes_on_one_gpu():
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank), with the developer switch
    PSDR_BENCH_ONE_GPU=1: both ranks on cuda:0 over gloo.  Not a measurement -- it EXECUTES the script's multi-rank code: sharded spp, the
    (deferred) image all-reduce of renderC, the [image || derivative image] all-reduce, the max-over-ranks clock, rank 0's JSON line."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PSDR_BENCH_ONE_GPU="1")
    port = 29700 + os.getpid() % 1000
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-pmc",
                        "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                       # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and d["config"]["global_spp"] == 128
    assert d["value"] > 0 and d["config"]["allreduce_bytes_per_step"] == 3 * 512 * 512 * 3 * 4


def test_bench_at_five_ranks_on_one_gpu(tmp_path):
    """The driver's multi-GPU command line (`torch.distributed.run --nproc-per-node N bench.py --gpus N`) executed BEFORE the GPUs exist: PSDR_BENCH_ONE_GPU=1 puts the
    five ranks (the most one GPU hosts in this suite: run_ranks) on cuda:0 over gloo.  Not a measurement.  Checked: rank 0 alone prints one line; the headline's weak
    scaling (64 spp per rank: global 320, one all-reduce of [image] and one of [image || derivative image] per step); BASELINE configs[3] as the strong-scaling block at
    world size 5 (global 512 spp over five ranks: uneven shards, the three all-reduces' byte count, finite gradients) in both forms."""
    import json
    world = 5
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PSDR_BENCH_ONE_GPU="1")
    codes, stdout, stderr = run_ranks(world, [os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "2", "--warmup", "1", "--full", "--no-pmc",
                                              "--no-cpu-baseline", "--no-tree-scenes"], env, tmp_path, timeout=1800)
    assert codes == [0] * world, (codes, stdout[0][-2000:], stderr)
    lines = [[l for l in out.splitlines() if l.startswith("{")] for out in stdout]
    assert len(lines[0]) == 1 and not any(lines[1:]), stdout[0][-2000:]
    d = json.loads(lines[0][0])
    assert d["n_gpus"] == world and d["config"]["world_size"] == world and d["config"]["global_spp"] == 64 * world and d["scaling"] == "weak"
    assert d["value"] > 0 and d["config"]["allreduce_bytes_per_step"] == 3 * 512 * 512 * 3 * 4 and len(d["config"]["devices"]) == world
    for key in ("c4_strong", "c4_strong_one_integrator"):
        c4 = d[key]
        assert "error" not in c4, c4
        assert c4["world_size"] == world and c4["global_spp"] == 512 and c4["scaling"] == "strong" and c4["steps"] == 5 and c4["ms_per_step"] > 0 and c4["grad_finite"]
        assert c4["allreduce_bytes_per_step"] >= 2 * 1024 * 1024 * 3 * 4 + c4["triangles"] * 24 * 4          # two images + the triangle-row gradients (+ the texels)
