"""Forward mode (JVP) of the table chain of Scene::configure on the HIP library: the psdr_geo_*_jvp entries (csrc/psdr_tables.hip) against
torch.func.jvp of each stage's torch formulation (scene.py), in fp32 on the device and against an fp64 evaluation on the host; enoki.forward
on the native path without a single call of a torch formulation; and renderD + enoki.forward end to end against the eager torch chain."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import load_scene, rel_l2, tangents_wrt
from psdr_cuda import _abi, tables_native
from psdr_cuda import scene as scene_mod
from psdr_cuda.fixtures import scene_path
from psdr_cuda.scene import primary_edge_records, process_mesh, secondary_edge_records

pytestmark = pytest.mark.gpu
SCENES = ["cbox_bunny", "bunny_light"]


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc):
    assert rc == 0, _abi.load_hip().psdr_last_error()


def to_world(v, mats, vmesh):
    mv = mats.index_select(0, vmesh)
    h = (mv[:, :3, :3] * v.unsqueeze(1)).sum(-1) + mv[:, :3, 3]
    w = (mv[:, 3, :3] * v).sum(-1) + mv[:, 3, 3]
    return h / w.unsqueeze(-1)


def jvp_refs(f, primals, tangents, index):
    """torch.func.jvp of f(*primals, index) in fp32 on the device and in fp64 on the host"""
    r32 = torch.func.jvp(lambda *p: f(*p, index), tuple(primals), tuple(tangents))[1]
    ic = index.cpu()
    r64 = torch.func.jvp(lambda *p: f(*p, ic), tuple(p.detach().double().cpu() for p in primals), tuple(t.double().cpu() for t in tangents))[1]
    return r32, r64


def assert_close(out, refs, mask=None, label=""):
    r32, r64 = refs
    o, a, b = out.detach().cpu().numpy(), r32.detach().cpu().numpy(), r64.detach().numpy()
    if mask is not None:
        m = mask.cpu().numpy().astype(bool)
        o, a, b = o[m], a[m], b[m]
    assert np.isfinite(o).all(), label
    assert np.abs(b).max() > 0, label
    e32, e64 = rel_l2(o, a), rel_l2(o, b)
    print("%s: rel-L2 %.2e vs fp32 torch, %.2e vs fp64" % (label, e32, e64))
    assert e32 <= 1e-5 and e64 <= 1e-4, (label, e32, e64)


_stage_cache = {}


def stage_inputs(name):
    """the primal inputs of every stage as configure() holds them (native chain), detached"""
    if name in _stage_cache:
        return _stage_cache[name]
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path(name), False)
    sc.opts.width = sc.opts.height = 32
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 1, 1, 1, 0
    sc.configure()
    bt, ms = sc._batch, sc.m_meshes
    tp = bt["tp"]
    mats = torch.bmm(torch.bmm(torch.stack([m._to_world_left for m in ms]), torch.stack([m._to_world_raw for m in ms])), torch.stack([m._to_world_right for m in ms]))
    d = dict(v_raw=torch.cat([m._raw_positions() for m in ms]).detach().float().contiguous(), mats=mats.detach().float().contiguous(),
             vmesh=tp["vmesh"].long(), vmesh_i32=tp["vmesh_i32"], faces=tp["faces"].long(), faces_i32=tp["faces_i32"], edges=tp["edges"].long(),
             edges_i32=tp["edges_i32"], facen=tp["edge_face_normals_u8"], v=bt["v_world"].detach().contiguous(), rows=bt["tri_info"].detach().contiguous(),
             cam22=sc.tables(0)["cam"][32:54].detach().contiguous())
    _stage_cache[name] = d
    return d


def randn(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g)


@pytest.mark.parametrize("name", SCENES)
def test_world_vertices_jvp(name):
    s, lib = stage_inputs(name), _abi.load_hip()
    V, M = s["v_raw"].shape[0], s["mats"].shape[0]
    out = torch.empty_like(s["v_raw"])
    _check(lib.psdr_geo_world_vertices_fwd(V, _p(s["v_raw"]), _p(s["vmesh_i32"]), _p(s["mats"]), _p(out), _stream()))
    tv, tm = randn(V, 3, seed=1), randn(M, 4, 4, seed=2) * 1e-2
    tm[:, 3, :3] *= 1e-3                                           # a projective part, small as it is next to w = 1
    for t_raw, t_mats in ((tv, tm), (tv, None), (None, tm)):
        t_out = torch.full_like(out, float("nan"))
        _check(lib.psdr_geo_world_vertices_jvp(V, _p(s["v_raw"]), _p(s["vmesh_i32"]), _p(s["mats"]), _p(out), _p(t_raw), _p(t_mats), _p(t_out), _stream()))
        zt = lambda t, like: torch.zeros_like(like) if t is None else t
        assert_close(t_out, jvp_refs(to_world, (s["v_raw"], s["mats"]), (zt(t_raw, s["v_raw"]), zt(t_mats, s["mats"])), s["vmesh"]),
                     label="%s world_vertices (%s)" % (name, "v" if t_mats is None else "mats" if t_raw is None else "v + mats"))


@pytest.mark.parametrize("name", SCENES)
def test_tri_rows_jvp(name):
    s, lib = stage_inputs(name), _abi.load_hip()
    v, faces_i32 = s["v"], s["faces_i32"]
    V, T, W = v.shape[0], faces_i32.shape[0], _abi.TRI_STRIDE
    vsum = torch.empty(V, 3, device="cuda")
    rows = torch.empty(T, W, device="cuda")
    _check(lib.psdr_geo_tri_rows_fwd(V, T, _p(v), _p(faces_i32), _p(vsum), _p(rows), W, _stream()))
    tv = randn(V, 3, seed=3)
    t_vsum = torch.empty(V, 3, device="cuda")
    t_rows = torch.full((T, W), float("nan"), device="cuda")
    _check(lib.psdr_geo_tri_rows_jvp(V, T, _p(v), _p(faces_i32), _p(vsum), _p(tv), W, _p(t_vsum), _p(t_rows), _stream()))
    assert float(t_rows[:, 22:].abs().max()) == 0.0                # padding words
    refs = jvp_refs(lambda x, f: process_mesh(x, f)[0], (v,), (tv,), s["faces"])
    assert_close(t_rows[:, :22], refs, label="%s tri_rows" % name)
    # the vertex-normal tangents are summed in double: the same bits from one call to the next
    t2 = torch.empty_like(t_rows)
    _check(lib.psdr_geo_tri_rows_jvp(V, T, _p(v), _p(faces_i32), _p(vsum), _p(tv), W, _p(t_vsum), _p(t2), _stream()))
    assert torch.equal(t2, t_rows)


@pytest.mark.parametrize("name", SCENES)
def test_sec_edges_jvp(name):
    s, lib = stage_inputs(name), _abi.load_hip()
    v, rows, edges_i32 = s["v"], s["rows"], s["edges_i32"]
    E, W = edges_i32.shape[0], rows.shape[1]
    info = torch.empty(E, 16, device="cuda")
    keep = torch.empty(E, dtype=torch.uint8, device="cuda")
    _check(lib.psdr_geo_sec_edges_fwd(E, _p(edges_i32), _p(v), _p(rows), W, _p(info), _p(keep), _stream()))
    tv, tr = randn(*v.shape, seed=4), randn(*rows.shape, seed=5)
    t_info = torch.full((E, 16), float("nan"), device="cuda")
    _check(lib.psdr_geo_sec_edges_jvp(E, _p(edges_i32), _p(tv), _p(tr), W, _p(t_info), _stream()))
    assert_close(t_info, jvp_refs(secondary_edge_records, (v, rows), (tv, tr), s["edges"]), keep.bool(), "%s sec_edges" % name)
    bnd = s["edges"][:, 3] < 0
    if bool(bnd.any()):                                            # boundary edges: zero n1 tangent, like the adjoint
        assert float(t_info[bnd][:, 9:12].abs().max()) == 0.0
    # a null tangent = zero
    t0 = torch.full((E, 16), float("nan"), device="cuda")
    _check(lib.psdr_geo_sec_edges_jvp(E, _p(edges_i32), None, _p(tr), W, _p(t0), _stream()))
    assert float(t0[:, [0, 1, 2, 3, 4, 5, 12, 13, 14, 15]].abs().max()) == 0.0 and torch.equal(t0[:, 6:12], t_info[:, 6:12])


@pytest.mark.parametrize("name", SCENES)
def test_prim_edges_jvp_and_compaction(name):
    s, lib = stage_inputs(name), _abi.load_hip()
    v, rows, edges_i32, cam22 = s["v"], s["rows"], s["edges_i32"], s["cam22"]
    E = edges_i32.shape[0]
    rows8, z4 = torch.empty(E, 8, device="cuda"), torch.empty(E, 4, device="cuda")
    keep = torch.empty(E, dtype=torch.uint8, device="cuda")
    _check(lib.psdr_geo_prim_edges_fwd(E, _p(edges_i32), _p(s["facen"]), _p(v), _p(rows), rows.shape[1], _p(cam22), _p(rows8), _p(z4), _p(keep), _stream()))
    w2s = cam22[:16].reshape(4, 4).contiguous()
    tv, tw = randn(*v.shape, seed=6), randn(4, 4, seed=7) * 1e-3
    t8 = torch.full((E, 8), float("nan"), device="cuda")
    _check(lib.psdr_geo_prim_edges_jvp(E, _p(edges_i32), _p(v), _p(cam22), _p(tv), _p(tw), _p(t8), _stream()))
    assert float(t8[:, 4:].abs().max()) == 0.0                     # edge normal and length: detached end points
    assert_close(t8, jvp_refs(primary_edge_records, (v, w2s), (tv, tw), s["edges"]), keep.bool(), "%s prim_edges" % name)
    # compaction: tangent rows follow their rows, the rows not kept leave nothing behind
    _, _, pos, _, _, hdr = tables_native.compact_edges(rows8, keep, 6, 1)
    n = int(hdr[:1].view(torch.int32))
    assert 0 < n < E
    t_out = torch.full_like(t8, float("nan"))
    _check(lib.psdr_geo_compact_edges_jvp(E, 8, _p(pos), _p(t8), _p(t_out), _stream()))
    assert torch.equal(t_out[:n], t8[keep.bool()]) and float(t_out[n:].abs().max()) == 0.0


def test_degenerate_faces_and_boundary_edges_give_finite_tangents():
    """a face with collinear corners and edges with one face: finite tangents, zero where the primal divides by |c| = 0 (as the adjoint guards)"""
    lib = _abi.load_hip()
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 0, 0], [3, 0, 0]], dtype=torch.float32, device="cuda")
    faces = torch.tensor([[0, 1, 2], [1, 3, 2], [1, 4, 5]], dtype=torch.int32, device="cuda")        # face 2 is degenerate
    V, T, W = 6, 3, _abi.TRI_STRIDE
    vsum, rows = torch.empty(V, 3, device="cuda"), torch.empty(T, W, device="cuda")
    _check(lib.psdr_geo_tri_rows_fwd(V, T, _p(v), _p(faces), _p(vsum), _p(rows), W, _stream()))
    tv = randn(V, 3, seed=8)
    t_vsum, t_rows = torch.empty(V, 3, device="cuda"), torch.empty(T, W, device="cuda")
    _check(lib.psdr_geo_tri_rows_jvp(V, T, _p(v), _p(faces), _p(vsum), _p(tv), W, _p(t_vsum), _p(t_rows), _stream()))
    assert bool(torch.isfinite(t_rows).all())
    assert float(t_rows[2, 18:22].abs().max()) == 0.0
    edges = torch.tensor([[1, 2, 0, 1, 0], [0, 1, 0, -1, 2], [2, 0, 0, -1, 1]], dtype=torch.int32, device="cuda")
    t_info = torch.empty(3, 16, device="cuda")
    _check(lib.psdr_geo_sec_edges_jvp(3, _p(edges), _p(tv), _p(t_rows), W, _p(t_info), _stream()))
    assert bool(torch.isfinite(t_info).all()) and float(t_info[1:, 9:12].abs().max()) == 0.0


def test_forward_mode_never_runs_the_torch_formulation(monkeypatch):
    """enoki.forward on the native chain: every table's tangent comes from the psdr_geo_*_jvp kernels -- a torch formulation that runs raises"""
    sc, P = load_scene("cbox_bunny", res=32, spp=2, sppe=2, sppse=2, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    img = psdr_cuda.DirectIntegrator(1, 1).renderD(sc, 0)

    def boom(*a, **k):
        raise AssertionError("a torch formulation of the table chain ran in forward mode")
    for fn in ("process_mesh", "transform_pos", "secondary_edge_records", "primary_edge_records"):
        monkeypatch.setattr(scene_mod, fn, boom)
    tan = tangents_wrt(tb, P)
    for k in ("tri_info", "sec_edge", "prim_edge"):
        assert tan[k] is not None and bool(torch.isfinite(tan[k]).all()) and float(tan[k].abs().max()) > 0, k
    # and through the renderer
    ek.forward(P, free_graph=True)
    g = ek.gradient(img).numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 0


def _scene_with_parameter(param):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_bunny"), False)
    sc.opts.width = sc.opts.height = 64
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 4, 4, 4, 0
    P = FloatD(0.)
    ek.set_requires_gradient(P)
    if param == "vertex":                                         # every bunny vertex along a smooth field: the normals turn too
        mesh = sc.param_map["Mesh[1]"]
        base = ek.detach(mesh.vertex_positions).t
        field = torch.stack([torch.sin(3.0 * base[:, 1]), torch.cos(2.0 * base[:, 0]), 0.5 * torch.sin(base[:, 2])], dim=-1)
        mesh.vertex_positions = Vector3fD(base + field * P.t.reshape(1, 1))
    else:                                                          # the camera pose: a translation of to_world
        cam = sc.m_sensors[0]
        base = cam._to_world.detach().clone()
        off = torch.zeros(4, 4, device="cuda")
        off[:3, 3] = torch.tensor([0.7, -0.4, 0.3], device="cuda") * P.t.reshape(1)
        cam._to_world = base + off
    sc.configure()
    return sc, P


@pytest.mark.parametrize("param", ["vertex", "camera"])
def test_render_forward_mode_matches_the_torch_chain(param):
    """renderD + enoki.forward on the native chain against the same render node fed the tangents of the eager torch chain (its configure() +
    double backward through the torch formulation), on the same sample streams.  (Two renders of the two configure() formulations differ by
    more than the JVP: the native chain normalises the edge distributions on the device, so a few edge samples land on other edges -- the
    parent tree shows the same difference.)"""
    from enoki._array import _jvp_wrt
    integ = psdr_cuda.DirectIntegrator(1, 1)
    sc, P = _scene_with_parameter(param)
    img = integ.renderD(sc, 0)
    node = img._node
    sc._rng_offset = [0, 0, 0]
    ek.forward(P, free_graph=True)
    g_native = ek.gradient(img).numpy().astype(np.float64)
    with tables_native.torch_formulation():
        sc_t, P_t = _scene_with_parameter(param)
        tan_t = _jvp_wrt(integ.renderD(sc_t, 0)._node.input_tensors(), P_t.t)
    assert (sc.tables(0)["num_sec_edges"], sc.tables(0)["num_prim_edges"]) == (sc_t.tables(0)["num_sec_edges"], sc_t.tables(0)["num_prim_edges"])
    tan = []
    for t, x in zip(tan_t, node.input_tensors()):                  # the native edge tables hold their kept rows first, at candidate capacity
        if t is not None and x is not None and t.shape[0] < x.shape[0]:
            t = torch.cat([t, torch.zeros(x.shape[0] - t.shape[0], *t.shape[1:], dtype=t.dtype, device=t.device)])
        tan.append(t)
    sc._rng_offset = [0, 0, 0]
    g_torch = node.render_forward(tan).detach().cpu().numpy().astype(np.float64)
    err = rel_l2(g_native, g_torch)
    print("%s: derivative image native vs torch-chain tangents rel-L2 %.2e (|g| max %.3g)" % (param, err, np.abs(g_torch).max()))
    assert np.isfinite(g_native).all() and np.abs(g_torch).max() > 0
    assert err <= 1e-5, err
