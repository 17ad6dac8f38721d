"""The reference module's bindings (src/psdr.cpp:48-294), name by name, against the package -- and Mesh.shift_vertices / Mesh.dump on the host path.

Every `.def` / `.def_readwrite` / `.def_readonly` name per class is listed inline (constructors and `__repr__` aside); the pair under
PSDR_MESH_ENABLE_1D_VERTEX_OFFSET (vertex_offset, shift_vertices) is a run-time option here and is listed too.  A name is looked up on an
instance where one is cheap to make (fields set in __init__), otherwise on the class.
"""

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from enoki.cuda_autodiff import Float32 as FloatD

from helpers import load_scene

REFERENCE_DEFS = {
    "Object": "type_name id",
    "RenderOption": "width height spp sppe sppse log_level",
    "RayC": "reversed o d",
    "RayD": "reversed o d",
    "FrameC": "s t n",
    "FrameD": "s t n",
    "Bitmap1fD": "load_openexr eval resolution data",
    "Bitmap3fD": "load_openexr eval resolution data",
    "InteractionC": "is_valid wi p t",
    "InteractionD": "is_valid wi p t",
    "IntersectionC": "shape n sh_frame uv J",
    "IntersectionD": "shape n sh_frame uv J",
    "Sampler": "clone seed next_1d next_2d",
    "DiscreteDistribution": "init sample sum pmf",
    "HyperCubeDistribution2f": "set_resolution set_mass sample_reuse pdf cells",
    "HyperCubeDistribution3f": "set_resolution set_mass sample_reuse pdf cells",
    "SampleRecordC": "pdf is_valid",
    "SampleRecordD": "pdf is_valid",
    "PositionSampleC": "p J pdf is_valid",
    "PositionSampleD": "p J pdf is_valid",
    "BSDF": "anisotropic",
    "DiffuseBSDF": "reflectance anisotropic",
    "RoughConductorBSDF": "alpha_u alpha_v eta k specular_reflectance anisotropic",
    "Sensor": "to_world",
    "PerspectiveCamera": "to_world",
    "Emitter": "",
    "AreaLight": "",
    "EnvironmentMap": "to_world set_transform radiance scale",
    "Mesh": "load configure set_transform append_transform sample_position num_vertices num_faces bsdf to_world vertex_positions vertex_normals "
            "vertex_uv face_indices face_uv_indices vertex_offset shift_vertices enable_edges edge_indices dump",
    "Scene": "load_file load_string configure sample_boundary_segment_direct opts num_sensors num_meshes param_map",
    "Integrator": "renderC renderD preprocess_secondary_edges",
    "FieldExtractionIntegrator": "renderC renderD preprocess_secondary_edges",
    "DirectIntegrator": "renderC renderD preprocess_secondary_edges hide_emitters",
}
# The value types the kernels keep internal: the intersection records and the sampler are not classes of the Python surface (COVERAGE.md).
# Listed so that the gap is explicit -- a class that appears, or a new class that goes missing, fails the test below.
NOT_ON_THE_SURFACE = {"InteractionC", "InteractionD", "IntersectionC", "IntersectionD", "Sampler"}

FACTORIES = {
    "Object": lambda: psdr_cuda.Object(),
    "RenderOption": lambda: psdr_cuda.RenderOption(),
    "RayC": lambda: psdr_cuda.RayC(),
    "RayD": lambda: psdr_cuda.RayD(),
    "FrameC": lambda: psdr_cuda.FrameC(),
    "FrameD": lambda: psdr_cuda.FrameD(),
    "Bitmap1fD": lambda: psdr_cuda.Bitmap1fD(),
    "Bitmap3fD": lambda: psdr_cuda.Bitmap3fD(),
    "DiffuseBSDF": lambda: psdr_cuda.DiffuseBSDF(),
    "RoughConductorBSDF": lambda: psdr_cuda.RoughConductorBSDF(),
    "EnvironmentMap": lambda: psdr_cuda.EnvironmentMap(),
    "Mesh": lambda: psdr_cuda.Mesh(),
    "Scene": lambda: psdr_cuda.Scene(),
    "DirectIntegrator": lambda: psdr_cuda.DirectIntegrator(),
}


def test_every_reference_binding_exists_on_the_package():
    absent_classes = {c for c in REFERENCE_DEFS if not hasattr(psdr_cuda, c)}
    assert absent_classes == NOT_ON_THE_SURFACE
    missing = []
    for c, names in REFERENCE_DEFS.items():
        if c in absent_classes:
            continue
        obj = FACTORIES[c]() if c in FACTORIES else getattr(psdr_cuda, c)
        missing += ["%s.%s" % (c, n) for n in names.split() if not hasattr(obj, n)]
    assert missing == []


# ---------------------------------------------------------------------------------------------- Mesh.shift_vertices (mesh.cpp:345-351)
def _bunny_with_offset(seed=0):
    sc, _ = load_scene("cbox_bunny", res=8, spp=1)
    mesh = max(sc.m_meshes, key=lambda m: m.num_vertices)
    g = torch.Generator().manual_seed(seed)
    off = (torch.rand(mesh.num_vertices, generator=g) - 0.5) * 0.2
    mesh.vertex_offset = FloatD._wrap(off.to(mesh._vertex_positions_raw.device))
    sc.configure()
    return sc, mesh


def test_shift_vertices_keeps_the_world_positions_and_zeroes_the_offset():
    sc, mesh = _bunny_with_offset()
    before = mesh._vertex_positions.detach().clone()
    raw_before = mesh._vertex_positions_raw
    mesh.shift_vertices()
    assert not mesh.m_ready
    assert mesh._vertex_positions_raw is not raw_before          # a new tensor: the configure cache sees it
    sc.configure()
    after = mesh._vertex_positions.detach()
    # same expression, same inputs: to an ulp of the position, plus what the normals along which the offset moves a vertex reproduce to
    assert torch.allclose(after, before, rtol=2.0 ** -23, atol=_normal_noise(after) * 0.1)          # (|offset| <= 0.1)
    off = mesh.vertex_offset
    assert torch.count_nonzero(off.t) == 0 and off.t.shape == (mesh.num_vertices,)
    # the zero offset is a stored tensor that can take a gradient again
    ek.set_requires_gradient(off)
    mesh.vertex_offset = off
    sc.configure()
    loss = mesh._vertex_positions.sum()
    loss.backward()
    g = ek.gradient(off).t
    assert g.shape == (mesh.num_vertices,) and torch.isfinite(g).all() and torch.count_nonzero(g) > 0


def test_shift_vertices_without_an_offset_leaves_the_positions():
    sc, _ = load_scene("cbox_occluder", res=8, spp=1)
    mesh = sc.m_meshes[-1]
    raw = mesh._vertex_positions_raw.clone()
    mesh.shift_vertices()
    assert torch.equal(mesh._vertex_positions_raw, raw)
    assert torch.count_nonzero(mesh.vertex_offset.t) == 0


def test_dump_writes_the_offset_vertices_before_and_after_shift_vertices(tmp_path):
    sc, mesh = _bunny_with_offset(1)
    a, b = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
    mesh.dump(a)
    raw_text = ["v %.9g %.9g %.9g" % tuple(p) for p in mesh._vertex_positions_raw.detach().cpu().numpy()]
    off = np.abs(mesh.vertex_offset.t.detach().cpu().numpy())
    mesh.shift_vertices()
    mesh.dump(b)
    ta, tb_ = open(a).read(), open(b).read()
    # %.9g round-trips a float32: to the printed precision the same vertices -- to an ulp, plus the offset times what the normals reproduce
    # to -- and the same faces
    va, vb = _obj_vertices(ta), _obj_vertices(tb_)
    assert np.all(np.abs(va - vb) <= np.spacing(np.maximum(np.abs(va), np.abs(vb))) + off[:, None] * _normal_noise(mesh._vertex_positions_raw))
    assert [l for l in ta.split("\n") if not l.startswith("v ")] == [l for l in tb_.split("\n") if not l.startswith("v ")]
    # the offset moved the vertices: the file is not the raw positions, and after the shift it is the new raw positions
    assert [l for l in ta.split("\n") if l.startswith("v ")] != raw_text
    np.testing.assert_array_equal(vb, mesh._vertex_positions_raw.detach().cpu().numpy())


def _normal_noise(t):
    """how far the raw vertex normals of the same positions agree between two evaluations: exactly on the CPU; on the GPU their face
    sums are scattered with atomics in no fixed order (process_mesh), and at a vertex whose faces nearly cancel that shows above an
    ulp of the unit normal; the bound allowed for it here is 1e-5"""
    return 0.0 if t.device.type == "cpu" else 1e-5


def _obj_vertices(text):
    return np.array([[float(x) for x in l.split()[1:]] for l in text.split("\n") if l.startswith("v ")], dtype=np.float32)


def test_dump_without_an_offset_writes_the_raw_vertices(tmp_path):
    """While no offset is set the output is the parent's: the raw positions in %.9g, then the faces."""
    sc, _ = load_scene("cbox_occluder", res=8, spp=1)
    mesh = sc.m_meshes[-1]
    p = str(tmp_path / "m.obj")
    mesh.dump(p)
    v = mesh._vertex_positions_raw.detach().cpu().numpy()
    f = mesh._face_indices.cpu().numpy()
    want = "".join("v %.9g %.9g %.9g\n" % (x[0], x[1], x[2]) for x in v)
    assert not mesh.m_has_uv
    want += "".join("f %d %d %d\n" % (x[0] + 1, x[1] + 1, x[2] + 1) for x in f)
    assert open(p).read() == want


# ----------------------------------------------------------------------------------- HyperCubeDistribution.sample_reuse, host path
@pytest.mark.parametrize("reso", [(7, 5), (6, 4, 3)])
def test_cube_sample_reuse_host_path(reso):
    cls = psdr_cuda.HyperCubeDistribution2f if len(reso) == 2 else psdr_cuda.HyperCubeDistribution3f
    d = cls()
    d.set_resolution(reso)
    g = torch.Generator().manual_seed(3)
    n = int(np.prod(reso))
    mass = torch.rand(n, generator=g)
    mass[torch.rand(n, generator=g) < 0.3] = 0.0
    s = torch.rand(8192, len(reso), generator=g).clamp(min=2.0 ** -24)
    with pytest.raises(RuntimeError):
        d.sample_reuse(s.clone())                      # before set_mass: psdr_assert(m_ready)
    d.set_mass(mass)
    w = s.clone()
    pdf = d.sample_reuse(w).t
    assert w.data_ptr() != s.data_ptr() and not torch.equal(w, s)     # warped in place
    assert ((w >= 0) & (w <= 1)).all()
    cell = torch.zeros(8192, dtype=torch.long)
    for i, r in enumerate(reso):
        cell = cell * r + torch.floor(w[:, i] * r).clamp(max=r - 1).long()
    assert (mass[cell] > 0).all()
    np.testing.assert_allclose(pdf.numpy(), (mass[cell] / mass.sum() * n).numpy(), rtol=1e-5)
    # a non-contiguous float64 view is computed, then copied back
    base = s.double().t().contiguous().t()
    assert not base.is_contiguous()
    pdf2 = d.sample_reuse(base).t
    np.testing.assert_allclose(base.numpy(), w.double().numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(pdf2.numpy(), pdf.numpy(), rtol=0, atol=0)


def test_cube_sample_reuse_host_one_cell_and_zero_mass():
    d = psdr_cuda.HyperCubeDistribution2f()
    d.set_resolution((1, 1))
    d.set_mass(torch.tensor([0.5]))
    s = torch.rand(64, 2)
    w = s.clone()
    assert torch.equal(d.sample_reuse(w).t, torch.ones(64)) and torch.equal(w, s)
    d = psdr_cuda.HyperCubeDistribution3f()
    d.set_resolution((2, 3, 4))
    d.set_mass(torch.zeros(24))
    w = torch.rand(64, 3)
    pdf = d.sample_reuse(w).t
    assert torch.equal(pdf, torch.zeros(64))
    assert (w[:, 0] < 0.5).all() and (w[:, 1] < 1 / 3).all() and (w[:, 2] < 0.25).all()      # cell 0
