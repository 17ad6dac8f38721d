"""tests/tables_cases.py held to its promises, on the CPU: the dictionary edge builder against the product's host edge list, the guarded float64 formulation
of process_mesh against process_mesh itself (value, adjoint, tangent), its transposition on the degenerate families, the margin of every edge from every
threshold a keep filter compares it with, and the sizes the families exist for."""
import numpy as np
import pytest
import torch

import tables_cases as tc
from psdr_cuda.scene import build_edge_indices, process_mesh

REGULAR = tuple(n for n in tc.FAMILIES if n not in tc.DEGENERATE)


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("name", tc.MANIFOLD)
def test_edge_builder_equals_the_host_edge_list(name):
    _, f, e = tc.case(name)
    host = build_edge_indices(f)
    assert len(e) == len(host) and set(map(tuple, e.tolist())) == set(map(tuple, host.tolist()))


@pytest.mark.parametrize("name", REGULAR)
def test_guarded_formulation_equals_process_mesh(name):
    v, f, _ = tc.case(name)
    plain, guarded = tc.tri_fn(name, guarded=False), tc.tri_fn(name, guarded=True)
    ref = tc.forward(plain, [v])
    assert bool(torch.isfinite(ref).all())
    a, t = _randn(ref.shape, 1), _randn(v.shape, 2)
    for x, y in ((tc.forward(guarded, [v]), ref), (tc.adjoint(guarded, [v], a)[0], tc.adjoint(plain, [v], a)[0]), (tc.tangent(guarded, [v], [t]), tc.tangent(plain, [v], [t]))):
        assert tc.rel_l2(x.numpy(), y.numpy()) <= 1e-12


@pytest.mark.parametrize("name", tc.DEGENERATE)
def test_guarded_formulation_on_degenerate_meshes(name):
    v, f, _ = tc.case(name)
    dead_f, dead_v = tc.degenerate_elements(name)
    assert dead_v.any() and (dead_f.any() or name == "folded")
    live = tc.live_row_mask(name)
    ref = tc.forward(tc.tri_fn(name, guarded=False), [v]).numpy()
    assert np.array_equal(np.isfinite(ref), live)                 # process_mesh is non-finite exactly on the words a degenerate element touches
    g = tc.tri_fn(name)
    out = tc.forward(g, [v]).numpy()
    assert np.isfinite(out).all() and tc.rel_l2(out[live], ref[live]) <= 1e-12 and not out[~live].any()
    a, t = _randn(ref.shape, 3), _randn(v.shape, 4)
    ga, jt = tc.adjoint(g, [v], a)[0], tc.tangent(g, [v], [t])
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(jt).all()) and not jt.numpy()[~live].any() and not jt.numpy()[dead_f, 21].any()
    lhs, rhs = float((a * jt).sum()), float((ga * t).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((a * jt).abs().sum())
    # a vertex that only degenerate faces use gets no gradient through their normals and areas; a cotangent on the dead words alone gives none at all
    only_dead = tc.adjoint(g, [v], torch.as_tensor(~live | (np.arange(22) == 21) & dead_f[:, None]).double() * a)[0]
    assert not only_dead.numpy().any()


@pytest.mark.parametrize("name", tc.FAMILIES)
def test_no_edge_sits_near_a_threshold(name):
    v, f, e = tc.case(name)
    rows = tc.rows_input(name).numpy()
    worst = [np.nanmin(tc.sec_keep(rows, e)[1])]
    for cam in (0, 1):
        for mode in tc.FLAG_MODES:
            worst.append(np.nanmin(tc.prim_keep(rows, e, tc.camera(cam), tc.face_normal_flags(name, mode))[1]))
    assert min(worst) >= tc.MIN_MARGIN, worst


def test_the_second_camera_sees_silhouettes_and_the_filters_work_on_both_sides():
    for name in ("grid_256", "hub1000", "tetra"):
        _, f, e = tc.case(name)
        rows = tc.rows_input(name).numpy()
        inner = e[:, 3] >= 0
        smooth = tc.prim_keep(rows, e, tc.camera(1), tc.face_normal_flags(name, 0))[0]
        face = tc.prim_keep(rows, e, tc.camera(1), tc.face_normal_flags(name, 1))[0]
        assert 0 < smooth[inner].sum() < inner.sum() and 0 < face[inner].sum() < inner.sum(), name
    _, _, e = tc.case("coplanar")
    keep, margin = tc.sec_keep(tc.rows_input("coplanar").numpy(), e)
    assert np.isinf(margin).sum() >= 20 and not keep[np.isinf(margin)].any() and keep[(e[:, 3] >= 0) & ~np.isinf(margin)].sum() == 4      # the fold


def test_family_sizes():
    for T in tc.GRID_T:
        v, f, e = tc.case("grid_%d" % T)
        assert len(f) == T and (e[:, 3] < 0).any() and len(np.unique(f)) == len(v)
    assert len(tc.case("grid_255")[2]) % 64 != 0
    v, f, _ = tc.case("hub1000")
    assert len(f) == 1000 and np.bincount(f.ravel()).max() == 1000
    v, f, _ = tc.case("isolated")
    assert 24 * len(v) > 4 * 24 * len(f) and len(np.unique(f)) == 4 and len(v) == 104
    assert len(tc.case("one")[1]) == 1 and not (tc.case("tetra")[2][:, 3] < 0).any()
    for name in tc.FAMILIES:
        v = tc.case(name)[0]
        assert np.array_equal(v, v.astype(np.float32).astype(np.float64)) and np.abs(v).max() <= 1.25
    for k in (0, 1):
        assert tc.camera(k).shape == (22,)
