"""Host side of Scene.sample_boundary_segment_direct's differentiable p0: the forward-mode node it registers with enoki (psdr_cuda/scene.py
_TensorNode) survives enoki.forward being called more than once while the record lives."""
import torch

import enoki as ek
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from psdr_cuda.scene import _TensorNode


def _record(P, d):
    """p0 as the native path builds it: a value plus (t - detach(t)) over a torch expression of P"""
    base = torch.rand(16, 3, generator=torch.Generator().manual_seed(0)).to(P.t.device)
    t = base + P.t * torch.tensor(d, device=P.t.device)
    p0 = Vector3fD._wrap(base + (t - t.detach()))
    ek.register_render_node(p0)
    p0._node = _TensorNode(t)
    return p0


def test_forward_twice_with_a_live_record():
    d = (0.5, -2.0, 1.0)
    P = FloatD(0.0)
    ek.set_requires_gradient(P)
    p0 = _record(P, d)
    ek.forward(P, free_graph=False)
    assert torch.equal(ek.gradient(p0).t, torch.tensor(d, device=P.t.device).expand(16, 3))
    ek.forward(P, free_graph=False)                       # the graph was kept: the same tangent again
    assert torch.equal(ek.gradient(p0).t, torch.tensor(d, device=P.t.device).expand(16, 3))
    ek.forward(P)                                         # frees the graph ...
    assert torch.equal(ek.gradient(p0).t, torch.tensor(d, device=P.t.device).expand(16, 3))
    ek.forward(P)                                         # ... so the next call finds no path to P: zeros, no exception
    g = ek.gradient(p0).t
    assert g.shape == (16, 3) and torch.count_nonzero(g) == 0


def test_forward_for_a_second_parameter():
    P, Q = FloatD(0.0), FloatD(0.0)
    ek.set_requires_gradient(P)
    ek.set_requires_gradient(Q)
    p0 = _record(P, (1.0, 2.0, 3.0))
    ek.forward(P)
    ek.forward(Q)                                         # p0 does not depend on Q
    assert torch.count_nonzero(ek.gradient(p0).t) == 0
