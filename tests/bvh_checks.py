"""The criteria by which the GPU tests judge the hits of a tree walk (tests/test_device_bvh_cases_gpu.py; kept apart for the tests of the two-level scenes): against
another handle that runs the same triangle test, and against the float64 brute force of tests/lbvh_cases.py.  A handle's answer is the tuple
GpuScene.trace returns: (shape, tri, u, v)."""
import numpy as np

import lbvh_cases as L


def hit_t(rows, o, d, tri, u, v):
    """t of a reported hit, in float64 from the reported (triangle, u, v): the distance of that point of the triangle along the ray"""
    r = rows.astype(np.float64)
    p = r[tri, 0:3] + u[:, None].astype(np.float64) * r[tri, 3:6] + v[:, None].astype(np.float64) * r[tri, 6:9]
    return ((p - o.astype(np.float64)) * d.astype(np.float64)).sum(1) / (d.astype(np.float64) ** 2).sum(1)


def deviation(rows, rays, bf, got, clear):
    """largest |u|, |v|, |t| deviation of a handle's hits from the brute force on the clear rays it names the same triangle on"""
    o, d, _ = rays
    _, tri, u, v = got
    m = clear & (tri >= 0) & (tri == bf["tri"][:, 0])
    t = hit_t(rows, o[m], d[m], tri[m], u[m], v[m])
    return max(np.abs(u[m] - bf["u"][m, 0]).max(), np.abs(v[m] - bf["v"][m, 0]).max()), np.abs(t - bf["t"][m, 0]).max()


def check_against_brute_force(label, rows, rays, bf, dev, host):
    """A handle's answers (`dev`) against brute_force, with the slack measured on `host` (the host builder's handle, not under test).
    Outside the rays brute_force marks as near an edge or a near-tie (at most 0.2 %), the named triangle is THE float64 hit of minimal t and a miss is a
    float64 miss; barycentrics and t deviate by at most four times what the host-built handle's do on the same rays."""
    o, d, owner = rays
    excluded = bf["near_edge"] | bf["near_tie"]
    assert excluded.mean() <= 0.002, excluded.mean()
    clear = ~excluded
    assert np.array_equal(host[1][clear], bf["tri"][clear, 0]), "%s: the HOST tree disagrees with the brute force -- the reference of this test is broken" % label
    wrong = clear & (dev[1] != bf["tri"][:, 0])
    assert not wrong.any(), "%s: %d clear rays answered wrongly, e.g. ray %d: got triangle %d, float64 says %d" % (
        label, wrong.sum(), np.nonzero(wrong)[0][0], dev[1][wrong][0], bf["tri"][wrong, 0][0])
    (h_uv, h_t), (d_uv, d_t) = deviation(rows, rays, bf, host, clear), deviation(rows, rays, bf, dev, clear)
    print("%s: %d rays (%.3f %% excluded): host tree off the brute force by %.3e in (u, v), %.3e in t; device tree by %.3e, %.3e" % (
        label, o.shape[0], 100 * excluded.mean(), h_uv, h_t, d_uv, d_t))
    assert d_uv <= 4 * h_uv and d_t <= 4 * h_t, (d_uv, h_uv, d_t, h_t)
    dead = np.nonzero(rows[:, 21] == 0)[0]
    assert not np.isin(dev[1], dead).any()              # no zero-area face is ever returned


def check_device_against_host(label, rows, rays, dev, host):
    """Both handles run the same triangle test: they may differ only where two candidates tie in t to float32 resolution -- judged per differing ray by
    the float64 test of the two named triangles (lbvh_cases.pair_test); at most 0.2 % of the rays; agreeing hits agree in (u, v) to 1e-5."""
    o, d, _ = rays
    diff = np.nonzero(dev[1] != host[1])[0]
    assert diff.size <= 0.002 * o.shape[0], diff.size / o.shape[0]
    if diff.size:
        assert (dev[1][diff] >= 0).all() and (host[1][diff] >= 0).all(), "%s: one tree hits where the other misses" % label
        a, b = L.pair_test(rows, o[diff], d[diff], dev[1][diff]), L.pair_test(rows, o[diff], d[diff], host[1][diff])
        assert (a["possible"] & b["possible"]).all(), "%s: a differing ray names a triangle float64 rules out" % label
        assert (np.abs(a["t"] - b["t"]) <= a["tol_t"] + b["tol_t"]).all(), "%s: a differing ray is no tie: %s" % (label, np.abs(a["t"] - b["t"]).max())
    same = (dev[1] == host[1]) & (host[1] >= 0)
    assert same.sum() > 0.1 * o.shape[0]
    assert np.abs(dev[2][same] - host[2][same]).max() < 1e-5 and np.abs(dev[3][same] - host[3][same]).max() < 1e-5
    assert np.array_equal(dev[0][same], host[0][same])
    return diff.size
