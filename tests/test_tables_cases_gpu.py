"""The psdr_geo_* entries (csrc/psdr_tables.hip) on the meshes of tests/tables_cases.py against float64 references: TriangleInfo rows, secondary- and
primary-edge records with their keep flags (every edge compared), each forward, in reverse and in forward mode, the transposition <a, J t> = <J^T a, t> of
every adjoint / tangent pair, edge compaction with its distributions, the emitter tables, the argument checks, and a render through a mesh with a collapsed
face.

Error bound of a case: max(4 r, 2e-6) with r = rel_l2(the float32 torch formulation on the CPU, float64) -- tables_cases.bound; every case prints r, the
kernel's error and their ratio ("RATIO ..." lines; a ratio is taken against max(r, 5e-7), so that it is the share of the bound used times 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
import tables_cases as tc
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from psdr_cuda import _abi, tables_native
from psdr_cuda.scene import look_at

pytestmark = pytest.mark.gpu
W = _abi.TRI_STRIDE
NAN = float("nan")


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc):
    assert rc == 0, _abi.load_hip().psdr_last_error()


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda().contiguous()


def host(t):
    return t.detach().double().cpu().numpy()


def full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def gauss(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def held(label, out, ref, r, mask=None, factor=tc.FACTOR):
    """the kernel's rel-L2 against float64 on the words the reference has (and the mask leaves) is within the case's bound"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    m = np.isfinite(ref) if mask is None else (mask & np.isfinite(ref))
    assert np.isfinite(out[m]).all(), label
    err = tc.rel_l2(out[m], ref[m]) if np.abs(ref[m]).sum() > 0 else float(np.abs(out[m]).max(initial=0.0))
    print("RATIO %s: r %.2e, kernel %.2e, ratio %.2f" % (label, r, err, err / max(r, tc.FLOOR / tc.FACTOR)))
    assert err <= tc.bound(r, factor), (label, err, r)


# ------------------------------------------------------------------------------------------------ 1. tri_rows
def tri_fwd(name, stride, offset=False):
    lib = _abi.load_hip()
    v64, f, _ = tc.case(name)
    v, faces = dev(v64), dev(f, torch.int32)
    V, T = v.shape[0], faces.shape[0]
    buf = full((T * stride + 1,), NAN)
    rows = (buf[1:] if offset else buf[:T * stride]).view(T, stride)
    assert rows.data_ptr() % 8 == (4 if offset else 0)
    vsum = full((V, 3), NAN)
    _check(lib.psdr_geo_tri_rows_fwd(V, T, _p(v), _p(faces), _p(vsum), _p(rows), stride, _stream()))
    return v, faces, vsum, rows


def tri_rev(v, faces, vsum, a, stride):
    V, T = v.shape[0], faces.shape[0]
    a_v, a_vsum = full((V, 3), 0.0), full((V, 3), NAN)
    d0 = dev(a)          # (held in names: a temporary would be freed, and its block reused, before the call)
    _check(_abi.load_hip().psdr_geo_tri_rows_rev(V, T, _p(v), _p(faces), _p(vsum), _p(d0), stride, _p(a_vsum), _p(a_v), _stream()))
    return host(a_v)


def tri_jvp(v, faces, vsum, t, stride):
    V, T = v.shape[0], faces.shape[0]
    t_vsum, t_rows = full((V, 3), NAN), full((T, stride), NAN)
    d0 = dev(t)
    _check(_abi.load_hip().psdr_geo_tri_rows_jvp(V, T, _p(v), _p(faces), _p(vsum), _p(d0), stride, _p(t_vsum), _p(t_rows), _stream()))
    return t_rows


@pytest.mark.parametrize("stride", (22, W))
@pytest.mark.parametrize("name", tc.FAMILIES)
def test_tri_rows(name, stride):
    v64, f, _ = tc.case(name)
    V, T = len(v64), len(f)
    live = tc.live_row_mask(name)
    dead_f, _ = tc.degenerate_elements(name)
    v, faces, vsum, rows = tri_fwd(name, stride)
    # forward: against process_mesh on every word it defines; a degenerate face has area 0, as before
    (r,), (ref,) = tc.float32_error("fwd", tc.tri_fn(name, guarded=False), [v64], mask=live)
    out = host(rows)
    held("%s/%d tri_rows fwd" % (name, stride), out[:, :22], ref.numpy(), r, mask=live)
    assert not out[:, 22:].any() and not out[dead_f, 21].any()
    _, _, vsum2, rows2 = tri_fwd(name, stride)
    assert torch.equal(bits(rows2), bits(rows)) and torch.equal(bits(vsum2), bits(vsum))
    if name == "isolated":                                        # a row table that is not 8-byte aligned: the accumulators take the scratch
        _, _, vsum3, rows3 = tri_fwd(name, stride, offset=True)
        assert torch.equal(bits(rows3), bits(rows)) and torch.equal(bits(vsum3), bits(vsum))
    # reverse: Gaussian cotangents, then with every third row zero; on a degenerate family against the guarded formulation, and once more with
    # nothing on the rows a degenerate element touches
    fn = tc.tri_fn(name)
    cots = [gauss((T, stride), 11), gauss((T, stride), 12)]
    cots[1][::3] = 0.0
    if name in tc.DEGENERATE:
        cots.append(gauss((T, stride), 13) * live.all(1)[:, None])
    for k, a in enumerate(cots):
        (r,), (g64,) = tc.float32_error("rev", fn, [v64], a[:, :22])
        g = tri_rev(v, faces, vsum, a, stride)
        assert np.isfinite(g).all(), (name, k)
        held("%s/%d tri_rows rev[%d]" % (name, stride, k), g, g64.numpy(), r)
    # forward mode
    t = gauss((V, 3), 14)
    (r,), (j64,) = tc.float32_error("jvp", fn, [v64], [t])
    t_rows = host(tri_jvp(v, faces, vsum, t, stride))
    assert np.isfinite(t_rows).all() and not t_rows[:, 22:].any()
    held("%s/%d tri_rows jvp" % (name, stride), t_rows[:, :22], j64.numpy(), r)


# ------------------------------------------------------------------------------------------------ 2. edge records
def edge_inputs(name):
    v64, f, e = tc.case(name)
    rows64 = tc.rows_input(name).numpy()
    rows = np.zeros((len(f), W), np.float32)
    rows[:, :22] = rows64
    return v64, e, rows64, dev(v64), dev(e, torch.int32), dev(rows)


def sec_rev(E, edges, a, V, T):
    """a_v and the row adjoint: 123 in the words the entry has no business in, and one row in front of the table (a face id of -1 must not be gathered)"""
    a_v = full((V, 3), 0.0)
    buf = full((T + 1, W), 123.0)
    a_rows = buf[1:]
    a_rows[:, 18:21] = 0.0
    d0 = dev(a)
    _check(_abi.load_hip().psdr_geo_sec_edges_rev(E, _p(edges), _p(d0), _p(a_v), _p(a_rows), W, _stream()))
    assert bool((buf[0] == 123.0).all())
    return a_v, a_rows


@pytest.mark.parametrize("name", tc.EDGE_FAMILIES)
def test_sec_edges(name):
    lib = _abi.load_hip()
    v64, e, rows64, v, edges, rows = edge_inputs(name)
    E, V, T = len(e), len(v64), rows.shape[0]
    bnd = e[:, 3] < 0
    fn = tc.sec_fn(name)
    info, keep = full((E, 16), NAN), full((E,), 7, torch.uint8)
    _check(lib.psdr_geo_sec_edges_fwd(E, _p(edges), _p(v), _p(rows), W, _p(info), _p(keep), _stream()))
    (r,), (ref,) = tc.float32_error("fwd", fn, [v64, rows64])
    out = host(info)
    held("%s sec_edges fwd" % name, out, ref.numpy(), r)
    assert np.array_equal(keep.cpu().numpy().astype(bool), tc.sec_keep(rows64, e)[0])                # every edge
    assert not out[bnd, 9:12].any() and np.array_equal(out[:, 15], bnd.astype(np.float64))
    # reverse: cotangents that are zero on every fourth edge; words 18..20 of the row adjoint and nothing else
    a = gauss((E, 16), 21)
    a[::4] = 0.0
    (rv, rr), (gv, gr) = tc.float32_error("rev", fn, [v64, rows64], a)
    a_v, a_rows = sec_rev(E, edges, a, V, T)
    held("%s sec_edges rev a_v" % name, host(a_v), gv.numpy(), rv)
    held("%s sec_edges rev a_rows" % name, host(a_rows)[:, 18:21], gr.numpy()[:, 18:21], rr)
    assert bool((a_rows[:, :18] == 123.0).all()) and bool((a_rows[:, 21:] == 123.0).all())
    z_v, z_rows = sec_rev(E, edges, np.zeros((E, 16), np.float32), V, T)
    assert not bool(z_v.any()) and not bool(z_rows[:, 18:21].any())
    # forward mode
    tv, tr = gauss((V, 3), 22), gauss((T, W), 23)
    (r,), (j64,) = tc.float32_error("jvp", fn, [v64, rows64], [tv, tr[:, :22]])
    t_info = full((E, 16), NAN)
    d0, d1 = dev(tv), dev(tr)
    _check(lib.psdr_geo_sec_edges_jvp(E, _p(edges), _p(d0), _p(d1), W, _p(t_info), _stream()))
    t_out = host(t_info)
    assert np.isfinite(t_out).all() and not t_out[bnd, 9:12].any() and not t_out[:, 15].any()
    held("%s sec_edges jvp" % name, t_out, j64.numpy(), r)


def prim_rev(E, edges, v, cam, a):
    a_v, a_w = full((v.shape[0], 3), 0.0), full((16,), 0.0)
    d0 = dev(a)
    _check(_abi.load_hip().psdr_geo_prim_edges_rev(E, _p(edges), _p(v), _p(cam), _p(d0), _p(a_v), _p(a_w), _stream()))
    return a_v, a_w.reshape(4, 4)


@pytest.mark.parametrize("cam_id", (0, 1))
@pytest.mark.parametrize("name", tc.EDGE_FAMILIES)
def test_prim_edges(name, cam_id):
    lib = _abi.load_hip()
    v64, e, rows64, v, edges, rows = edge_inputs(name)
    E, V = len(e), len(v64)
    cam64 = tc.camera(cam_id)
    cam, w2s64 = dev(cam64), cam64[:16].reshape(4, 4)
    fn = tc.prim_fn(name)
    for mode in tc.FLAG_MODES:
        flags = tc.face_normal_flags(name, mode)
        rows8, z4, keep = full((E, 8), NAN), full((E, 4), NAN), full((E,), 7, torch.uint8)
        d0 = dev(flags, torch.uint8)
        _check(lib.psdr_geo_prim_edges_fwd(E, _p(edges), _p(d0), _p(v), _p(rows), W, _p(cam), _p(rows8), _p(z4), _p(keep), _stream()))
        assert np.array_equal(keep.cpu().numpy().astype(bool), tc.prim_keep(rows64, e, cam64, flags)[0]), mode       # every edge
    (r,), (ref,) = tc.float32_error("fwd", fn, [v64, w2s64])
    held("%s/cam%d prim_edges fwd" % (name, cam_id), host(rows8), ref.numpy(), r)
    z64, faces2 = tc.prim_z4(v64, e, cam64)
    assert tc.rel_l2(host(z4[:, :2]), z64) <= tc.FLOOR                                                # one dot product and one division of exact inputs
    assert np.array_equal(bits(z4[:, 2:]).cpu().numpy(), faces2)
    # reverse: zero on every fourth edge
    a = gauss((E, 8), 31)
    a[::4] = 0.0
    (rv, rw), (gv, gw) = tc.float32_error("rev", fn, [v64, w2s64], a)
    a_v, a_w = prim_rev(E, edges, v, cam, a)
    held("%s/cam%d prim_edges rev a_v" % (name, cam_id), host(a_v), gv.numpy(), rv)
    held("%s/cam%d prim_edges rev a_w2s" % (name, cam_id), host(a_w)[[0, 1, 3]], gw.numpy()[[0, 1, 3]], rw)
    assert not bool(a_w[2].any()) and not gw.numpy()[2].any()
    z_v, z_w = prim_rev(E, edges, v, cam, np.zeros((E, 8), np.float32))
    assert not bool(z_v.any()) and not bool(z_w.any())
    # forward mode
    tv, tw = gauss((V, 3), 32), gauss((4, 4), 33) * np.float32(1e-2)
    (r,), (j64,) = tc.float32_error("jvp", fn, [v64, w2s64], [tv, tw])
    t8 = full((E, 8), NAN)
    d0, d1 = dev(tv), dev(tw)
    _check(lib.psdr_geo_prim_edges_jvp(E, _p(edges), _p(v), _p(cam), _p(d0), _p(d1), _p(t8), _stream()))
    t_out = host(t8)
    assert np.isfinite(t_out).all() and not t_out[:, 4:].any()
    held("%s/cam%d prim_edges jvp" % (name, cam_id), t_out, j64.numpy(), r)


# ------------------------------------------------------------------------------------------------ 3. transposition
def transposed(label, a_jt, jta_t, r):
    """<a, J t> (the products given term by term) against <J^T a, t>, both summed in float64, to the case's bound times sum |a_i (J t)_i|"""
    lhs, rhs, scale = float(np.sum(a_jt)), float(np.sum(jta_t)), float(np.abs(a_jt).sum())
    assert np.isfinite([lhs, rhs]).all(), label
    print("RATIO %s: <a, Jt> %.9e, <JTa, t> %.9e, bound %.2e, difference / scale %.2e" % (label, lhs, rhs, tc.bound(r), abs(lhs - rhs) / max(scale, 1e-30)))
    assert abs(lhs - rhs) <= tc.bound(r) * scale, (label, lhs, rhs, scale)


@pytest.mark.parametrize("name", tc.FAMILIES)
def test_tri_rows_adjoint_is_the_transpose_of_the_tangent(name):
    v64, f, _ = tc.case(name)
    fn = tc.tri_fn(name)
    v, faces, vsum, _ = tri_fwd(name, W)
    a, t = gauss((len(f), W), 41), gauss((len(v64), 3), 42)
    r = max(tc.float32_error("rev", fn, [v64], a[:, :22])[0][0], tc.float32_error("jvp", fn, [v64], [t])[0][0])
    jt = host(tri_jvp(v, faces, vsum, t, W))
    transposed("%s tri_rows" % name, a.astype(np.float64) * jt, tri_rev(v, faces, vsum, a, W) * t.astype(np.float64), r)


@pytest.mark.parametrize("name", tc.EDGE_FAMILIES)
def test_edge_adjoints_are_the_transposes_of_the_tangents(name):
    lib = _abi.load_hip()
    v64, e, rows64, v, edges, rows = edge_inputs(name)
    E, V, T = len(e), len(v64), rows.shape[0]
    a, tv, tr = gauss((E, 16), 43), gauss((V, 3), 44), gauss((T, W), 45)
    fn = tc.sec_fn(name)
    r = max(tc.float32_error("rev", fn, [v64, rows64], a)[0] + tc.float32_error("jvp", fn, [v64, rows64], [tv, tr[:, :22]])[0])
    t_info = full((E, 16), NAN)
    d0, d1 = dev(tv), dev(tr)
    _check(lib.psdr_geo_sec_edges_jvp(E, _p(edges), _p(d0), _p(d1), W, _p(t_info), _stream()))
    a_v, a_rows = sec_rev(E, edges, a, V, T)
    rhs = np.concatenate([(host(a_v) * tv).ravel(), (host(a_rows)[:, 18:21] * tr[:, 18:21]).ravel()])
    transposed("%s sec_edges" % name, a.astype(np.float64) * host(t_info), rhs, r)
    cam64 = tc.camera(1)
    cam, w2s64 = dev(cam64), cam64[:16].reshape(4, 4)
    a8, tw = gauss((E, 8), 46), gauss((4, 4), 47) * np.float32(1e-2)
    fn = tc.prim_fn(name)
    r = max(tc.float32_error("rev", fn, [v64, w2s64], a8)[0] + tc.float32_error("jvp", fn, [v64, w2s64], [tv, tw])[0])
    t8 = full((E, 8), NAN)
    d0, d1 = dev(tv), dev(tw)
    _check(lib.psdr_geo_prim_edges_jvp(E, _p(edges), _p(v), _p(cam), _p(d0), _p(d1), _p(t8), _stream()))
    a_v, a_w = prim_rev(E, edges, v, cam, a8)
    rhs = np.concatenate([(host(a_v) * tv).ravel(), (host(a_w) * tw).ravel()])
    transposed("%s prim_edges" % name, a8.astype(np.float64) * host(t8), rhs, r)


# ------------------------------------------------------------------------------------------------ 4. compaction
def make_rows(E, S, w0, wn, seed, zero=None):
    """Gaussian rows whose weight (|row[w0:w0+3]| or row[w0]) is log-uniform over 1e-6 .. 1e3; zero: a bool [E] of rows of weight exactly zero"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = torch.randn(E, S, device="cuda", generator=g)
    wt = 10.0 ** (torch.rand(E, device="cuda", generator=g) * 9.0 - 6.0)
    if zero is not None:
        wt = wt * (~zero).float()
    if wn == 1:
        rows[:, w0] = wt
    else:
        d = rows[:, w0:w0 + 3]
        rows[:, w0:w0 + 3] = d / d.norm(dim=1, keepdim=True) * wt[:, None]
    return rows


def walk(cmf, size, u):
    """sample_reuse's binary search (csrc/psdr_math.h) over a table of `size` entries, for every u at once"""
    lo, hi = np.zeros(len(u), np.int64), np.full(len(u), size - 1, np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) >> 1
        less = cmf[mid] < u
        lo, hi = np.where(act & less, np.minimum(mid + 1, hi), lo), np.where(act & ~less, mid, hi)
    return lo


def check_compaction(rows, keep, w0, wn, aux=None, A=0):
    E, S = rows.shape
    out, aux_out, pos, pmf, cmf, hdr = tables_native.compact_edges(rows, keep, w0, wn, aux=aux, aux_cols=A)
    k = keep.bool()
    n = int(k.sum())
    assert int(hdr[:1].view(torch.int32)) == n
    assert torch.equal(out[:n], rows[k]) and not bool(out[n:].any())
    if A:
        assert torch.equal(aux_out[:n], aux[k][:, :A]) and not bool(aux_out[n:].any())
    assert torch.equal(pos[k].long(), torch.arange(n, device="cuda")) and bool((pos[~k] == -1).all())
    w = rows[k][:, w0].double() if wn == 1 else rows[k][:, w0:w0 + 3].double().norm(dim=1)
    total = float(w.sum())
    assert abs(float(hdr[1]) - total) <= 1e-5 * total
    assert bool(torch.isfinite(cmf).all()) and float(cmf.min()) >= 0.0 and float(cmf.max()) <= 1.0
    assert float(cmf[max(n - 1, 0):].min()) == 1.0 and not bool(pmf[n:].any())
    if total > 0:
        ref_pmf = w / total
        assert tc.rel_l2(host(pmf[:n]), ref_pmf.cpu().numpy()) < 1e-6
        assert abs(float(pmf.double().sum()) - 1.0) < 1e-5
        if n > 1:
            assert float((cmf[:n - 1].double() - torch.cumsum(ref_pmf, 0)[:n - 1]).abs().max()) < 1e-5
        # the search of sample_reuse over the capacity table: inside the kept rows, and on a row of zero weight only at a u that is a cmf entry
        c, p = cmf.cpu().numpy(), pmf.cpu().numpy()
        u = np.random.default_rng(E).random(4096, dtype=np.float32)
        i = walk(c, E, u)
        assert int(i.max()) < n
        assert not ((p[i] == 0) & (c[i] != u)).any()
    else:
        assert not bool(pmf.any())
    # reverse and forward mode through pos: the scatter and the gather, to the bit; outputs fully written
    lib, idx = _abi.load_hip(), torch.nonzero(k).reshape(-1)
    g = torch.Generator(device="cuda").manual_seed(E + 1)
    a_out, t_rows = torch.randn(E, S, device="cuda", generator=g), torch.randn(E, S, device="cuda", generator=g)
    a_rows, t_out = full((E, S), NAN), full((E, S), NAN)
    _check(lib.psdr_geo_compact_edges_rev(E, S, _p(pos), _p(a_out), _p(a_rows), _stream()))
    _check(lib.psdr_geo_compact_edges_jvp(E, S, _p(pos), _p(t_rows), _p(t_out), _stream()))
    ref = torch.zeros(E, S, device="cuda")
    ref[idx] = a_out[:n]
    assert torch.equal(a_rows, ref)
    assert torch.equal(t_out[:n], t_rows[k]) and not bool(t_out[n:].any())
    return out, aux_out, pos, pmf, cmf, hdr


def bernoulli(E, seed=0):
    g = torch.Generator(device="cuda").manual_seed(1000 + E + seed)
    return (torch.rand(E, device="cuda", generator=g) < 0.37).to(torch.uint8)


def aux_words(E):
    g = torch.Generator(device="cuda").manual_seed(E)
    return torch.randint(-5, 1 << 20, (E, 5), device="cuda", generator=g, dtype=torch.int32)


@pytest.mark.parametrize("E", (1, 63, 64, 65, 1023, 1024, 1025, 2048))
def test_compaction_sizes(E):
    keep = bernoulli(E)
    if E == 1:
        keep[:] = 1
    check_compaction(make_rows(E, 16, 13, 3, E), keep, 13, 3, aux=aux_words(E), A=2)        # weight in the last columns, two aux words of a stride of five
    check_compaction(make_rows(E, 16, 15, 1, E), keep, 15, 1)                                 # wn = 1 in the last column, no aux words


@pytest.mark.parametrize("E", (1 << 20, (1 << 20) + 1))
def test_compaction_past_one_trip_of_the_top_scan(E):
    """more than 1024 blocks of 1024 rows: k_compact_top walks its loop twice at E = 2^20 + 1"""
    rows = make_rows(E, 8, 7, 1, E)
    check_compaction(rows, bernoulli(E), 7, 1)
    if E > 1 << 20:
        for keep in keep_patterns(E):
            check_compaction(rows, keep, 7, 1)


def keep_patterns(E):
    ar = torch.arange(E, device="cuda")
    return [(m.to(torch.uint8)) for m in (ar >= 0, ar < 0, ar == 0, ar == E - 1, (ar // 1024) % 2 == 0, (ar // 1024) % 2 == 1)]


@pytest.mark.parametrize("wn", (1, 3))
def test_compaction_keep_patterns(wn):
    E, S = 1025, 16
    rows = make_rows(E, S, S - wn, wn, 5)
    for keep in keep_patterns(E):
        check_compaction(rows, keep, S - wn, wn, aux=aux_words(E), A=2)


@pytest.mark.parametrize("wn", (1, 3))
def test_compaction_zero_weights(wn):
    E, S = 2048, 16
    keep = bernoulli(E, 1)
    kept = torch.nonzero(keep).reshape(-1)
    zero = torch.zeros(E, dtype=torch.bool, device="cuda")
    mid = len(kept) // 2
    zero[kept[mid - 20:mid + 20]] = True                         # a run of kept rows of weight zero in the middle ...
    zero[kept[-1]] = True                                         # ... and the last kept row
    check_compaction(make_rows(E, S, S - wn, wn, 6, zero=zero), keep, S - wn, wn)
    zero[kept[-30:]] = True                                       # a run at the end
    check_compaction(make_rows(E, S, S - wn, wn, 7, zero=zero), keep, S - wn, wn)
    # every kept weight zero: a zero sum, an all-zero pmf, a finite cmf that is 1 from the last kept row on
    _, _, _, pmf, cmf, hdr = check_compaction(make_rows(E, S, S - wn, wn, 8, zero=keep.bool()), keep, S - wn, wn)
    assert float(hdr[1]) == 0.0 and not bool(pmf.any()) and bool(torch.isfinite(cmf).all())


def test_compaction_c_entry_writes_every_output_word():
    """the forward entry itself on NaN / sentinel-filled buffers against the wrapper's result"""
    E, S = 1025, 16
    rows, keep, aux = make_rows(E, S, 13, 3, 9), bernoulli(E, 2), aux_words(E)
    want = tables_native.compact_edges(rows, keep, 13, 3, aux=aux, aux_cols=2)
    out, aux_out, pos = full((E, S), NAN), full((E, 2), -77, torch.int32), full((E,), -77, torch.int32)
    pmf, cmf, hdr = full((E,), NAN), full((E,), NAN), full((2,), NAN)
    scratch = torch.empty(4 * ((E + 1023) // 1024), dtype=torch.int32, device="cuda")
    _check(_abi.load_hip().psdr_geo_compact_edges_fwd(E, _p(rows), S, _p(keep), 13, 3, _p(aux), 5, 2, _p(scratch), _p(out), _p(aux_out), _p(pos), _p(pmf), _p(cmf),
                                                      _p(hdr), _stream()))
    for x, y in zip((out, aux_out, pos, pmf, cmf, hdr), want):
        assert torch.equal(bits(x), bits(y))


# ------------------------------------------------------------------------------------------------ 5. emitter tables
def test_emitter_tables_on_synthetic_meshes():
    counts = [1, 1023, 1024, 1025, 2049]
    foff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    F = int(foff[-1])
    rng = np.random.default_rng(50)
    area = (10.0 ** rng.uniform(-3, 1, F)).astype(np.float32)
    rows = torch.zeros(F, W, device="cuda")
    rows[:, 21] = dev(area)
    # emitters out of mesh order: mesh 4, the environment, mesh 1, mesh 2
    em_mesh, env_w = [4, 0, 1, 2], np.array([-1.0, 0.75, -1.0, -1.0], np.float32)
    mesh_emitter = np.array([-1, 2, 3, -1, 0], np.int32)
    emitter_i, off = np.zeros((4, 4), np.int32), 0
    for k, m in enumerate(em_mesh):
        if env_w[k] < 0:
            emitter_i[k] = [m, 0, counts[m], off]
            off += counts[m]
    radiance = rng.uniform(0.5, 4.0, (4, 3)).astype(np.float32)
    a64 = area.astype(np.float64)
    mesh_ref = np.array([a64[foff[m]:foff[m + 1]].sum() for m in range(5)])
    marea, ef, epmf, ecmf, fpmf, fcmf = tables_native.emitter_tables(rows, dev(foff, torch.int32), dev(mesh_emitter, torch.int32), dev(emitter_i, torch.int32),
                                                                     dev(radiance), dev(env_w), off)
    assert np.abs(host(marea) / mesh_ref - 1).max() < 1e-5
    lum = radiance.astype(np.float64) @ np.array([.2126, .7152, .0722])
    wt = np.where(env_w >= 0, env_w, mesh_ref[em_mesh] * lum)
    assert abs(host(epmf).sum() - 1) < 1e-6 and abs(float(ecmf[-1]) - 1) < 1e-6
    assert tc.rel_l2(host(epmf), wt / wt.sum()) < 1e-6 and np.abs(host(ecmf) - np.cumsum(wt / wt.sum())).max() < 1e-6
    ef_ref = np.zeros((4, 8))
    for k, m in enumerate(em_mesh):
        ef_ref[k, 3] = wt[k] / wt.sum()
        if env_w[k] < 0:
            seg = a64[foff[m]:foff[m + 1]]
            o = emitter_i[k, 3]
            assert np.array_equal(host(fpmf[o:o + counts[m]]), seg)
            got = host(fcmf[o:o + counts[m]])
            assert abs(got[-1] / seg.sum() - 1) < 1e-5 and tc.rel_l2(got, np.cumsum(seg)) < 1e-5
            ef_ref[k, :3], ef_ref[k, 4], ef_ref[k, 5] = radiance[k], 1.0 / seg.sum(), seg.sum()
    got = host(ef)
    assert tc.rel_l2(got[:, :6], ef_ref[:, :6]) < 1e-5 and not got[:, 6:].any() and not got[1, [0, 1, 2, 4, 5]].any()
    # no emitter at all: the areas alone, null emitter pointers
    marea0, *_ = tables_native.emitter_tables(rows, dev(foff, torch.int32), dev(np.full(5, -1), torch.int32), None, None, None, 0)
    assert np.abs(host(marea0) / mesh_ref - 1).max() < 1e-5


# ------------------------------------------------------------------------------------------------ 6. argument checks
def test_invalid_arguments_fail_before_any_launch():
    lib = _abi.load_hip()
    v64, f, e = tc.case("tetra")
    V, T, E, S = len(v64), len(f), len(e), 8
    v, faces, edges = dev(v64), dev(f, torch.int32), dev(e, torch.int32)
    ins = dict(rows=full((T, W), 1.0), cam=dev(tc.camera(0)), flags=full((E,), 1, torch.uint8), a16=full((E, 16), 1.0), a8=full((E, 8), 1.0), keep=full((E,), 1, torch.uint8),
               pos=full((E,), 0, torch.int32), aux=full((E, 5), 3, torch.int32), vmesh=full((V,), 0, torch.int32), mats=torch.eye(4, device="cuda").reshape(1, 4, 4).contiguous(),
               foff=dev([0, T], torch.int32), mem=dev([-1], torch.int32))
    o = {k: full(s, 77.0) for k, s in dict(vsum=(V, 3), rows=(T, W), a_v=(V, 3), info=(E, 16), rows8=(E, 8), z4=(E, 4), a_w=(16,), out=(E, S), pmf=(E,), cmf=(E,), hdr=(2,),
                                           area=(1,)).items()}
    oi = {k: full(s, 77, dt) for k, (s, dt) in dict(keep=((E,), torch.uint8), pos=((E,), torch.int32), aux=((E, 2), torch.int32), scratch=((4,), torch.int32)).items()}
    x, y, st = {k: _p(t) for k, t in ins.items()}, {k: _p(t) for k, t in {**o, **oi}.items()}, _stream()
    pv, pf, pe = _p(v), _p(faces), _p(edges)
    valid = {
        "psdr_geo_world_vertices_fwd": [V, pv, x["vmesh"], x["mats"], y["a_v"], st],
        "psdr_geo_tri_rows_fwd": [V, T, pv, pf, y["vsum"], y["rows"], W, st],
        "psdr_geo_tri_rows_rev": [V, T, pv, pf, pv, x["rows"], W, y["vsum"], y["a_v"], st],
        "psdr_geo_tri_rows_jvp": [V, T, pv, pf, pv, pv, W, y["vsum"], y["rows"], st],
        "psdr_geo_sec_edges_fwd": [E, pe, pv, x["rows"], W, y["info"], y["keep"], st],
        "psdr_geo_sec_edges_rev": [E, pe, x["a16"], y["a_v"], y["rows"], W, st],
        "psdr_geo_sec_edges_jvp": [E, pe, pv, x["rows"], W, y["info"], st],
        "psdr_geo_prim_edges_fwd": [E, pe, x["flags"], pv, x["rows"], W, x["cam"], y["rows8"], y["z4"], y["keep"], st],
        "psdr_geo_prim_edges_rev": [E, pe, pv, x["cam"], x["a8"], y["a_v"], y["a_w"], st],
        "psdr_geo_prim_edges_jvp": [E, pe, pv, x["cam"], pv, None, y["rows8"], st],
        "psdr_geo_compact_edges_fwd": [E, x["a8"], S, x["keep"], 5, 3, x["aux"], 5, 2, y["scratch"], y["out"], y["aux"], y["pos"], y["pmf"], y["cmf"], y["hdr"], st],
        "psdr_geo_compact_edges_rev": [E, S, x["pos"], x["a8"], y["out"], st],
        "psdr_geo_compact_edges_jvp": [E, S, x["pos"], x["a8"], y["out"], st],
        "psdr_geo_emitter_tables": [1, x["rows"], W, x["foff"], x["mem"], 0, None, None, None, y["area"], None, None, None, None, None, st],
    }
    # (entry, argument index, bad value): sizes of zero, a row stride of 21, wn = 2, w0 + wn > S, aux_stride < A, and a null in place of every required pointer
    bad = [("psdr_geo_world_vertices_fwd", 0, 0), ("psdr_geo_tri_rows_fwd", 0, 0), ("psdr_geo_tri_rows_fwd", 1, 0), ("psdr_geo_tri_rows_fwd", 6, 21),
           ("psdr_geo_tri_rows_rev", 0, 0), ("psdr_geo_tri_rows_rev", 1, 0), ("psdr_geo_tri_rows_rev", 6, 21), ("psdr_geo_tri_rows_jvp", 0, 0),
           ("psdr_geo_tri_rows_jvp", 1, 0), ("psdr_geo_tri_rows_jvp", 6, 21), ("psdr_geo_sec_edges_fwd", 0, 0), ("psdr_geo_sec_edges_fwd", 4, 21),
           ("psdr_geo_sec_edges_rev", 0, 0), ("psdr_geo_sec_edges_rev", 5, 21), ("psdr_geo_sec_edges_jvp", 0, 0), ("psdr_geo_sec_edges_jvp", 4, 21),
           ("psdr_geo_prim_edges_fwd", 0, 0), ("psdr_geo_prim_edges_fwd", 5, 21), ("psdr_geo_prim_edges_rev", 0, 0), ("psdr_geo_prim_edges_jvp", 0, 0),
           ("psdr_geo_compact_edges_fwd", 0, 0), ("psdr_geo_compact_edges_fwd", 5, 2), ("psdr_geo_compact_edges_fwd", 4, 6), ("psdr_geo_compact_edges_fwd", 7, 1),
           ("psdr_geo_compact_edges_rev", 0, 0), ("psdr_geo_compact_edges_jvp", 0, 0), ("psdr_geo_emitter_tables", 0, 0), ("psdr_geo_emitter_tables", 2, 21)]
    optional = {("psdr_geo_sec_edges_jvp", 2), ("psdr_geo_sec_edges_jvp", 3), ("psdr_geo_prim_edges_jvp", 4), ("psdr_geo_prim_edges_jvp", 5)}     # a null tangent = zero
    for name, args in valid.items():
        if name == "psdr_geo_emitter_tables":
            bad += [(name, i, None) for i in (1, 3, 4, 9)]
        else:
            bad += [(name, i, None) for i, a in enumerate(args[:-1]) if a is not None and a > 1 << 20 and (name, i) not in optional]      # the pointers
    torch.cuda.synchronize()
    for name, i, value in bad:
        args = list(valid[name])
        args[i] = value
        assert getattr(lib, name)(*args) != 0, (name, i, value)
        assert b"invalid argument" in lib.psdr_last_error() and name.encode() in lib.psdr_last_error(), (name, i, lib.psdr_last_error())
    torch.cuda.synchronize()
    for k, t in {**o, **oi}.items():
        assert bool((t == 77).all()), k


# ------------------------------------------------------------------------------------------------ 7. end to end
def sliver_scene(with_sliver, sppe):
    """a floor pair under an area light, and a mesh of two live faces with (or without) a collinear face on two of their vertices, seen from z = +5"""
    sc = psdr_cuda.Scene()
    sc.opts.width = sc.opts.height = 16
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 4, sppe, sppe, 0
    cam = psdr_cuda.PerspectiveCamera(40.0, 0.1, 1e3)
    cam.to_world = look_at([0, 0, 5], [0, 0, 0], [0, 1, 0])
    sc.add_sensor(cam)
    b = psdr_cuda.Diffuse([0.5, 0.6, 0.7]); b.id = "b"
    sc.add_bsdf(b)
    v64, f, _ = tc.case("sliver")
    parts = [(([[2, -0.5, 3], [3, -0.5, 3], [3, 0.5, 3], [2, 0.5, 3]], [[0, 2, 1], [0, 3, 2]]), [30.0, 30.0, 30.0]),          # the light, turned towards -z, outside the view
             (([[-1.5, -1.5, -1], [1.5, -1.5, -1], [1.5, 1.5, -1], [-1.5, 1.5, -1]], [[0, 1, 2], [0, 2, 3]]), None),
             ((v64[:5], f[:3] if with_sliver else f[:2]), None)]
    for (verts, faces), radiance in parts:
        m = psdr_cuda.Mesh()
        m.use_face_normals = True
        m.set_geometry(np.asarray(verts, np.float32), np.asarray(faces, np.int32))
        sc.add_mesh(m, b, emitter_radiance=radiance)
    sc.finalize()
    v = Vector3fD(ek.detach(m.vertex_positions))
    ek.set_requires_gradient(v)
    m.vertex_positions = v
    sc.configure()
    return sc, v


def render_gradient(with_sliver, sppe):
    sc, v = sliver_scene(with_sliver, sppe)
    img = psdr_cuda.DirectIntegrator(1, 1).renderD(sc, 0)
    adj = torch.randn(img.t.shape, generator=torch.Generator().manual_seed(70)).cuda()
    ek.backward(FloatD._wrap((img.t * adj).sum().reshape(1)))
    return host(img.t), host(ek.gradient(v).t)


def test_render_gradient_through_a_mesh_with_a_collapsed_face():
    img1, g1 = render_gradient(True, 0)
    img0, g0 = render_gradient(False, 0)
    assert np.isfinite(img1).all() and np.isfinite(g1).all()
    assert np.abs(g0[:4]).max() > 0
    err = tc.rel_l2(g1[:4], g0[:4])
    print("vertex gradient with the collapsed face against without: rel-L2 %.2e" % err)
    assert err <= 1e-5, err
    img2, g2 = render_gradient(True, 4)
    assert np.isfinite(img2).all() and np.isfinite(g2).all()
