"""The fit-quality metric on the device (csrc/nw_evaluation.hip) against its definition on the host (ch_shrinkwrap_amd/evaluation.py) and
against the fixtures the reference's own functions produced: the samples bit for bit and in order, the nearest neighbours against
scipy's cKDTree, the two mean squared distances, run-to-run identity and the statuses of bad input."""
import ctypes

import numpy as np
import pytest
from scipy.spatial import cKDTree

from conftest import load_golden
from ch_shrinkwrap_amd import evaluation as E
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere

pytestmark = pytest.mark.gpu

OFFSET = np.array([5000.0, -3000.0, 800.0])


class Duck(object):
    """the least a mesh needs for the metric"""

    def __init__(self, v, f):
        self._vertices, self.faces = {'position': np.ascontiguousarray(v, np.float32)}, np.ascontiguousarray(f, np.int32)


def _sorted(p):
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def sampling_case(name):
    """(vertices, faces, spacings)"""
    if name in ('fit_quality', 'evaluation_case'):
        g = load_golden(name)
        return g['vertices'], g['faces'], (5.0, 11.0) if name == 'fit_quality' else (3.0, 7.5)
    if name == 'off_origin':
        v, f = icosphere(6, 300.0)
        return (v + OFFSET.astype('f4')).astype('f4'), f, (5.0,)
    if name == 'zero_area':
        v, f = icosphere(3, 100.0)
        f = f.copy()
        f[7] = [f[7, 0], f[7, 1], f[7, 1]]
        f[100] = [f[100, 2], f[100, 2], f[100, 2]]
        return v, f, (3.0,)
    if name == 'remeshed_c2':
        from ch_shrinkwrap_amd import synth
        from ch_shrinkwrap_amd.remesh import remesh_device
        cfg = synth.make_config('c2', seed=0)
        e = cfg['vertices'][cfg['faces'][:, 1]] - cfg['vertices'][cfg['faces'][:, 0]]
        v, f = remesh_device(cfg['vertices'], cfg['faces'], 3, 0.8 * float(np.linalg.norm(e, axis=1).mean()))
        return v, f, (5.0, 2.0)
    raise KeyError(name)


@pytest.fixture(scope='module')
def ctx():
    c = E.EvaluationContext()
    yield c
    c.close()


def check_samples(ctx, v, f, dx):
    """the device's samples of one mesh at one spacing against the host function's -> (samples, face ids)"""
    mesh = Duck(v, f)
    host = E.points_from_mesh(mesh, dx_min=dx)
    n = ctx.sample_mesh(v, f, dx)
    dev, face = ctx.samples(return_faces=True)
    assert n == host.shape[0] and dev.dtype == np.float64 and dev.shape == host.shape
    assert np.array_equal(_bits(dev), _bits(host))
    assert face.dtype == np.int32 and (np.diff(face) >= 0).all() and face.min() >= 0 and face.max() < len(f)
    # each sample lies in the plane of the face it names (float32 corners: a few ulp of the coordinates)
    p0 = np.asarray(v, np.float64)[np.asarray(f)[face, 0]]
    nrm = np.cross(np.asarray(v, np.float64)[np.asarray(f)[face, 1]] - p0, np.asarray(v, np.float64)[np.asarray(f)[face, 2]] - p0)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    assert np.abs(((dev - p0) * nrm).sum(1)).max() < 1e-4 * max(1.0, np.abs(v).max())
    assert np.array_equal(_bits(E.points_from_mesh(mesh, dx_min=dx, backend='device', context=ctx)), _bits(host))
    return dev, face


@pytest.mark.parametrize('name', ['fit_quality', 'evaluation_case', 'off_origin', 'zero_area', 'remeshed_c2'])
def test_samples_equal_the_host_function_bit_for_bit_and_in_order(ctx, name):
    v, f, spacings = sampling_case(name)
    for dx in spacings:
        dev, face = check_samples(ctx, v, f, dx)
        assert dev.shape[0] > 100
        if name in ('fit_quality', 'evaluation_case'):
            tag = 'points_dx' + ('%g' % dx).replace('.', '_')
            assert np.array_equal(_sorted(dev), load_golden(name)[tag])
    if name == 'zero_area':
        assert 7 not in face and 100 not in face


def test_one_context_serves_a_large_mesh_and_then_a_small_one(ctx):
    big = sampling_case('off_origin')
    small = sampling_case('fit_quality')
    for v, f, dx in ((big[0], big[1], 5.0), (small[0], small[1], 11.0), (big[0], big[1], 5.0), (small[0], small[1], 5.0)):
        host = E.points_from_mesh(Duck(v, f), dx_min=dx)
        assert ctx.sample_mesh(v, f, dx) == host.shape[0]
        assert np.array_equal(_bits(ctx.samples()), _bits(host))
        # ... and the held samples are what a query sees: every sample is its own nearest neighbour
        dist, idx, s = ctx.nearest(E.SAMPLES, host)
        assert (dist == 0).all() and s == 0.0 and np.array_equal(host[idx], host)


def cloud_pair(name):
    """(reference, queries)"""
    rng = np.random.default_rng(17)
    if name == 'golden_fit_quality':
        g = load_golden('fit_quality')
        return g['points_dx5'], g['truth'].astype(np.float64)
    if name == 'golden_evaluation_case':
        g = load_golden('evaluation_case')
        return g['a'], g['b']
    if name == 'sphere':
        v, f = icosphere(6, 300.0)
        d = rng.normal(size=(400000, 3))
        return E.points_from_mesh(Duck(v, f), dx_min=3.5), 300.0 * d / np.linalg.norm(d, axis=1)[:, None]
    if name == 'off_origin':
        d = rng.normal(size=(50000, 3))
        a = 150.0 * d / np.linalg.norm(d, axis=1)[:, None] + rng.normal(scale=4.0, size=d.shape) + OFFSET
        d = rng.normal(size=(30000, 3))
        return a, 160.0 * d / np.linalg.norm(d, axis=1)[:, None] + OFFSET
    if name == 'duplicates':
        a = rng.uniform(-100.0, 100.0, size=(5000, 3))
        return np.concatenate([a, a[:1000]]), rng.uniform(-110.0, 110.0, size=(20000, 3))
    raise KeyError(name)


def check_nearest(ctx, ref, q, duplicates=False):
    dist, idx, s = ctx.nearest(ref, q)
    assert dist.dtype == np.float64 and idx.dtype == np.int32 and dist.shape == idx.shape == (q.shape[0],)
    if duplicates:
        uniq, first = np.unique(ref, axis=0, return_index=True)
        d, i = cKDTree(uniq).query(q, k=2)
        want = first[i[:, 0]]
    else:
        d, i = cKDTree(ref).query(q, k=2)
        want = i[:, 0]
    assert np.allclose(dist, d[:, 0], rtol=1e-14, atol=0)         # (the order in which three squares are added is all that may differ)
    clear = d[:, 1] > d[:, 0] * (1 + 1e-12)
    share = 1.0 - clear.mean()
    print('near ties: %d of %d' % ((~clear).sum(), q.shape[0]))
    assert share <= 1e-4
    assert np.array_equal(idx[clear], want[clear])
    # the distance belongs to the index, and the sum to the distances
    e = ref[idx] - q
    assert np.array_equal(dist, np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]))
    assert np.isclose(s, (dist ** 2).sum(), rtol=1e-12, atol=0)
    return dist, idx, s


@pytest.mark.parametrize('name', ['golden_fit_quality', 'golden_evaluation_case', 'sphere', 'off_origin', 'duplicates'])
def test_nearest_against_ckdtree(ctx, name):
    a, b = cloud_pair(name)
    check_nearest(ctx, a, b, duplicates=name == 'duplicates')
    if name == 'duplicates':
        # a query ON a duplicated point: both copies are at distance 0, the first one is named
        dist, idx, _ = ctx.nearest(a, a[5000:])
        assert (dist == 0).all() and np.array_equal(idx, np.arange(1000))
    else:
        check_nearest(ctx, b, a)


def test_a_cloud_may_be_a_device_pointer_or_the_held_samples(ctx):
    import torch
    a, b = cloud_pair('off_origin')
    want = ctx.nearest(a, b)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    for ref, q in (((ta.data_ptr(), a.shape[0]), b), (a, (tb.data_ptr(), b.shape[0])), ((ta.data_ptr(), a.shape[0]), (tb.data_ptr(), b.shape[0]))):
        got = ctx.nearest(ref, q)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    v, f, _ = sampling_case('evaluation_case')
    ctx.sample_mesh(v, f, 3.0)
    s = ctx.samples()
    for x, y in ((ctx.nearest(E.SAMPLES, b), ctx.nearest(s, b)), (ctx.nearest(a, E.SAMPLES), ctx.nearest(a, s))):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
    assert ctx.average_squared_distance(E.SAMPLES, b) == ctx.average_squared_distance(s, b)


def test_mean_squared_distances_against_the_host(ctx):
    g = load_golden('fit_quality')
    mesh = TriMesh(g['vertices'], g['faces'])
    for tag, dx in (('dx5', 5.0), ('dx11', 11.0)):
        host = E.fit_quality(mesh, g['truth'], dx_min=dx)
        dev = E.fit_quality(mesh, g['truth'], dx_min=dx, backend='device', context=ctx)
        print(tag, host, dev)
        assert dev['n_mesh_points'] == host['n_mesh_points'] == g['points_' + tag].shape[0]
        for k in ('mse01', 'mse10', 'mse_rms'):
            assert np.isclose(dev[k], host[k], rtol=1e-12, atol=0)
        assert np.allclose([dev['mse01'], dev['mse10'], dev['mse_rms']], g['mse_' + tag], rtol=1e-12, atol=0)
    e = load_golden('evaluation_case')
    assert np.allclose(E.average_squared_distance(e['a'], e['b'], backend='device', context=ctx), e['asd'], rtol=1e-12, atol=0)
    assert np.allclose(E.average_squared_distance(e['a'], e['b'], backend='device'), e['asd'], rtol=1e-12, atol=0)      # (a context of its own)
    emesh = TriMesh(e['vertices'], e['faces'])
    host = E.fit_quality(emesh, e['b'], dx_min=3.0)
    dev = E.fit_quality(emesh, e['b'], dx_min=3.0, backend='device')
    assert dev['n_mesh_points'] == 7288 and all(np.isclose(dev[k], host[k], rtol=1e-12, atol=0) for k in ('mse01', 'mse10', 'mse_rms'))
    # the large pair: a float64 sum of n <= 10^7 non-negative terms in any order is within n 2^-53 of exact
    a, b = cloud_pair('sphere')
    host = E.average_squared_distance(a, b)
    dev = ctx.average_squared_distance(a, b)
    print('sphere pair', host, dev)
    assert np.allclose(dev, host, rtol=1e-9, atol=0)


def test_two_identical_calls_are_bit_identical(ctx):
    a, b = cloud_pair('sphere')
    x, y = ctx.nearest(a, b), ctx.nearest(a, b)
    assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(x[1], y[1])
    assert np.float64(x[2]).view(np.uint64) == np.float64(y[2]).view(np.uint64)
    m, n = ctx.average_squared_distance(a, b), ctx.average_squared_distance(a, b)
    assert np.array_equal(_bits(np.array(m)), _bits(np.array(n)))
    other = E.EvaluationContext()
    try:
        z = other.nearest(a, b)
    finally:
        other.close()
    assert np.array_equal(_bits(x[0]), _bits(z[0])) and np.array_equal(x[1], z[1]) and x[2] == z[2]
    v, f, _ = sampling_case('off_origin')
    ctx.sample_mesh(v, f, 5.0)
    s0, f0 = ctx.samples(return_faces=True)
    ctx.sample_mesh(v, f, 5.0)
    s1, f1 = ctx.samples(return_faces=True)
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(f0, f1)


def test_normals_of_the_nearest_face_centroid(ctx):
    g = load_golden('evaluation_case')
    mesh = TriMesh(g['vertices'], g['faces'])
    pts, nrm = E.points_from_mesh(mesh, dx_min=3.0, backend='device', return_normals=True, context=ctx)
    hpts, hnrm = E.points_from_mesh(mesh, dx_min=3.0, return_normals=True)
    assert np.array_equal(_bits(pts), _bits(hpts)) and nrm.shape == pts.shape and nrm.dtype == np.float32
    centers = g['vertices'][g['faces']].mean(1)
    d, i = cKDTree(centers).query(pts, k=2)
    clear = d[:, 1] > d[:, 0] * (1 + 1e-12)
    assert clear.mean() >= 1 - 1e-4
    assert np.array_equal(nrm[clear], mesh.face_normals[i[clear, 0]]) and np.array_equal(nrm[clear], hnrm[clear])
    t = E.PointsFromMesh(dx_min=3.0, backend='device').execute({'membrane0': mesh})
    assert np.array_equal(np.stack([t['x'], t['y'], t['z']], 1), hpts) and np.array_equal(np.stack([t['xn'], t['yn'], t['zn']], 1), nrm)
    sub, subn = E.points_from_mesh(mesh, dx_min=3.0, p=0.25, rng=np.random.default_rng(2), backend='device', return_normals=True, context=ctx)
    pick = np.random.default_rng(2).choice(hpts.shape[0], size=int(0.25 * hpts.shape[0]), replace=False)
    assert np.array_equal(sub, hpts[pick]) and np.array_equal(subn, nrm[pick])


def test_bad_arguments_and_non_finite_points_return_their_statuses():
    c = E.EvaluationContext()
    try:
        L, h = c.L, c.h
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        a, b = cloud_pair('golden_evaluation_case')
        s = ctypes.c_double()
        assert L.nwe_nearest(h, p(a), a.shape[0], p(b), b.shape[0], None, None, ctypes.byref(s)) == E.NWE_OK and s.value > 0
        assert L.nwe_nearest(h, p(a), 0, p(b), b.shape[0], None, None, ctypes.byref(s)) == E.NWE_ERR_BADARG
        assert L.nwe_nearest(h, p(a), a.shape[0], p(b), 0, None, None, ctypes.byref(s)) == E.NWE_ERR_BADARG
        assert L.nwe_nearest(h, None, a.shape[0], p(b), b.shape[0], None, None, ctypes.byref(s)) == E.NWE_ERR_BADARG
        assert L.nwe_nearest(h, None, E.NWE_SAMPLES, p(b), b.shape[0], None, None, ctypes.byref(s)) == E.NWE_ERR_NOSAMPLES
        assert b'no samples' in L.nwe_last_error(h)
        assert L.nwe_get_samples(h, None, None) == E.NWE_ERR_NOSAMPLES
        for bad in (np.nan, np.inf, -np.inf):
            x = a.copy()
            x[123, 1] = bad
            assert L.nwe_nearest(h, p(x), x.shape[0], p(b), b.shape[0], None, None, ctypes.byref(s)) == E.NWE_ERR_NONFINITE
            assert b'reference' in L.nwe_last_error(h)
            assert L.nwe_nearest(h, p(b), b.shape[0], p(x), x.shape[0], None, None, ctypes.byref(s)) == E.NWE_ERR_NONFINITE
            assert b'query' in L.nwe_last_error(h)
            m0, m1 = ctypes.c_double(), ctypes.c_double()
            assert L.nwe_average_squared_distance(h, p(x), x.shape[0], p(b), b.shape[0], ctypes.byref(m0), ctypes.byref(m1)) == E.NWE_ERR_NONFINITE
        with pytest.raises(RuntimeError, match='non-finite'):
            c.nearest(x, b)
        v, f = icosphere(4, 300.0)
        n = ctypes.c_int64(-7)
        assert L.nwe_sample_mesh(h, p(v), v.shape[0], p(f), f.shape[0], 1e-3, ctypes.byref(n)) == E.NWE_ERR_TOOMANY and n.value == 0
        assert L.nwe_sample_mesh(h, p(v), v.shape[0], p(f), f.shape[0], 0.0, ctypes.byref(n)) == E.NWE_ERR_BADARG
        assert L.nwe_sample_mesh(h, p(v), v.shape[0], p(f), f.shape[0], 1e4, ctypes.byref(n)) == E.NWE_OK and n.value == 0    # no node falls in a face
        assert L.nwe_get_samples(h, None, None) == E.NWE_ERR_NOSAMPLES
        vbad = v.copy()
        vbad[3, 0] = np.nan
        assert L.nwe_sample_mesh(h, p(vbad), v.shape[0], p(f), f.shape[0], 5.0, ctypes.byref(n)) == E.NWE_ERR_BADARG
        # the context works after every refusal
        assert c.sample_mesh(v, f, 20.0) == E.points_from_mesh(Duck(v, f), dx_min=20.0).shape[0]
        with pytest.raises(ValueError):
            E.points_from_mesh(type('M', (), {'_vertices': {'position': v.astype('f8')}, 'faces': f})(), backend='device', context=c)
    finally:
        c.close()


def test_mesh_properties_on_the_device():
    from test_evaluation_recipes import CASES
    from ch_shrinkwrap_amd import surgery
    for name in sorted(CASES):
        (v, f), euler, genus, comps, area, volume = CASES[name]
        mesh = TriMesh(v, f)
        host = E.mesh_properties(mesh, label_faces=surgery.scipy_label_faces)
        dev = E.MeshProperties().execute({'membrane': mesh})
        assert (dev['euler'][0], dev['genus'][0], dev['manifold'][0], dev['components'][0]) == (euler, genus, 1, comps)
        assert mesh.components == comps and mesh.genus == genus
        assert np.isclose(dev['area'][0], host['area'], rtol=1e-6) and np.isclose(dev['volume'][0], host['volume'], rtol=1e-6)
