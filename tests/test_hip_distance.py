"""The distance from points to a mesh on the device (csrc/nw_distance.hip) against its NumPy restatement (tests/mesh_distance_ref.py):
d2, closest point, face and feature bit for bit, the sign wherever it is not a matter of rounding -- the equalities the compiled core
owes it in tests/test_distance_core_cpu.py -- on closed, open and mis-shaped meshes, at every count around the block and wave sizes,
through one context and through the Python surface; then against the winding number and the mesh sampler, which know nothing of it."""
import numpy as np
import pytest

import mesh_distance_ref as R
from ch_shrinkwrap_amd import distance as D
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = D.DistanceContext()
    yield c
    c.close()


def device(ctx, q, signed=True, rings=False):
    dist, closest, face, feature, s = ctx.query(q, signed=signed, return_closest=True, return_face=True, return_feature=True, return_sum=True,
                                                rings=rings)
    return dict(d2=None, dist=dist, closest=closest, face=face, feature=feature, sum=s)


def check(ctx, v, f, tw, q, signed=True):
    """one mesh and one query set on the device against the restatement -> (device arrays, restatement, signs compared)"""
    ref = R.distance(q, v, f, tw if signed else None)
    ctx.set_mesh(v, f, tw)
    dev = device(ctx, q, signed)
    # (the device hands back dist, not d2: its square root is correctly rounded, so equal |dist| bits and an equal closest point stand
    # for an equal d2; d2 itself is recomputed from the closest point the way the core does)
    e = np.ascontiguousarray(q, np.float64).reshape(-1, 3) - dev['closest']
    dev['d2'] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    n = R.same_as_restatement(dev, ref, signed)
    assert np.isclose(dev['sum'], (dev['dist'] ** 2).sum(), rtol=1e-12)
    return dev, ref, n


def mesh_case(name):
    if name == 'icosphere3':
        v, f = icosphere(3, 40.0)
        return v, f
    return getattr(R, name)()


def queries_for(v, n, seed):
    """inside and around the box, up to ten box diagonals away, and at the mesh's vertices"""
    vd = np.asarray(v, np.float64)
    diag = np.linalg.norm(vd.max(0) - vd.min(0))
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n // 4, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    far = vd.mean(0) + d * rng.uniform(1.0, 10.0, (n // 4, 1)) * diag
    return np.concatenate([R.around(v, n - n // 4, seed), far, vd[:: max(1, len(vd) // 64)]])


# ---- parity and exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cube', 'spike', 'l_prism', 'icosphere3'])
def test_closed_meshes_equal_the_restatement(ctx, name):
    v, f = mesh_case(name)
    tw = R.twins(f)
    assert (tw >= 0).all()
    q = queries_for(v, 1200, 11)
    if name == 'cube':
        q = np.concatenate([q, np.zeros((1, 3))])
    if name == 'spike':
        q = np.concatenate([q, R.spike_queries(400)])
    dev, ref, n = check(ctx, v, f, tw, q)
    assert n > 1000 and (dev['dist'] < 0).sum() > 20 and (dev['dist'] > 0).sum() > 500
    at_vertices = dev['d2'] == 0
    assert at_vertices.sum() >= min(len(v), 64) and not np.signbit(dev['dist'][at_vertices]).any()
    if name == 'cube':
        assert dev['face'][-1] == 0 and dev['dist'][-1] == -1.0                            # twelve faces tie at the centre: the smallest id
        assert np.abs(dev['dist'] - R.box_sdf(q)).max() <= 1e-12
    if name == 'spike':
        assert (dev['dist'][-400:] > 0).all()
    if name == 'l_prism':
        assert ((dev['dist'] < 0) == R.l_prism_inside(q))[np.abs(dev['dist']) > 1e-9].all()
    # without the sign: the same distances
    unsigned = ctx.query(q, signed=False)
    assert np.array_equal(unsigned, np.abs(dev['dist'])) and not np.signbit(unsigned).any()


def test_one_face_spanning_the_box_costs_time_not_exactness(ctx):
    v, f = icosphere(3, 40.0)
    big = np.array([[-45.0, -45.0, -45.0], [45.0, 45.0, -45.0], [0.0, 45.0, 45.0]], np.float32)
    v2 = np.concatenate([v, big])
    f2 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    tw = R.twins(f2)
    assert (tw[-3:] == -1).all()
    q = queries_for(v2, 1000, 12)
    dev, ref, n = check(ctx, v2, f2, tw, q)
    assert (dev['face'] == len(f)).sum() > 50 and (dev['face'] < len(f)).sum() > 200
    # the walk did go further than on the sphere alone, where the same queries end within a few rings
    rings_big = device(ctx, q, rings=True)['feature'] >> 8
    ctx.set_mesh(v, f, R.twins(f))
    rings = device(ctx, q, rings=True)['feature'] >> 8
    near = slice(0, 750)                                                                   # (the queries in and around the box)
    print('rings walked: sphere median %d max %d; with the spanning face median %d max %d'
          % (np.median(rings[near]), rings[near].max(), np.median(rings_big[near]), rings_big[near].max()))
    assert np.median(rings_big[near]) > np.median(rings[near])


def test_needles_equal_the_restatement(ctx):
    v, f = R.needles()
    vd = v.astype(np.float64)
    rng = np.random.default_rng(13)
    w = rng.dirichlet([1, 1, 1], 500)
    k = rng.integers(0, len(f), 500)
    on = (w[:, :, None] * vd[f[k]]).sum(1)
    q = np.concatenate([on + rng.normal(scale=0.05, size=on.shape), on + rng.normal(scale=30.0, size=on.shape), vd + rng.normal(scale=5.0, size=vd.shape),
                        R.around(v, 300, 13)])
    dev, ref, n = check(ctx, v, f, R.twins(f), q)
    assert n > 1000 and len(set((dev['feature'] & 7).tolist())) >= 6


def test_a_mesh_a_million_from_the_origin(ctx):
    v, f = icosphere(2, 50.0)
    v = (v + np.float32(1e6)).astype(np.float32)
    dev, ref, n = check(ctx, v, f, R.twins(f), R.around(v, 1000, 7))
    assert n > 800 and (dev['dist'] < 0).sum() > 100


# ---- counts and reuse ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sphere_case():
    v, f = icosphere(2, 30.0)
    tw = R.twins(f)
    q = queries_for(v, 513 - 41, 14)[:513]
    assert len(q) == 513
    return v, f, tw, q, R.distance(q, v, f, tw)


def test_query_counts_around_the_wave_and_block_sizes(ctx, sphere_case):
    v, f, tw, q, ref = sphere_case
    ctx.set_mesh(v, f, tw)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        dev = device(ctx, q[:n])
        assert np.array_equal(np.abs(dev['dist']), np.abs(ref['dist'][:n]))
        assert np.array_equal(dev['closest'], ref['closest'][:n]) and np.array_equal(dev['face'], ref['face'][:n])
        assert np.array_equal(dev['feature'], ref['feature'][:n])
        clear = ref['margin'][:n] > 1e-9
        assert np.array_equal(np.signbit(dev['dist'][clear]), np.signbit(ref['dist'][:n][clear]))
        assert np.isclose(dev['sum'], (dev['dist'] ** 2).sum(), rtol=1e-12)
    # any output may be left out
    only = ctx.query(q[:65])
    assert isinstance(only, np.ndarray) and np.array_equal(only, device(ctx, q[:65])['dist'])
    assert ctx.query(np.zeros((0, 3))).shape == (0,)


@pytest.mark.parametrize('n_faces', [1, 2])
def test_meshes_of_one_and_two_faces(ctx, n_faces):
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0], [4, 3, 1]], np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3]], np.int32)[:n_faces]
    v = v[:3] if n_faces == 1 else v
    q = np.concatenate([R.around(v, 300, 15, spread=3.0), R.triangle_region_queries()[2]])
    dev, ref, n = check(ctx, v, f, R.twins(f), q)
    assert n > 200 and len(set(dev['feature'].tolist())) == 7


def test_queries_on_the_device(ctx, sphere_case):
    import torch
    v, f, tw, q, ref = sphere_case
    ctx.set_mesh(v, f, tw)
    t = torch.from_numpy(q).to('cuda')
    torch.cuda.synchronize()
    dev = device(ctx, (t.data_ptr(), len(q)))
    host = device(ctx, q)
    for k in ('dist', 'closest', 'face', 'feature'):
        assert np.array_equal(dev[k], host[k])
    assert dev['sum'] == host['sum']
    bad = q.copy()
    bad[100, 1] = np.nan
    t = torch.from_numpy(bad).to('cuda')
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.query((t.data_ptr(), len(bad)))
    assert np.array_equal(ctx.query(q), host['dist'])


def test_one_context_across_three_meshes_and_runs_are_identical(sphere_case):
    c = D.DistanceContext()
    try:
        seen = []
        for name in ('icosphere3', 'cube', 'disk', 'icosphere3'):
            v, f = mesh_case(name)
            tw = R.twins(f)
            for seed in (16, 17):
                dev, ref, n = check(c, v, f, tw, queries_for(v, 300, seed))
                seen.append((name, seed, dev))
            again = device(c, queries_for(v, 300, 17))
            for k in ('dist', 'closest', 'face', 'feature'):
                assert again[k].tobytes() == dev[k].tobytes()
            assert np.float64(again['sum']).tobytes() == np.float64(dev['sum']).tobytes()
        # the first mesh again, after two others: the same bytes as the first time
        for k in ('dist', 'closest', 'face', 'feature'):
            assert seen[0][2][k].tobytes() == seen[6][2][k].tobytes()
        assert seen[0][2]['sum'] == seen[6][2]['sum']
    finally:
        c.close()


# ---- open meshes and bad input ----------------------------------------------------------------------------------------------------------
def test_open_disk_unsigned_and_signed(ctx):
    v, f = R.disk()
    tw = R.twins(f)
    a = 2.0 * np.pi * np.arange(64) / 64
    rim = np.stack([2.5 * np.cos(a), 2.5 * np.sin(a), 0.4 * np.cos(3 * a) + 0.05], 1)       # nearest to the border's edges and vertices
    q = np.concatenate([R.around(v, 400, 18, spread=2.0) + [0, 0, 0.3], rim])
    taken = {}
    R.distance(q, v, f, tw, taken=taken)
    assert taken.get('border', 0) > 10 and taken.get('border_edge', 0) > 10                # the inputs do take the border branches
    dev, ref, n = check(ctx, v, f, tw, q)
    assert n > 400
    above = q[:, 2] > 1e-6
    assert (dev['dist'][above] > 0).all() and (dev['dist'][q[:, 2] < -1e-6] < 0).all()
    check(ctx, v, f, None, q, signed=False)


def test_signed_needs_a_twin_table(ctx):
    v, f = R.disk()
    ctx.set_mesh(v, f, None)
    with pytest.raises(RuntimeError, match='bad argument'):
        ctx.query(np.zeros((4, 3)), signed=True)
    assert ctx.query(np.array([[0.0, 0.0, 2.0]]), signed=False)[0] == 2.0


def test_bad_input_is_refused_and_the_context_stays_usable(ctx):
    v, f = R.cube()
    tw = R.twins(f)
    q = R.around(v, 100, 19)
    ctx.set_mesh(v, f, tw)
    good = ctx.query(q)
    not_involution = tw.copy()
    not_involution[0] = tw[1]
    out_of_range = tw.copy()
    out_of_range[5] = 3 * len(f)
    for bad in (not_involution, out_of_range):
        with pytest.raises(RuntimeError, match='bad argument'):
            ctx.set_mesh(v, f, bad)
        with pytest.raises(RuntimeError, match='no mesh'):                                  # a failed set_mesh leaves no mesh behind
            ctx.query(q)
    nan_pos = v.copy()
    nan_pos[3, 2] = np.nan
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.set_mesh(nan_pos, f, tw)
    ctx.set_mesh(v, f, tw)
    nan_q = q.copy()
    nan_q[7, 0] = np.inf
    with pytest.raises(RuntimeError, match='non-finite'):
        ctx.query(nan_q)
    assert np.array_equal(ctx.query(q), good)


# ---- cross-checks with units that know nothing of this one ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['cube', 'spike', 'l_prism', 'icosphere3'])
def test_sign_agrees_with_the_winding_number(ctx, name):
    from ch_shrinkwrap_amd.surgery import SurgeryContext
    v, f = mesh_case(name)
    # in and around the box, and -- the spike fills a twentieth of its box -- convex combinations of the vertices (inside, where the
    # mesh is convex), with as many again scaled by 1.6 about the vertices' mean (the winding query takes float32 points)
    rng = np.random.default_rng(23)
    w = rng.dirichlet(np.ones(len(v)) * (1.0 if len(v) <= 12 else 0.05), 256)
    hull = w @ v.astype(np.float64)
    q = np.concatenate([R.around(v, 512, 20), hull, v.astype(np.float64).mean(0) + 1.6 * (hull - v.astype(np.float64).mean(0))])
    q = q.astype(np.float32).astype(np.float64)
    ctx.set_mesh(v, f, R.twins(f))
    dist = ctx.query(q)
    s = SurgeryContext()
    try:
        w = s.winding(v, f, np.zeros(len(f), np.int32), 1, q.astype(np.float32))[:, 0]
    finally:
        s.close()
    diag = np.linalg.norm(v.max(0).astype(np.float64) - v.min(0))
    clear = np.abs(dist) > 1e-3 * diag
    print('%s: %d queries clear of the surface, %d of them inside by the winding number' % (name, clear.sum(), (w[clear] > 0.5).sum()))
    assert clear.sum() > 800 and (w[clear] > 0.5).sum() > 150 and (w[clear] < 0.5).sum() > 150
    assert np.array_equal(dist[clear] < 0, w[clear] > 0.5)


def test_no_sample_of_the_mesh_is_nearer_than_the_mesh(ctx):
    from ch_shrinkwrap_amd.evaluation import EvaluationContext, SAMPLES
    v, f = icosphere(3, 40.0)
    q = queries_for(v, 1000, 21)
    ctx.set_mesh(v, f, R.twins(f))
    dist = ctx.query(q)
    e = EvaluationContext()
    try:
        assert e.sample_mesh(v, f, 2.0) > 1000
        nearest, _, _ = e.nearest(SAMPLES, q, return_index=False)
    finally:
        e.close()
    assert (np.abs(dist) <= nearest * (1 + 1e-9)).all()
    assert np.median(nearest - np.abs(dist)) < 2.0                                          # ... and not by much: the samples are 2 apart


# ---- the Python surface, end to end ---------------------------------------------------------------------------------------------------------
def test_python_surface(ctx):
    v, f = icosphere(2, 30.0)
    q = queries_for(v, 300, 22)
    ref = R.distance(q, v, f, R.twins(f))
    mesh = TriMesh(v, f)
    d, c, face = D.distance_to_mesh(q, mesh, return_closest=True, return_face=True)
    assert np.array_equal(np.abs(d), np.abs(ref['dist'])) and np.array_equal(c, ref['closest']) and np.array_equal(face, ref['face'])
    assert np.array_equal(mesh.signed_distance(q), d)
    assert np.array_equal(D.distance_to_mesh(q, (v, f), context=ctx), d) and ctx.n_faces == len(f) and ctx.has_twin
    assert np.array_equal(D.distance_to_mesh(q, (v, f), signed=False, context=ctx), np.abs(d)) and not ctx.has_twin


def test_c1_fit_then_distance_to_mesh():
    """Config C1 as synth.make_config defines it (2 562 vertices 20 nm outside a sphere of 100 nm, 10^4 localizations of sigma 10 nm,
    20 iterations in one block at lams = 10) through ShrinkwrapMembrane, then DistanceToMesh.  Measured on an MI355X: the start surface
    has a median signed distance of -19.1 nm (97 % of the localizations inside it), the fit -4.2 nm (quantiles 5 / 95 %: -20.1 / +11.3;
    67 % inside).  With the recipe module's own defaults instead of the config's (curvature_weight 20, remeshed every 5) 20 iterations
    leave -13.9 nm and 39 leave -9.7: that fit needs some 160 iterations (tests/test_evaluation.py)."""
    from ch_shrinkwrap_amd import synth
    from ch_shrinkwrap_amd.evaluation import EvaluationContext, SAMPLES
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    cfg = synth.make_config('c1', seed=0)
    assert cfg['vertices'].shape[0] == 2562 and cfg['points'].shape[0] == 10000

    class Surf(object):
        vertices, faces = cfg['vertices'], cfg['faces']
    pts = cfg['points']
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    ns = {'surf': Surf, 'filtered_localizations': table}
    mesh = ShrinkwrapMembrane(max_iters=cfg['iters'], curvature_weight=cfg['lams'][0], remesh_frequency=cfg['block']).execute(ns)
    out = D.DistanceToMesh().execute(ns)
    assert ns['distances'] is out and sorted(out) == sorted(list(table) + ['distance_to_mesh', 'closest_face'])
    for k in table:
        assert out[k] is table[k]
    d, face = out['distance_to_mesh'], out['closest_face']
    assert d.shape == (10000,) and d.dtype == np.float64 and face.dtype == np.int32 and face.min() >= 0 and face.max() < len(mesh.faces)
    e = EvaluationContext()
    try:
        assert e.sample_mesh(np.asarray(mesh.vertices), mesh.faces, 5.0) > 1000             # fit_quality's samples
        nearest, _, _ = e.nearest(SAMPLES, np.ascontiguousarray(pts, np.float64), return_index=False)
    finally:
        e.close()
    assert (np.abs(d) <= nearest * (1 + 1e-9)).all()
    print('C1: signed distance quantiles 5/50/95 %% = %s nm, %.1f %% inside' % (np.round(np.percentile(d, [5, 50, 95]), 2), 100.0 * (d < 0).mean()))
    assert abs(np.median(d)) < 10.0
    assert (d < 0).mean() > 0.2 and (d > 0).mean() > 0.2                                    # localizations scatter to both sides of a good fit
