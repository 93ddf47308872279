"""
GPU test: ray casting on the device (include/nw_rays.h, csrc/nw_rays.hip) against the brute-force NumPy restatement
(tests/mesh_rays_ref.py, itself tied to closed forms by tests/test_mesh_rays_ref.py): t, face, the exit bit and the number of faces
hit, exactly, with and without NWC_COUNT, from host arrays and from device pointers.  The restatement looks at every face for every
ray with no grid, no clipping and no pieces, so the device's walk is checked as well as its arithmetic.  No mesh has more than
about 1 300 faces.
"""
import ctypes

import numpy as np
import pytest

import mesh_rays_ref as R
from ch_shrinkwrap_amd import rays as C
from ch_shrinkwrap_amd.trimesh import TriMesh

pytestmark = pytest.mark.gpu

UP = np.array([0.0, 0.0, 1.0])


@pytest.fixture(scope='module')
def ctx():
    c = C.RayContext()
    yield c
    c.close()


def device(ctx, o, d, **kw):
    r = ctx.cast(o, d, **kw)
    r['info'] = r['exits'].astype(np.int32)
    return r


def check(ctx, v, f, o, d, sv=None, sf=None, t_max=np.inf, on_device=False):
    """set_mesh, then the cast with NWC_COUNT and without it, against the restatement; returns the restatement's answer"""
    ref = R.cast(v, f, o, d, sv, sf, t_max)
    ctx.set_mesh(v, f)
    o = np.ascontiguousarray(o, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(d, np.float64).reshape(-1, 3)
    keep = None
    if on_device:
        import torch
        keep = [torch.from_numpy(o).to('cuda'), torch.from_numpy(d).to('cuda')]
        kw_ids = {}
        for name, a in (('skip_vertex', sv), ('skip_face', sf)):
            if a is not None:
                keep.append(torch.from_numpy(np.ascontiguousarray(a, np.int32)).to('cuda'))
                kw_ids[name] = int(keep[-1].data_ptr())
        torch.cuda.synchronize()
        o, d = (keep[0].data_ptr(), len(o)), (keep[1].data_ptr(), len(d))
    else:
        kw_ids = dict(skip_vertex=sv, skip_face=sf)
    counted = device(ctx, o, d, t_max=t_max, count=True, **kw_ids)
    R.same(counted, ref)
    first = device(ctx, o, d, t_max=t_max, **kw_ids)
    assert first['hits'] is None
    R.same(first, ref, count=False)
    return ref


@pytest.fixture(scope='module')
def noisy():
    v, f = R.noisy_sphere()
    o, d = R.mixed_rays(v, 513, 5)
    return v, f, o, d, R.cast(v, f, o, d)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 513])
def test_ray_counts_around_the_wave_and_the_block(ctx, noisy, n):
    v, f, o, d, ref = noisy
    ctx.set_mesh(v, f)
    part = {k: a[:n] for k, a in ref.items()}
    R.same(device(ctx, o[:n], d[:n], count=True), part)
    R.same(device(ctx, o[:n], d[:n]), part, count=False)


def test_every_kind_of_ray_around_the_noisy_sphere(ctx, noisy):
    """origins inside, outside, on the box's faces and ten diagonals away; directions with one and two zero components; rays that
    miss the box"""
    v, f, o, d, ref = noisy
    kind = np.arange(len(o)) % 8
    assert ((d[kind == 5] == 0).sum(1) == 1).all() and ((d[kind == 6] == 0).sum(1) == 2).all()
    assert (ref['face'][kind == 7] == -1).all() and (ref['face'][kind == 4] >= 0).all() and (ref['face'][kind == 3] >= 0).sum() > 30
    assert 100 < (ref['face'] >= 0).sum() < 450 and (ref['hits'] >= 2).sum() > 60 and 0 < ref['info'].sum() < (ref['face'] >= 0).sum()
    check(ctx, v, f, o, d)
    check(ctx, v, f, o, d, on_device=True)
    # axis-parallel rays from the box's own faces: every slab branch with o_k on the boundary
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    oo, dd = [], []
    for axis in range(3):
        for side, sign in ((lo, 1.0), (hi, -1.0), (lo, -1.0)):
            for shift in (0.0, 0.11, -0.23):
                p = 0.5 * (lo + hi) + shift
                p[axis] = side[axis]
                e = np.zeros(3)
                e[axis] = sign
                oo.append(p)
                dd.append(e)
    ref = check(ctx, v, f, oo, dd)
    assert (ref['face'] >= 0).sum() == 18 and (ref['face'] < 0).sum() == 9


def test_t_max(ctx, noisy):
    v, f, o, d, ref = noisy
    cut = check(ctx, v, f, o, d, t_max=0.7)
    assert 20 < (cut['face'] >= 0).sum() < (ref['face'] >= 0).sum()
    assert (check(ctx, v, f, o, d, t_max=0.0)['face'] == -1).all()


@pytest.mark.parametrize('length', [1e300, 1e155, 3e-162, 1e-300])
def test_directions_of_every_finite_length(ctx, sphere3, length):
    """lengths at which d.d overflows, is denormal, or is zero (nothing is hit then): the definition's answer, and no longer a walk
    than at length one (tests/test_rays_core_cpu.py settles the same, and more lengths, on the CPU)"""
    v, f = np.asarray(sphere3.vertices), np.asarray(sphere3.faces)
    o, d = R.mixed_rays(v, 257, 5)
    unit = d / np.linalg.norm(d, axis=1)[:, None]
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        ref = check(ctx, v, f, o, unit * length)
        check(ctx, v, f, o, unit * length, on_device=True)
    assert (ref['face'] == -1).all() if length < 1e-162 else 60 < (ref['face'] >= 0).sum() < 230
    pieces = ctx.cast(o, unit * length, count=True, stats=True)['pieces']
    assert pieces <= ctx.cast(o, unit, count=True, stats=True)['pieces'] + len(o)


def test_the_lattice_cube(ctx):
    v, f, ids = R.lattice_box()
    bottom = np.array([[x, y, 0] for x in (1, 2, 3) for y in (1, 2, 3)], np.float64)
    up = np.tile(UP, (9, 1))
    ref = check(ctx, v, f, bottom, up)
    assert (ref['t'] == 4.0).all() and (ref['hits'] == 6).all() and (ref['info'] == 1).all()
    own = [ids[tuple(int(c) for c in b)] for b in bottom]
    for on_device in (False, True):
        ref = check(ctx, v, f, bottom, up, sv=own, on_device=on_device)
        assert (ref['t'] == 4.0).all() and (ref['hits'] == 6).all()
    # t_max at the hit, one ulp below it, and none
    for t_max, hit in ((4.0, True), (np.nextafter(4.0, 0.0), False), (np.inf, True)):
        ref = check(ctx, v, f, bottom, up, t_max=t_max)
        assert (ref['face'] >= 0).all() == hit and (ref['face'] < 0).all() == (not hit)
    # the face hit first, passed over: the next of the fan; both skips at once; -1 for none
    first = R.cast(v, f, bottom, up)['face']
    ref = check(ctx, v, f, bottom, up, sf=first)
    assert (ref['t'] == 4.0).all() and (ref['hits'] == 5).all() and (ref['face'] != first).all()
    top = [ids[(int(b[0]), int(b[1]), 4)] for b in bottom]
    ref = check(ctx, v, f, bottom, up, sv=top, sf=first, on_device=True)
    assert (ref['face'] == -1).all()
    ref = check(ctx, v, f, bottom, up, sv=np.full(9, -1), sf=np.full(9, -1))
    assert (ref['hits'] == 6).all()
    # through vertices and edge midpoints, along the side faces (in their planes) and the diagonals, from inside and from outside
    o, d = [], []
    for start in ([1, 1, 1], [2, 1, 3], [1.5, 2, 2], [2, 2.5, 1], [-3, 2, 2], [1, 1, -2], [7, 7, 7], [0, 0, 0], [4, 2, 2], [0, 1, -1]):
        for step in ([1, 0, 0], [0, -1, 0], [0, 0, 1], [1, 1, 0], [0, 1, -1], [1, 1, 1], [-1, -1, -1], [1, -1, 1], [2, 1, 0], [0, 0, 0]):
            o.append(start)
            d.append(step)
    ref = check(ctx, v, f, o, d)
    assert (ref['hits'] > 2).sum() > 20
    assert (ref['face'][9::10] == -1).all()                                               # a direction of length zero


def test_flat_faces_needles_and_an_open_patch(ctx):
    n = 9
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    pv = np.stack([gx.ravel(), gy.ravel(), np.zeros(n * n)], axis=1).astype(np.float32)
    pf = np.array([t for i in range(n - 1) for j in range(n - 1) for t in ([i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1],
                                                                               [i * n + j, (i + 1) * n + j + 1, i * n + j + 1])], np.int32)
    assert R.centroid_grid(pv, pf)['dims'][2] == 1                                          # a grid one cell thick
    o, d = R.mixed_rays(np.array([[0, 0, -2], [8, 8, 2]], np.float32), 300, 10)
    ref = check(ctx, pv, pf, o, d)
    assert 30 < (ref['face'] >= 0).sum() < 290
    ref = check(ctx, pv, pf, [[-1, 3.3, 0], [4.2, 4.1, 0], [4.2, 4.1, 1.0]], [[1, 0, 0], [1, 0.3, 0], [5, 0, -1]])
    assert (ref['face'] == -1).all()                                                      # in the plane; out through the border
    fv = np.concatenate([pv, [[1, 1, 1], [2, 2, 2], [3, 3, 3]]]).astype(np.float32)
    ff = np.concatenate([pf[:20], [[0, 0, 5], [81, 82, 83]], pf[20:]]).astype(np.int32)
    ref = check(ctx, fv, ff, o, d)
    assert not np.isin(ref['face'], [20, 21]).any() and (ref['face'] >= 0).sum() > 30
    from mesh_intersections_ref import soup
    rng = np.random.default_rng(23)
    tris = []
    for i in range(600):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3))
        w /= np.linalg.norm(w)
        c = rng.normal(scale=0.02, size=3)
        tris.append(np.array([c - 50.0 * u, c + 50.0 * u, c + rng.uniform(-0.4, 0.4) * 50.0 * u + 0.01 * w]))
    v, f = soup(*tris)
    o = rng.normal(scale=20.0, size=(300, 3))
    ref = check(ctx, v, f, o, rng.normal(scale=0.5, size=(300, 3)) - o)
    assert (ref['hits'] > 0).sum() > 30 and ref['hits'].max() >= 3


def test_one_oversize_face_makes_every_ray_read_every_centroid(ctx):
    v, f = R.noisy_sphere(oversize=True)
    o, d = R.mixed_rays(v[:-3], 256, 6)
    ref = check(ctx, v, f, o, d)
    assert (ref['face'] == len(f) - 1).sum() > 5
    r = ctx.cast(o, d, count=True, stats=True)
    reached = int((R.cast(v, f, o, d)['hits'] > 0).sum())
    assert r['pieces'] > 0 and r['centroids'] >= reached * len(f) and 0 < r['tested'] < r['centroids']
    plain = ctx.set_mesh(*R.noisy_sphere()).cast(o, d, count=True, stats=True)
    assert r['centroids'] > 20 * plain['centroids'] > 0
    assert ctx.cast(o, d, count=True)['hits'].sum() > 0 and ctx.L.nwc_get_stats(ctx.h, C._p(np.zeros(3, np.int64))) == 0


def test_a_mesh_a_million_from_the_origin(ctx):
    v, f = R.sphere(2, 100.0, 1e6)
    o, d = R.mixed_rays(v, 300, 7)
    ref = check(ctx, v, f, o, d)
    assert 80 < (ref['face'] >= 0).sum() < 280
    ref = check(ctx, v, f, np.asarray(v, np.float64), -R.vertex_normals(v, f), sv=np.arange(len(v)))
    assert (ref['face'] >= 0).all() and (np.abs(ref['t'] - 200.0) < 2.0).all()


def test_one_and_two_faces(ctx):
    from mesh_intersections_ref import A_TRI, soup
    o, d = R.mixed_rays(np.array([[0, 0, -1], [4, 4, 1]], np.float32), 200, 9)
    ref = check(ctx, A_TRI, [[0, 1, 2]], o, d)
    assert 5 < (ref['face'] == 0).sum() < 150
    v, f = soup(A_TRI, A_TRI + np.float32([0, 0, 0.5]))
    assert (check(ctx, v, f, o, d)['hits'] == 2).sum() > 5


def test_one_context_across_meshes_and_its_refusals(ctx, noisy):
    v, f, o, d, ref = noisy
    cube = R.lattice_box()[:2]
    own = C.RayContext()
    try:
        t = np.zeros(4)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert own.L.nwc_cast(own.h, p(o), p(d), 4, None, None, np.inf, 0, p(t), None, None, None) == C.NWC_ERR_NOMESH
        for mesh in (cube, (v, f), cube, (v, f)):
            check(own, mesh[0], mesh[1], o[:100], d[:100])
        # a non-finite ray on a live context is refused, from the host and from the device, and the context goes on
        for bad_o, bad_d in ((True, False), (False, True)):
            oo, dd = o[:100].copy(), d[:100].copy()
            (oo if bad_o else dd)[37, 2] = np.nan if bad_o else np.inf
            with pytest.raises(RuntimeError, match='non-finite'):
                own.cast(oo, dd)
            import torch
            to, td = torch.from_numpy(oo).to('cuda'), torch.from_numpy(dd).to('cuda')
            torch.cuda.synchronize()
            with pytest.raises(RuntimeError, match='non-finite'):
                own.cast((to.data_ptr(), 100), (td.data_ptr(), 100))
        # ... and so is an origin so far out that the walk's allowance for rounding would exceed a cell
        far = o[:100].copy()
        far[3] = [1e12, 0.0, 0.0]
        with pytest.raises(RuntimeError, match='bad argument'):
            own.cast(far, d[:100])
        R.same(device(own, o[:100], d[:100], count=True), {k: a[:100] for k, a in ref.items()})
        # a failed set_mesh leaves the context without a mesh
        bad = np.array(v, np.float32)
        bad[5, 1] = np.nan
        with pytest.raises(RuntimeError):
            own.set_mesh(bad, f)
        assert own.L.nwc_cast(own.h, p(o), p(d), 4, None, None, np.inf, 0, p(t), None, None, None) == C.NWC_ERR_NOMESH
    finally:
        own.close()


def test_every_output_may_be_left_out(ctx, noisy):
    v, f, o, d, ref = noisy
    ctx.set_mesh(v, f)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = 100
    oo, dd = np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n])
    assert ctx.L.nwc_cast(ctx.h, p(oo), p(dd), n, None, None, np.inf, C.NWC_COUNT, None, None, None, None) == C.NWC_OK
    hits = np.full(n, -7, np.int32)
    assert ctx.L.nwc_cast(ctx.h, p(oo), p(dd), n, None, None, np.inf, C.NWC_COUNT, None, None, None, p(hits)) == C.NWC_OK
    assert np.array_equal(hits, ref['hits'][:n])
    face = np.full(n, -7, np.int32)
    assert ctx.L.nwc_cast(ctx.h, p(oo), p(dd), n, None, None, np.inf, 0, None, p(face), None, None) == C.NWC_OK
    assert np.array_equal(face, ref['face'][:n])


# ---- through Python ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sphere3():
    v, f = R.sphere(3)
    return TriMesh(v, f)


@pytest.mark.parametrize('n_rays', [1, 30])
def test_thickness_is_the_restatement_on_the_same_rays(ctx, sphere3, n_rays):
    mesh = sphere3
    r = C.thickness(mesh, n_rays=n_rays, context=ctx)
    ids, origins, dirs = C.thickness_rays(mesh, 'in', n_rays, 120.0)
    M = len(mesh.vertices)
    assert np.array_equal(ids, np.arange(M)) and np.array_equal(origins, np.asarray(mesh.vertices, np.float32).astype(np.float64))
    ref = R.cast(mesh.vertices, mesh.faces, np.repeat(origins, n_rays, axis=0), dirs.reshape(-1, 3), skip_vertex=np.repeat(ids, n_rays))
    ok = ((ref['face'] >= 0) & (ref['info'] == 1)).reshape(M, n_rays)
    t = np.where(ok, ref['t'].reshape(M, n_rays), np.nan)
    assert ok.all()                                                                        # a convex body: every inward ray is valid
    assert np.array_equal(r['n_valid'], ok.sum(1)) and np.array_equal(r['thickness'], np.nanmedian(t, axis=1))
    if n_rays == 1:
        assert np.array_equal(r['face'], ref['face']) and (np.abs(r['thickness'] - 200.0) < 1.0).all()
        assert np.array_equal(mesh.thickness()['thickness'], r['thickness'])
    else:
        # chords of a sphere at cos(theta) spread evenly over [1/2, 1]: the median is near 200 x 3/4
        assert (np.abs(r['thickness'] - 150.0) < 5.0).all() and (r['face'] >= 0).all()
    out = C.thickness(mesh, direction='out', n_rays=n_rays, context=ctx)
    assert np.isnan(out['thickness']).all() and (out['n_valid'] == 0).all() and (out['face'] == -1).all()


def test_thickness_of_a_slab_and_the_module(ctx):
    """a 40 x 40 x 5 box: the thickness of its large faces' interior vertices is 5 exactly, and a vertex no face refers to has none"""
    v, f, ids = R.lattice_box(8, 8, 1)
    v = (v * np.float32([5, 5, 5])).astype(np.float32)
    v = np.concatenate([v, [[100, 100, 100]]]).astype(np.float32)
    mesh = TriMesh(v, f)
    r = C.thickness(mesh, context=ctx)
    inner = [ids[(x, y, z)] for x in range(1, 8) for y in range(1, 8) for z in (0, 1)]
    assert (r['thickness'][inner] == 5.0).all() and (r['n_valid'][inner] == 1).all()
    assert np.isnan(r['thickness'][-1]) and r['n_valid'][-1] == 0 and r['face'][-1] == -1
    table = C.MeshThickness().execute({'membrane': mesh})
    assert list(table) == ['x', 'y', 'z', 'thickness', 'n_valid'] and len(table['x']) == len(v) - 1
    assert np.array_equal(table['thickness'], r['thickness'][:-1], equal_nan=True)
    with pytest.raises(AttributeError):
        C.MeshThickness(colour='red')
    with pytest.raises(ValueError):
        C.thickness(mesh, direction='sideways')


def test_inside_three_ways(ctx, sphere3):
    """parity along the default direction = the restatement's = the sign of distance_to_mesh = the winding number, on the points that
    are surely inside or surely outside"""
    from test_mesh_rays_ref import parity_classes
    from ch_shrinkwrap_amd import distance, surgery
    mesh = sphere3
    v, f = np.asarray(mesh.vertices), np.asarray(mesh.faces)
    p, _, inner, outer = parity_classes(v)
    sure = inner | outer
    assert (~sure).sum() <= 0.05 * len(p)
    ins = C.inside(p, mesh, context=ctx)
    assert np.array_equal(ins, R.inside(p, v, f, C.DEFAULT_DIRECTION))                       # exactly, on all 300
    assert np.array_equal(ins[sure], inner[sure])
    assert np.array_equal(ins[sure], (distance.distance_to_mesh(p, mesh) < 0)[sure])
    s = surgery.SurgeryContext()
    try:
        w = s.winding(v, f, np.zeros(len(f), np.int32), 1, p)[:, 0]
    finally:
        s.close()
    assert np.array_equal(ins[sure], (w >= 0.5)[sure])
    assert np.array_equal(C.inside(p, (v, f)), ins)


def test_cast_rays_in_one_call(noisy):
    v, f, o, d, ref = noisy
    r = C.cast_rays((v, f), o, d, count=True)
    r['info'] = r['exits'].astype(np.int32)
    R.same(r, ref)
