"""The local shape of a cloud on the device (csrc/nw_structure.hip) against the NumPy restatement (tests/local_shape_ref.py): every integer
of the moments and every bit of the eigenvalues and vectors -- on query and cloud counts around the wave and the workgroups, on the
lattice at exactly r and one ulp either side, on duplicates and on 5 000 points in one cell, on planar, axis, diagonal and single-point
clouds, with queries ten diagonals outside, with r tiny against the spacing and larger than the box, 10^6 from the origin, from host
arrays and device pointers through one context with changing r, shuffled, with and without a viewpoint; then against the pair counts,
which know nothing of this unit, and through LocalShape on a torus from PointcloudFromShape."""
import functools

import numpy as np
import pytest

import local_shape_ref as R
from ch_shrinkwrap_amd import structure as C

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 4097]
VIEW = (30.0, 30.0, 500.0)
TORUS_DENSITY = 0.004             # fluorophores per nm^3 of the simulator's lattice: about 3 000 points on the torus of the last test


@pytest.fixture(scope='module')
def ctx():
    c = C.StructureContext()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def cloud(n):
    return R.mixed(n, n + 1)


@functools.lru_cache(maxsize=None)
def reference(n, r):
    """the restatement once per size and radius, auto mode"""
    return R.local_shape(cloud(n), r)


def viewed(ref, Q, r, viewpoint):
    """the restatement with a viewpoint from the one without: the moments are the same, the float64 procedure runs again"""
    out = dict(ref)
    out.update(R.shape(ref['moments'], r, Q, viewpoint))
    return out


def run(ctx, P, r, queries=None, viewpoint=None, on_device=False):
    if on_device:
        import torch
        keep = [torch.from_numpy(np.ascontiguousarray(P, np.float32)).to('cuda')]
        cl = (keep[0].data_ptr(), len(P))
        if queries is not None:
            keep.append(torch.from_numpy(np.ascontiguousarray(queries, np.float32)).to('cuda'))
            queries = (keep[1].data_ptr(), len(keep[1]))
        torch.cuda.synchronize()
        ctx.set_cloud(cl)
    else:
        ctx.set_cloud(P)
    return ctx.query(r, queries, viewpoint)


def check(ctx, P, r, queries=None, viewpoint=None, ref=None):
    """host arrays, device pointers and once more on the cloud at hand: the restatement's integers and bits every time"""
    if ref is None:
        ref = R.local_shape(P, r, viewpoint=viewpoint) if queries is None else R.local_shape(queries, r, other=P, viewpoint=viewpoint)
    host = run(ctx, P, r, queries, viewpoint)
    R.same_as_restatement(host, ref)
    dev = run(ctx, P, r, queries, viewpoint, on_device=True)
    R.same_as_restatement(dev, ref)
    again = ctx.query(r, queries, viewpoint)
    R.same_as_restatement(again, ref)
    bare = ctx.query(r, queries, viewpoint, moments=False)
    assert bare['moments'] is None and bare['vectors'].tobytes() == host['vectors'].tobytes() and bare['flags'].tobytes() == host['flags'].tobytes()
    info = host['info']
    assert info['neighbours'] == int(ref['n'].sum()) and info['few'] == int((ref['n'] < 3).sum())
    assert info['tests'] >= info['neighbours'] and info['cells_read'] >= (1 if info['neighbours'] else 0) and info['n_cloud'] == len(P) and info['n_queries'] == len(ref['n'])
    assert again['info'] == info and dev['info'] == info                       # what is tested depends on the grid alone
    return host, ref


@pytest.mark.parametrize('n', SIZES)
def test_sizes_around_the_wave_and_the_workgroups(ctx, n):
    """n cloud points in auto mode, and n queries against a cloud of another size"""
    check(ctx, cloud(n), 6.0, ref=reference(n, 6.0))
    other = cloud(513 if n != 513 else 257)
    check(ctx, other, 6.0, queries=cloud(n), viewpoint=VIEW)


def test_lattice_points_at_exactly_r(ctx):
    L = R.lattice(7)
    for r in (2.0, float(np.nextafter(2.0, 0.0)), float(np.nextafter(2.0, 3.0))):
        host, ref = check(ctx, L, r)
        assert host['moments'][171, 0] == (27 if r < 2.0 else 33)
    host, _ = check(ctx, L, 2.0)
    assert host['moments'][171].tolist() == [33, 0, 0, 0, 26 * 2 ** 34, 0, 0, 26 * 2 ** 34, 0, 26 * 2 ** 34]


def test_a_crowded_cell_and_duplicates(ctx):
    rng = np.random.default_rng(3)
    crowd = (np.array([40.0, 40.0, 40.0]) + rng.uniform(0.0, 1.0, (4998, 3))).astype(np.float32)       # 5 000 points, all but two in one cell
    P = np.concatenate([crowd, np.array([[0.0, 0.0, 0.0], [80.0, 80.0, 80.0]], np.float32)])
    Q = np.concatenate([crowd[:300], P[-2:], [[40.5, 40.5, 41.9]]]).astype(np.float32)
    host, ref = check(ctx, P, 1.0, queries=Q)
    assert ref['n'][:300].min() > 500 and host['info']['cell_size'] > 1.0
    dup = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    host, _ = check(ctx, dup, 0.5)
    assert (host['moments'] == np.array([300] + [0] * 9)).all() and (host['flags'] == C.NWF_FLAG_POINT).all()


@pytest.mark.parametrize('name', ['plane', 'lattice_plane', 'axis', 'diagonal', 'single', 'far'])
def test_degenerate_extents_and_far_clouds(ctx, name):
    rng = np.random.default_rng(11)
    if name == 'plane':
        P = R.mixed(600, 2)
        P[:, 2] = 3.0
    elif name == 'lattice_plane':
        g = np.arange(11, dtype=np.float64)
        P = np.stack(np.meshgrid(g, g, [7.0], indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    elif name == 'axis':
        P = np.zeros((400, 3), np.float32)
        P[:, 1] = rng.uniform(0.0, 300.0, 400)
    elif name == 'diagonal':
        P = (np.arange(-20, 21, dtype=np.float64)[:, None] * np.array([[1.0, 2.0, -1.0]])).astype(np.float32)
    elif name == 'single':
        P = np.array([[1.0, 2.0, 3.0]], np.float32)
    else:
        P = R.mixed(600, 3, offset=1.0e6)                         # float32 steps of 1/16 out there
    for r in (3.0, 7.5):
        host, ref = check(ctx, P, r, viewpoint=VIEW if name == 'far' else None)
    if name == 'lattice_plane':
        host, _ = check(ctx, P, 3.0)
        assert host['moments'][60, 0] == 29 and (host['eigenvalues'][:, 2] == 0.0).all() and (host['vectors'][:, 2] == [0.0, 0.0, 1.0]).all()
    if name == 'single':
        check(ctx, P, 1.0, queries=np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [100.0, 2.0, 3.0]], np.float32), viewpoint=(0.0, 0.0, 9.0))


def test_queries_far_outside_see_nothing(ctx):
    rng = np.random.default_rng(5)
    P = cloud(513)
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    u = rng.normal(size=(120, 3))
    Q = ((lo + hi) / 2 + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(1.0, 10.0, (120, 1)) * diag).astype(np.float32)
    host, _ = check(ctx, P, 6.0, queries=Q, viewpoint=VIEW)
    assert (host['moments'] == 0).all() and (host['flags'] == C.NWF_FLAG_EMPTY).all()
    assert np.isnan(host['eigenvalues']).all() and (host['vectors'] == 0.0).all()
    faces = rng.uniform(lo, hi, (64, 3))
    for k in range(64):                                           # on the box's faces
        faces[k, k % 3] = lo[k % 3] if k % 2 else hi[k % 3]
    check(ctx, P, 6.0, queries=faces.astype(np.float32))


def test_a_tiny_radius_and_one_larger_than_the_box(ctx):
    P = cloud(513)
    host, _ = check(ctx, P, 1.0e-4)
    assert (host['moments'][:, 0] == 1).all() and (host['moments'][:, 1:] == 0).all() and (host['flags'] == C.NWF_FLAG_FEW).all()
    host, _ = check(ctx, P, 1.0e5)
    assert (host['moments'][:, 0] == len(P)).all() and host['info']['cells'] == 1 and host['info']['tests'] == len(P) ** 2


def test_one_context_across_clouds_and_radii(ctx):
    """one context, the cloud and the radius changing under it; a shuffled cloud gives the same rows, shuffled"""
    P = cloud(4097)
    refs = {r: reference(4097, r) for r in (6.0, 3.0)}
    perm = np.random.default_rng(1).permutation(len(P))
    for r in (6.0, 3.0, 6.0):
        R.same_as_restatement(run(ctx, P, r), refs[r])
        sh = run(ctx, P[perm], r)
        assert np.array_equal(sh['moments'], refs[r]['moments'][perm])
        assert sh['eigenvalues'].tobytes() == refs[r]['eigenvalues'][perm].tobytes() and sh['vectors'].tobytes() == refs[r]['vectors'][perm].tobytes()
    small = cloud(65)
    R.same_as_restatement(run(ctx, small, 9.0), reference(65, 9.0))
    R.same_as_restatement(run(ctx, P, 3.0, viewpoint=VIEW), viewed(refs[3.0], P, 3.0, VIEW))
    with pytest.raises(RuntimeError):
        ctx.query(0.0)
    with pytest.raises(RuntimeError):
        ctx.query(3.0, np.array([[0.0, np.nan, 0.0]], np.float32))
    R.same_as_restatement(ctx.query(3.0), refs[3.0])                            # a refused call leaves the context as it was


def test_n_equals_the_pair_counts(ctx):
    """the neighbour count against the pair-count unit's cumulative count of the same radius, cross mode with the cloud as its own queries"""
    from ch_shrinkwrap_amd.pairs import pair_counts
    P = cloud(1025)
    for r in (2.0, 6.0):
        mine = run(ctx, P, r)
        theirs = pair_counts(P, [r], other=P, local=True)
        assert np.array_equal(mine['moments'][:, 0], np.cumsum(theirs['local'], axis=1)[:, -1].astype(np.int64))
        assert mine['info']['neighbours'] == int(theirs['cumulative'][-1])


def test_the_functions_and_the_features(ctx):
    P = cloud(513)
    ref = R.local_shape(P, 6.0, viewpoint=VIEW)
    S = C.local_shape(P, 6.0, viewpoint=VIEW, context=ctx)
    R.same_as_restatement(S, ref)
    for k in ('linearity', 'planarity', 'scattering', 'surface_variation', 'centroid_offset'):
        assert S[k].tobytes() == ref[k].tobytes(), k                            # the same float64 expressions on the same numbers
    assert np.array_equal(S['valid'], ref['valid']) and np.array_equal(S['n'], ref['n'])
    assert np.array_equal(S['axis'], ref['axis']) and np.array_equal(S['normal'], ref['normal'])
    M = C.local_moments(P[:100], 6.0, other=P)
    assert np.array_equal(M['moments'], ref['moments'][:100]) and M['quantum'] == 2.0 ** -15 and np.array_equal(M['S2'], ref['moments'][:100, 4:])
    N = C.cloud_normals(P, 6.0, viewpoint=VIEW)
    assert N.dtype == np.float32 and np.array_equal(N, ref['normal'].astype(np.float32))
    r = C.radius_from_k(P, k=10)
    from ch_shrinkwrap_amd.neighbours import kth_distance
    assert r == 1.5 * float(np.median(kth_distance(P, None, 11)))


def test_local_shape_of_a_torus_end_to_end():
    """LocalShape on a torus from PointcloudFromShape, undisturbed points on the surface: the normals lie within the sphere shells' measured
    angles (tests/local_shape_ref.py's SHELL_ANGLES, the largest median and the largest maximum, times ANGLE_FACTOR) of the shape's own
    xn yn zn up to sign, and most points are classed as plane.  The figures are printed (run with -s)."""
    from ch_shrinkwrap_amd.simulation import PointcloudFromShape
    ns = {}
    PointcloudFromShape(output='filtered_localizations', shape_name='Torus', shape_params="{'radius': 100, 'r': 30}", density=TORUS_DENSITY, p=1.0,
                        no_jitter=True).execute(ns)
    out = C.LocalShape().execute(ns)
    n = len(out['x'])
    assert 2000 <= n <= 5000 and ns['shape_localizations'] is out
    for k in ('n_neighbours', 'linearity', 'planarity', 'scattering', 'xn', 'yn', 'zn', 'xa', 'ya', 'za', 'shape_class'):
        assert len(out[k]) == n, k
    valid = out['shape_class'] >= 0
    truth = np.stack([ns['filtered_localizations'][k] for k in ('xn', 'yn', 'zn')], 1).astype(np.float64)
    truth /= np.linalg.norm(truth, axis=1)[:, None]
    mine = np.stack([out['xn'], out['yn'], out['zn']], 1)
    ang = np.degrees(np.arccos(np.minimum(1.0, np.abs((mine * truth).sum(1)))))
    shares = [float((out['shape_class'] == c).mean()) for c in (0, 1, 2)]
    print('torus: %d points, radius %.3f, neighbours %d..%d, angle median %.4f max %.4f, line/plane/blob %.3f %.3f %.3f'
          % (n, out['metadata']['radius'], out['n_neighbours'].min(), out['n_neighbours'].max(), np.median(ang), ang.max(), *shares))
    assert valid.all()
    assert np.median(ang) <= R.ANGLE_FACTOR * max(a for a, _ in R.SHELL_ANGLES.values())
    assert ang.max() <= R.ANGLE_FACTOR * max(b for _, b in R.SHELL_ANGLES.values())
    assert shares[1] > 0.9
