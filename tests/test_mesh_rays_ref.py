"""
The NumPy restatement of ray casting (tests/mesh_rays_ref.py) tied to ground truth that does not come from it: closed forms on lattice
boxes and spheres, the parity of points known to be inside or outside, the degenerate cases of the definition, three mutations that
each turn an assertion red, and agreement with the sign of the point-to-mesh distance's restatement.
"""
import numpy as np
import pytest

import mesh_distance_ref as D
import mesh_rays_ref as R

UP = np.array([0.0, 0.0, 1.0])


def bottom_rays(n=4):
    o = np.array([[x, y, 0] for x in range(1, n) for y in range(1, n)], np.float64)
    return o, np.tile(UP, (len(o), 1))


def cube_checks(mutate=None):
    """the closed lattice cube's closed forms, as a list of booleans by name"""
    v, f, ids = R.lattice_box()
    assert v.shape == (98, 3) and f.shape == (192, 3)
    o, d = bottom_rays()
    r = R.cast(v, f, o, d, mutate=mutate)
    out = {'vertex_t': bool((r['t'] == 4.0).all()), 'vertex_exits': bool((r['info'] == 1).all()), 'vertex_fan': bool((r['hits'] == 6).all())}
    # the fan's six faces tie at t = 4: the smallest id among the faces of the top vertex
    top = [ids[(int(p[0]), int(p[1]), 4)] for p in o]
    out['tie_smallest'] = all(r['face'][i] == np.flatnonzero((f == top[i]).any(1)).min() for i in range(len(o)))
    d64 = v.astype(np.float64)
    cen = d64[f].mean(1)
    low = np.flatnonzero(cen[:, 2] == 0.0)
    rc = R.cast(v, f, cen[low], np.tile(UP, (len(low), 1)), mutate=mutate)
    out['centroid_t'] = bool((rc['t'] == 4.0).all() and (rc['hits'] >= 1).all() and (rc['info'] == 1).all())
    hit = R.cast(v, f, o, d, t_max=4.0, mutate=mutate)
    miss = R.cast(v, f, o, d, t_max=np.nextafter(4.0, 0.0), mutate=mutate)
    out['t_max'] = bool((hit['t'] == 4.0).all() and (miss['face'] == -1).all() and np.isinf(miss['t']).all() and (miss['hits'] == 0).all())
    return out


def test_the_closed_lattice_cube():
    assert all(cube_checks().values()), cube_checks()


def test_three_mutations_are_caught():
    red = {m: [k for k, ok in cube_checks(m).items() if not ok] for m in R.MUTATIONS}
    assert 'vertex_t' in red['strict'] and 'vertex_fan' in red['strict']                  # the ray leaks through the top vertex
    assert 'vertex_fan' in red['t_ge'] and 'vertex_t' in red['t_ge']                      # the origin's own fan is hit at t = 0
    assert red['tie_larger'] == ['tie_smallest']


def test_a_strict_edge_test_leaks_through_every_lattice_vertex():
    v, f, _ = R.lattice_box()
    o, d = bottom_rays()
    assert (R.cast(v, f, o, d, mutate='strict')['face'] == -1).all() and (R.cast(v, f, o, d)['face'] >= 0).all()


@pytest.mark.parametrize('a,b,c', [(1, 1, 1), (2, 3, 5), (7, 1, 2)])
def test_integer_boxes_give_their_opposite_face_distances(a, b, c):
    v, f, _ = R.lattice_box(a, b, c)
    cen = v.astype(np.float64)[f].mean(1)
    nrm = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    r = R.cast(v, f, cen, -nrm, skip_face=np.arange(len(f)))                                # inward from every face's centroid
    axis = np.argmax(np.abs(nrm), axis=1)
    length = np.array([a, b, c], np.float64)[axis]
    assert (r['face'] >= 0).all() and (r['info'] == 1).all()
    assert np.array_equal(r['t'] * np.abs(nrm).max(1), length)                              # |nrm| = 1 on a unit lattice: t is the distance
    assert np.array_equal(cen[np.arange(len(f)), axis] == 0, v.astype(np.float64)[f[r['face']]][:, 0, :][np.arange(len(f)), axis] == length)


@pytest.mark.parametrize('nsub', [2, 3])
def test_inward_rays_of_a_sphere(nsub):
    Rs = 100.0
    v, f = R.sphere(nsub, Rs)
    d64 = v.astype(np.float64)
    n = R.vertex_normals(v, f)
    r = R.cast(v, f, d64, -n, skip_vertex=np.arange(len(v)))
    assert (r['face'] >= 0).all() and (r['info'] == 1).all()
    vmax = np.linalg.norm(d64, axis=1).max()
    assert (r['t'] <= 2.0 * vmax).all()
    # the mesh contains the ball of radius r_in (the least distance of a face's plane from the centre); a ray from |p| = R' tilted by
    # alpha from the radial direction leaves that ball at R' cos(alpha) + sqrt(r_in^2 - R'^2 sin^2(alpha)), and the mesh no earlier
    fn = np.cross(d64[f[:, 1]] - d64[f[:, 0]], d64[f[:, 2]] - d64[f[:, 0]])
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    r_in = np.abs((fn * d64[f[:, 0]]).sum(1)).min()
    rad = np.linalg.norm(d64, axis=1)
    cos_a = np.clip((n * d64).sum(1) / rad, -1.0, 1.0)
    bound = rad * cos_a + np.sqrt(r_in ** 2 - rad ** 2 * (1.0 - cos_a ** 2))
    assert (r['t'] >= bound).all()
    if nsub == 2:
        assert 98.2 < r_in < 98.25 and 199.1 < r['t'].min() and r['t'].max() < 200.00001


def parity_classes(v):
    """(points, directions, surely inside, surely outside) of the 300 parity points against a sphere mesh of radius 100"""
    p, d = R.parity_points()
    d64 = np.asarray(v, np.float64)
    f = R.sphere(3)[1]
    fn = np.cross(d64[f[:, 1]] - d64[f[:, 0]], d64[f[:, 2]] - d64[f[:, 0]])
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    r_in = np.abs((fn * d64[f[:, 0]]).sum(1)).min()
    rad = np.linalg.norm(p, axis=1)
    return p, d, rad < r_in, rad > np.linalg.norm(d64, axis=1).max()


def test_parity_of_points_in_and_around_a_sphere():
    v, f = R.sphere(3)
    p, d, inner, outer = parity_classes(v)
    assert (~inner & ~outer).sum() <= 0.05 * len(p) and inner.sum() > 30 and outer.sum() > 100
    hits = R.cast(v, f, p, d)['hits']
    assert (hits[inner] % 2 == 1).all() and (hits[outer] % 2 == 0).all()
    assert set(hits[inner]) == {1} and set(hits[outer]) <= {0, 2}                          # a convex body, off its edges


def test_degenerate_cases():
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    one = [[0, 1, 2]]
    assert R.cast(tri, one, [[1, 1, -1]], [[0, 0, 2]])['t'][0] == 0.5
    # a flat face is never hit: a repeated id, three collinear corners
    assert R.cast(tri, [[0, 0, 1]], [[1, 0, -1]], [UP])['face'][0] == -1
    line = np.array([[0, 0, 0], [1, 1, 0], [2, 2, 0]], np.float32)
    assert R.cast(line, one, [[1, 1, -1]], [UP])['hits'][0] == 0
    # a ray in the face's plane: den == 0
    r = R.cast(tri, one, [[-1, 1, 0]], [[1, 0, 0]])
    assert r['face'][0] == -1 and r['hits'][0] == 0 and np.isinf(r['t'][0])
    # a direction of length zero
    assert R.cast(tri, one, [[1, 1, -1]], [[0, 0, 0]])['face'][0] == -1
    # the origin on the face: t = 0 is no hit; behind the origin neither
    assert R.cast(tri, one, [[1, 1, 0]], [UP])['face'][0] == -1 and R.cast(tri, one, [[1, 1, 1]], [UP])['face'][0] == -1
    # the length of the direction scales t, not the hit
    assert R.cast(tri, one, [[1, 1, -1]], [[0, 0, 0.25]])['t'][0] == 4.0
    # the back of the face: the exit bit
    assert R.cast(tri, one, [[1, 1, -1]], [UP])['info'][0] == 1 and R.cast(tri, one, [[1, 1, 1]], [-UP])['info'][0] == 0
    # skips are by id
    two_v = np.concatenate([tri, tri + np.float32([0, 0, 1])])
    two = [[0, 1, 2], [3, 4, 5]]
    assert R.cast(two_v, two, [[1, 1, -1]], [UP])['face'][0] == 0 and R.cast(two_v, two, [[1, 1, -1]], [UP])['hits'][0] == 2
    assert R.cast(two_v, two, [[1, 1, -1]], [UP], skip_face=[0])['face'][0] == 1
    assert R.cast(two_v, two, [[1, 1, -1]], [UP], skip_vertex=[1])['face'][0] == 1
    assert R.cast(two_v, two, [[1, 1, -1]], [UP], skip_vertex=[-1], skip_face=[-1])['hits'][0] == 2
    assert R.cast(two_v, two, [[1, 1, -1]], [UP], skip_vertex=[4], skip_face=[0])['face'][0] == -1


def test_an_open_patch_is_left_through_its_border():
    n = 5
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    v = np.stack([gx.ravel(), gy.ravel(), np.zeros(n * n)], axis=1).astype(np.float32)
    f = np.array([t for i in range(n - 1) for j in range(n - 1) for t in ([i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1],
                                                                           [i * n + j, (i + 1) * n + j + 1, i * n + j + 1])], np.int32)
    o = [[2.2, 2.1, 1.0], [2.2, 2.1, 1.0], [6.0, 2.0, 1.0]]
    d = [[0, 0, -1], [1, 0, -0.2], [0, 0, -1]]
    r = R.cast(v, f, o, d)
    assert r['t'][0] == 1.0 and r['hits'][0] == 1 and r['info'][0] == 0                     # onto the front of the patch
    assert r['face'][1] == -1 and r['face'][2] == -1                                        # past the border; beside the patch


def test_inside_agrees_with_the_sign_of_the_distance():
    v, f = R.sphere(3)
    p, _ = R.parity_points()
    ref = D.distance(p, v, f, D.twins(f))
    d64 = v.astype(np.float64)
    diag = np.linalg.norm(d64.max(0) - d64.min(0))
    clear = np.abs(ref['dist']) > 1e-6 * diag
    assert clear.sum() >= 0.95 * len(p)
    from ch_shrinkwrap_amd.rays import DEFAULT_DIRECTION
    ins = R.inside(p, v, f, DEFAULT_DIRECTION)
    assert np.array_equal(ins[clear], (ref['dist'] < 0)[clear]) and 30 < ins.sum() < 150
    # and on a body that is not convex: the L-shaped prism, against its closed form
    lv, lf = D.l_prism()[:2]
    q = np.random.default_rng(4).uniform(-0.5, 2.5, (400, 3)) * [1, 1, 0.6]
    assert np.array_equal(R.inside(q, lv, lf, DEFAULT_DIRECTION), D.l_prism_inside(q))
