"""
CPU test of the restatement alone (tests/local_shape_ref.py): the NumPy brute force that the compiled core and the device are later asked
to equal bit for bit is tied here to closed forms on lattices, to exact geometry (a plane, a line), to counts, to its own invariances, to
np.linalg.eigvalsh and to the radial direction of a noisy sphere shell; three one-line mutations are shown caught.
"""
import numpy as np
import pytest

import local_shape_ref as R

# the noisy sphere shells of the tests (radius 100, sigma 3): (points, seed, r, how many of the points are queries)
SHELLS = {'2000_r50': (2000, 0, 50.0, 2000), '2000_r35': (2000, 1, 35.0, 2000), '20000_r20': (20000, 2, 20.0, 1500)}
# The largest |eigenvalue - eigvalsh| / largest eigenvalue the restatement shows on the inputs of test_eigenvalues_against_eigvalsh
EIGVALSH_SEEN = 1.502e-15


@pytest.fixture(scope='module')
def shells():
    out = {}
    for name, (n, seed, r, nq) in SHELLS.items():
        P = R.shell(n, seed)
        out[name] = (P, r, R.local_shape(P[:nq], r, other=P))
    return out


def test_the_lattice_in_closed_form():
    """the 7^3 unit lattice at its centre, r = 2: the centre, 6 at distance 1, 12 at sqrt 2, 8 at sqrt 3 and 6 at exactly 2 are in: 33.
    R = 2, s = 2^17: sum u_x^2 = (2 + 8 + 8) * 2^34 + 2 * 4 * 2^34 = 26 * 2^34.  One ulp below 2 the six at distance 2 leave (R, s stay)."""
    L = R.lattice(7)
    c = np.array([[3.0, 3.0, 3.0]], np.float32)
    M = R.moments(c, 2.0, other=L)[0]
    assert M.tolist() == [33, 0, 0, 0, 446676598784, 0, 0, 446676598784, 0, 446676598784] and 26 * 2 ** 34 == 446676598784
    M = R.moments(c, float(np.nextafter(2.0, 0.0)), other=L)[0]
    assert M.tolist() == [27, 0, 0, 0, 18 * 2 ** 34, 0, 0, 18 * 2 ** 34, 0, 18 * 2 ** 34]
    M = R.moments(c, float(np.nextafter(2.0, 3.0)), other=L)[0]                  # one ulp above: R = 4, s = 2^16, the same 33 points
    assert M.tolist() == [33, 0, 0, 0, 26 * 2 ** 32, 0, 0, 26 * 2 ** 32, 0, 26 * 2 ** 32]
    S = R.local_shape(c, 2.0, other=L)
    assert S['eigenvalues'][0].tolist() == [26.0 / 33.0] * 3 and S['flags'][0] == R.FLAG_VALID      # isotropic: C is diagonal, no rotation runs
    assert np.array_equal(S['vectors'][0], np.eye(3))


def test_a_plane_is_exactly_flat():
    """an 11 x 11 lattice at z = 7, r = 3: every u_z is 0, so is row z of C, the rotations that touch z are skipped"""
    g = np.arange(11, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, [7.0], indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    S = R.local_shape(P, 3.0)
    c = 5 * 11 + 5
    assert P[c].tolist() == [5.0, 5.0, 7.0] and S['n'][c] == 29
    assert (S['eigenvalues'][:, 2] == 0.0).all() and np.array_equal(S['normal'], np.tile([0.0, 0.0, 1.0], (121, 1)))
    assert S['valid'].all() and (S['planarity'] + S['linearity'] == 1.0).all() and (S['scattering'] == 0.0).all()
    assert S['planarity'][c] == 1.0 and S['centroid_offset'][c] == 0.0


def test_a_line_has_one_axis():
    """a collinear lattice along (1, 2, -1): the axis is parallel to it and linearity is 1, both to 1e-15.  The two small eigenvalues are
    zero up to rounding and may be a few ulp (of the largest) below zero: the features clamp them, the eigenvalues are reported as
    computed."""
    t = np.arange(-20, 21, dtype=np.float64)[:, None] * np.array([[1.0, 2.0, -1.0]])
    S = R.local_shape(t.astype(np.float32), 7.5)
    d = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    assert S['valid'].all() and S['n'].min() == 4 and S['n'].max() == 7
    assert np.abs(np.abs(S['axis'] @ d) - 1.0).max() <= 1e-15
    assert np.abs(S['linearity'] - 1.0).max() <= 1e-15
    assert (S['axis'][:, 1] > 0).all()                                           # the largest component, y, is positive
    small = S['eigenvalues'][:, 1:]
    assert np.abs(small).max() <= 8 * np.finfo(np.float64).eps * S['eigenvalues'][:, 0].max()


def test_counts_and_degenerate_neighbourhoods():
    dup = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    S = R.local_shape(dup, 0.5)
    assert (S['moments'] == np.array([300] + [0] * 9)).all()
    assert (S['flags'] == R.FLAG_POINT).all() and not S['valid'].any() and (S['eigenvalues'] == 0.0).all() and np.isnan(S['linearity']).all()
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    S = R.local_shape(one, 1.0)
    assert S['n'].tolist() == [1] and S['flags'].tolist() == [R.FLAG_FEW] and not S['valid'][0]
    two = np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], np.float32)
    S = R.local_shape(two, 1.0)
    assert S['n'].tolist() == [2, 2] and S['flags'].tolist() == [R.FLAG_FEW] * 2 and not S['valid'].any() and (S['eigenvalues'][:, 0] > 0).all()
    S = R.local_shape(np.array([[50.0, 0.0, 0.0]], np.float32), 1.0, other=two)   # nothing near
    assert S['n'].tolist() == [0] and S['flags'].tolist() == [R.FLAG_EMPTY] and np.isnan(S['eigenvalues']).all() and (S['vectors'] == 0.0).all()
    for bad in (0.0, -1.0, np.nan, np.inf, 2.0 ** 40 * 1.0000001, 1e-170):
        with pytest.raises(ValueError):
            R.scale(bad)
    assert R.scale(2.0 ** 40)[1] == 2.0 ** 40 and R.scale(3.0)[1:] == (4.0, 2.0 ** 16, 2.0 ** -16) and R.scale(0.75)[1] == 1.0


def test_invariances():
    P = R.mixed(900, 3)
    ref = R.local_shape(P, 5.0)
    perm = np.random.default_rng(0).permutation(len(P))
    S = R.local_shape(P[perm], 5.0)
    assert np.array_equal(S['moments'], ref['moments'][perm])                    # the order of the cloud
    S = R.local_shape(P, 5.0, other=P)
    R.same_as_restatement(S, ref)                                                # auto equals cross with itself
    Pq = (np.round(P.astype(np.float64) * 16.0) / 16.0).astype(np.float32)       # multiples of 1/16: exact in float32 at 10^6 as well
    far = (Pq.astype(np.float64) + 1.0e6).astype(np.float32)
    assert np.array_equal(far.astype(np.float64) - 1.0e6, Pq.astype(np.float64))
    R.same_as_restatement(R.local_shape(far, 5.0), R.local_shape(Pq, 5.0))      # a translation that is exact in float32


def _eigvalsh_difference(S, radius):
    M = S['moments']
    C = R.covariance(M)
    step = R.scale(radius)[3]
    A = np.zeros((len(M), 3, 3))
    for (i, j), c in zip([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)], C):
        A[:, i, j] = A[:, j, i] = c
    ok = S['eigenvalues'][:, 0] > 0
    w = np.linalg.eigvalsh(A[ok])[:, ::-1] * step * step
    return float((np.abs(w - S['eigenvalues'][ok]).max(1) / S['eigenvalues'][ok][:, 0]).max())


def test_eigenvalues_against_eigvalsh(shells):
    """|eigenvalue - np.linalg.eigvalsh| relative to the largest eigenvalue, over the three shells and two mixed clouds (one of them 10^6
    from the origin).  Seen on the restatement: 1.12e-15, 1.25e-15, 1.18e-15 on the shells, 1.14e-15 and 1.50e-15 on the mixed clouds; the
    bound is 16 x the largest of them."""
    seen = [_eigvalsh_difference(S, r) for _, r, S in shells.values()]
    seen.append(_eigvalsh_difference(R.local_shape(R.mixed(3000, 5), 6.0), 6.0))
    seen.append(_eigvalsh_difference(R.local_shape(R.mixed(2000, 6, 1.0e6), 5.0), 5.0))
    print('eigvalsh differences', seen)
    assert max(seen) <= 16 * EIGVALSH_SEEN


def shell_angles(P, normals):
    rad = P.astype(np.float64)
    rad /= np.linalg.norm(rad, axis=1)[:, None]
    return np.degrees(np.arccos(np.minimum(1.0, np.abs((normals * rad).sum(1)))))


@pytest.mark.parametrize('name', list(SHELLS))
def test_sphere_shell_normals(shells, name):
    """the normal against the radial direction on a noisy shell (R 100, sigma 3), up to sign: the median and the maximum angle stay within
    1.5 x what the restatement was measured at (local_shape_ref.SHELL_ANGLES)"""
    P, r, S = shells[name]
    assert S['valid'].all()
    ang = shell_angles(P[:len(S['n'])], S['normal'])
    print(name, 'median %.4f max %.4f' % (np.median(ang), ang.max()))
    assert np.median(ang) <= R.ANGLE_FACTOR * R.SHELL_ANGLES[name][0] and ang.max() <= R.ANGLE_FACTOR * R.SHELL_ANGLES[name][1]
    assert (S['planarity'] > S['linearity']).mean() > 0.9 and np.nanmedian(S['scattering']) < 0.2


def test_the_viewpoint_orients_the_normals(shells):
    """a viewpoint at the sphere's centre makes every normal point inward; turned round, outward"""
    P, r, S = shells['2000_r50']
    V = R.shape(S['moments'], r, P, viewpoint=(0.0, 0.0, 0.0))
    inward = (V['vectors'][:, 2] * P.astype(np.float64)).sum(1)
    assert (inward < 0).all()
    outward = -V['vectors'][:, 2]
    assert ((outward * P.astype(np.float64)).sum(1) > 0).all()
    assert np.array_equal(np.abs(V['vectors']), np.abs(S['vectors'])) and np.array_equal(V['eigenvalues'], S['eigenvalues'])
    turned = (V['flags'] & R.FLAG_TURNED) != 0
    assert 0 < turned.sum() < len(P) and np.array_equal(V['vectors'][~turned], S['vectors'][~turned])
    assert np.array_equal(V['vectors'][turned, 2], -S['vectors'][turned, 2]) and np.array_equal(V['vectors'][:, :2], S['vectors'][:, :2])


def test_three_mutations_are_caught():
    L = R.lattice(7)
    c = np.array([[3.0, 3.0, 3.0]], np.float32)
    assert R.moments(c, 2.0, other=L)[0, 0] == 33 and R.moments(c, 2.0, other=L, mutate='open_ball')[0, 0] == 27        # < for <=
    P = R.mixed(600, 9)
    ref = R.local_shape(P, 5.0)
    cut = R.local_shape(P, 5.0, mutate='no_rint')                               # a dropped rint
    assert np.array_equal(cut['n'], ref['n']) and not np.array_equal(cut['moments'], ref['moments'])
    swapped = R.local_shape(P, 5.0, mutate='order')                             # a swapped rotation order
    assert np.array_equal(swapped['moments'], ref['moments'])
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert not np.array_equal(bits(swapped['eigenvalues']), bits(ref['eigenvalues'])) or not np.array_equal(bits(swapped['vectors']), bits(ref['vectors']))
    assert np.abs(swapped['eigenvalues'] - ref['eigenvalues']).max() <= 1e-12 * ref['eigenvalues'].max()               # the same matrix all the same
