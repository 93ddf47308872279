"""The mirrors of upstream's evaluation recipe modules (recipe_modules/surface_feature_extraction.py:76-167): table shapes and column names
on the host, MeshProperties' topology columns on a sphere, a torus and two spheres with the host labeller.  The device parts (the default
labeller, backend='device') are in tests/test_hip_evaluation.py."""
import numpy as np
import pytest

from ch_shrinkwrap_amd import evaluation as E
from ch_shrinkwrap_amd import surgery
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere


def torus(R=100.0, r=30.0, nu=48, nv=24):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing='ij')
    pos = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3).astype('f4')
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    a, b = i * nv + j, ((i + 1) % nu) * nv + j
    c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype('i4')
    return pos, faces


def two_spheres():
    v, f = icosphere(3, 50.0)
    return np.concatenate([v, v + np.array([200.0, 0, 0], 'f4')]).astype('f4'), np.concatenate([f, f + len(v)]).astype('i4')


CASES = {
    # name: (mesh, euler, genus, components, area, volume)
    'sphere': (icosphere(4, 100.0), 2, 0, 1, 4 * np.pi * 100.0 ** 2, 4 / 3 * np.pi * 100.0 ** 3),
    'torus': (torus(), 0, 1, 1, 4 * np.pi ** 2 * 100.0 * 30.0, 2 * np.pi ** 2 * 100.0 * 30.0 ** 2),
    'two_spheres': (two_spheres(), 4, 0, 2, 2 * 4 * np.pi * 50.0 ** 2, 2 * 4 / 3 * np.pi * 50.0 ** 3),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_mesh_properties_topology_on_the_host(name):
    (v, f), euler, genus, comps, area, volume = CASES[name]
    mesh = TriMesh(v, f)
    t = E.MeshProperties(label_faces=surgery.scipy_label_faces).execute({'membrane': mesh})
    assert sorted(t) == ['area', 'components', 'euler', 'genus', 'manifold', 'volume']
    assert all(np.asarray(c).shape == (1,) for c in t.values())
    assert (t['euler'][0], t['genus'][0], t['manifold'][0], t['components'][0]) == (euler, genus, 1, comps)
    assert mesh.euler == mesh.euler_characteristic == euler and mesh.manifold is True
    # the inscribed polyhedra are a little smaller than the smooth surfaces (edges of 8 nm on radii of 30 nm and more)
    assert 0.95 * area < t['area'][0] <= area and 0.93 * volume < t['volume'][0] <= volume


def test_manifold_flags_a_pinched_vertex_and_an_open_border():
    v, f = two_spheres()
    f = f.copy()
    f[f == f.max()] = 0                                        # the two spheres now share vertex 0: two closed fans at one vertex
    top = E.mesh_topology(f, len(v))
    assert top['manifold'] is False
    v, f = icosphere(3, 50.0)
    top = E.mesh_topology(f[:-1], len(v))                      # one face removed: still a manifold, with one border loop
    assert top['manifold'] is True and top['border_loops'] == 1 and top['euler'] == 1
    flipped = f.copy()
    flipped[5] = flipped[5, ::-1]                              # one face wound the other way: its directed edges occur twice
    assert E.mesh_topology(flipped, len(v))['manifold'] is False


def test_points_and_distance_tables_on_the_host():
    v, f = icosphere(3, 100.0)
    ns = {'membrane0': TriMesh(v, f)}
    t = E.PointsFromMesh(dx_min=4.0).execute(ns)
    assert ns['membrane0_localizations'] is t and sorted(t) == ['x', 'xn', 'y', 'yn', 'z', 'zn']
    pts = E.points_from_mesh(ns['membrane0'], dx_min=4.0)
    assert np.array_equal(np.stack([t['x'], t['y'], t['z']], 1), pts) and pts.shape[0] > 5000
    nrm = np.stack([t['xn'], t['yn'], t['zn']], 1)
    assert nrm.shape == pts.shape and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
    # on a sphere about the origin the face normal at a sample points along the sample
    assert ((nrm * pts).sum(1) / np.linalg.norm(pts, axis=1) > 0.95).all()
    # p < 1: the same draw gives the same rows of both arrays
    d, n = E.points_from_mesh(ns['membrane0'], dx_min=4.0, p=0.3, rng=np.random.default_rng(5), return_normals=True)
    sub = np.random.default_rng(5).choice(pts.shape[0], size=int(0.3 * pts.shape[0]), replace=False)
    assert np.array_equal(d, pts[sub]) and np.array_equal(n, nrm[sub])
    rng = np.random.default_rng(0)
    truth = rng.normal(size=(3000, 3))
    truth = 100.0 * truth / np.linalg.norm(truth, axis=1)[:, None]
    ns.update(filtered_localizations=t, filtered={'x': truth[:, 0], 'y': truth[:, 1], 'z': truth[:, 2]})
    a = E.AverageSquaredDistance().execute(ns)
    assert ns['average_squared_distance'] is a and sorted(a) == ['mse01', 'mse10', 'mse_rms']
    assert all(np.asarray(c).shape == (1,) for c in a.values())
    m0, m1 = E.average_squared_distance(pts, truth)
    assert (a['mse01'][0], a['mse10'][0]) == (m0, m1) and a['mse_rms'][0] == np.sqrt((m0 + m1) / 2)
    with pytest.raises(AttributeError):
        E.PointsFromMesh(spacing=3.0)
