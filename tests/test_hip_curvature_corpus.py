"""GPU: the block-boundary curvature kernel (nw_curvature through MembraneMesh.curvature_grad_c) against the oracle's restatement
(oracle/nw_oracle.c: nwo_curvature_grad) on the meshes a fit produces, not only on the golden sphere of tests/test_curvature.py:
synthetic networks of several components, remeshed meshes with irregular valences, an open border, spare vertex slots, a full 20-slot ring,
coordinates far from the origin, non-default energy parameters, and a mesh taken from the middle of a fit (the device-resident fast path).

Both sides get the same float32 positions and normals, the same ring order and an explicit seeded jitter array.  All twelve outputs are held
to the golden test's tolerance (rtol 2e-5, atol 1e-7 max|ref|), no output excepted; the largest deviation of each is printed (run with -s)."""
import functools
import zlib

import numpy as np
import pytest

from curvature_ref import NAMES, tables, oracle_curvature, oracle_of_mesh, device_outputs, deviations, assert_close
from ch_shrinkwrap_amd.membrane_mesh import MembraneMesh
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere, geodesic_sphere
from ch_shrinkwrap_amd import synth

pytestmark = pytest.mark.gpu

F32 = np.float32
OFFSETS = {'origin': (0.0, 0.0, 0.0), 'offset_4e4': (4e4, 3e4, 1e3), 'offset_2e5': (2e5, -1.5e5, 1e5)}
# (kc, kg, c0, dN): the recipe's kc with the upstream kg, a spontaneous curvature, and two finite-difference steps
PARAMS = [(1.0, -20.0 * 0.0257, 0.02, 0.1), (20.0 * 0.0257, -0.3, -0.01, 1.0)]


def uv_sphere(n_lon, n_lat=12, radius=60.0):
    """latitude-longitude sphere: each pole has valence n_lon"""
    th = np.linspace(0.0, np.pi, n_lat + 1)[1:-1]
    ph = np.arange(n_lon) * 2.0 * np.pi / n_lon
    T, P = np.meshgrid(th, ph, indexing='ij')
    ring = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    v = radius * np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]])
    south = v.shape[0] - 1
    idx = lambda i, j: 1 + i * n_lon + (j % n_lon)
    f = []
    for j in range(n_lon):
        f.append([0, idx(0, j), idx(0, j + 1)])
        f.append([south, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)])
    for i in range(n_lat - 2):
        for j in range(n_lon):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [[a, b, c], [a, c, d]]
    return v, np.array(f, np.int32)


def _remeshed(device):
    from ch_shrinkwrap_amd.remesh import remesh, remesh_device
    c = synth.make_config('c5', scale=0.02)
    v, f = c['vertices'], np.ascontiguousarray(c['faces'], np.int32)
    mean = float(np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean())
    # coarsened with no relaxation: collapses and flips leave valences from 3 up
    if device:
        nv, nf = remesh_device(v, f, 5, 1.8 * mean, 0.5, 0)
    else:
        nv, nf = remesh(v, f, 5, 1.8 * mean, 0.5, 0)
    return nv, nf


@functools.lru_cache(maxsize=None)
def corpus_mesh(name):
    """(vertices float64 (V,3), faces int32) of a corpus case; vertices no face refers to are spare slots (valid = 0)"""
    if name == 'icosphere':
        v, f = icosphere(3, 100.0)
        v = v * (1.0 + 0.05 * np.sin(np.asarray(v, 'f8')[:, :1] * 0.07))
    elif name == 'geodesic':
        v, f = geodesic_sphere(12, 150.0)
    elif name == 'network_c5':
        c = synth.make_config('c5', scale=0.02)
        v, f = c['vertices'], c['faces']
    elif name == 'remesh_device':
        v, f = _remeshed(True)
    elif name == 'remesh_host':
        v, f = _remeshed(False)
    elif name == 'half_sphere':
        v, f = icosphere(3, 100.0)
        f = f[: f.shape[0] // 2]                                    # an open border; the other half's vertices are unreferenced slots
    elif name == 'spare_slots':
        v, f = geodesic_sphere(8, 80.0)
        extra = np.random.default_rng(7).uniform(-80.0, 80.0, (97, 3))
        v = np.concatenate([np.asarray(v, 'f8'), extra])           # max_vertices > used: slots no face refers to
    elif name == 'uv_pole20':
        v, f = uv_sphere(20)
    else:
        raise KeyError(name)
    return np.asarray(v, 'f8'), np.ascontiguousarray(f, np.int32)


CASES = ['icosphere', 'geodesic', 'network_c5', 'remesh_device', 'remesh_host', 'half_sphere', 'spare_slots', 'uv_pole20']


def _at(name, offset):
    v, f = corpus_mesh(name)
    return (v + np.asarray(OFFSETS[offset])).astype(F32), f


@pytest.mark.parametrize('offset', list(OFFSETS))
@pytest.mark.parametrize('case', CASES)
def test_curvature_kernel_equals_the_oracle_on_the_corpus(case, offset, monkeypatch):
    v, f = _at(case, offset)
    valence = np.bincount(f.ravel(), minlength=v.shape[0])
    used = valence > 0
    print('\n%s at %s: %d vertices (%d spare), %d faces, valence %d..%d'
          % (case, offset, v.shape[0], (~used).sum(), f.shape[0], valence[used].min(), valence[used].max()))
    if case == 'uv_pole20':
        assert valence.max() == 20                                   # the ring row is full: no -1 terminator
    if case == 'remesh_device' or case == 'remesh_host':
        assert valence[used].min() <= 4 and valence.max() >= 8
    if case == 'half_sphere':
        from ch_shrinkwrap_amd.surgery import twins
        assert (twins(f, v.shape[0]) < 0).sum() > 0                 # an open border
    if case == 'spare_slots':
        assert (~used).sum() > 0
    rng = np.random.default_rng(zlib.crc32(('%s/%s' % (case, offset)).encode()))
    for host in ('1', '0'):
        monkeypatch.setenv('NW_HOST_TABLES', host)
        for p, (kc, kg, c0, dN) in enumerate(PARAMS):
            m = MembraneMesh(v, f, kc=kc, kg=kg, c0=c0)
            jit = rng.random((v.shape[0], 3))
            got = device_outputs(m, m.curvature_grad_c(dN=dN, jitter=jit))
            ref = oracle_of_mesh(m, jit, dN)
            dev = deviations(got, ref)
            same = [n for n in NAMES if np.array_equal(got[n], ref[n], equal_nan=True)]
            print('  host_tables=%s params=%d: %s; bit-identical: %d of 12'
                  % (host, p, ', '.join('%s %.2e' % (n, dev[n][0]) for n in NAMES), len(same)))
            assert_close(got, ref, '%s %s host_tables=%s params=%d' % (case, offset, host, p))
            assert np.abs(got['H'][used]).max() > 0                 # (something was computed)


@pytest.mark.parametrize('host', ['1', '0'])
def test_a_vertex_of_valence_21_is_refused(host, monkeypatch):
    """The 1-ring table has 20 slots: a pole of valence 21 cannot be represented and must not be computed on a truncated ring."""
    monkeypatch.setenv('NW_HOST_TABLES', host)
    v, f = uv_sphere(21)
    m = MembraneMesh(v.astype(F32), f)
    with pytest.raises(ValueError):
        m.curvature_grad_c(dN=0.1, jitter=np.zeros((v.shape[0], 3)))


def test_fast_path_in_a_fit_equals_the_oracle_and_selects_the_same_necks(monkeypatch):
    """A short fit (c2, remesher None) with the neck traits on: at every block boundary, while the device-resident fast path is live
    (positions of the block's last iteration, normals refreshed on the device), the curvature it produced is compared with the oracle on
    the device's positions (`cg.fs`) and refreshed normals (`mesh.vertex_normals`)."""
    monkeypatch.setenv('NW_HOST_TABLES', '0')
    c = synth.make_config('c2', scale=0.1, seed=5)
    lo, hi = -1e-3, 1e-2                                            # the recipe's thresholds (ShrinkwrapMembrane)
    m = MembraneMesh(c['vertices'].copy(), c['faces'], kc=1.0, step_size=20.0, max_iter=20, remesh_frequency=5, delaunay_remesh_frequency=0,
                     neck_first_iter=1, neck_threshold_low=lo, neck_threshold_high=hi)
    m.remesher = None
    m._warned_fixed_topology = True
    checks, removed = [], []
    original = m.neck_vertices

    def checked_neck_vertices(low, high):
        key = m._native.mesh_key
        assert m._in_fit and key is not None and key[0] == id(m)
        verts = original(low, high)
        assert m._native.mesh_key == key                           # nothing was uploaded: the fast path ran
        K_fast = np.array(m._K)
        pos = np.array(m.cg.fs, F32)
        nrm = np.array(m.vertex_normals, F32)
        # the oracle's tables from the device's positions (face areas in float32 as the kernel builds them)
        t = TriMesh(pos, np.asarray(m.faces))
        nbr, nxt, area = tables(t)
        valid = (t._vertices['halfedge'] != -1).astype('u1')
        ref_hash = oracle_curvature(pos, nrm, valid, nbr, nxt, area, None, 0.1, float(m.kc), float(m.kg), float(m.c0))
        # the selection: equal to the oracle-K selection except for vertices whose oracle K lies within the tolerance band of a threshold
        K = ref_hash['K']
        tol = lambda thr: 2e-5 * abs(thr) + 1e-7 * max(1.0, float(np.abs(K).max()))
        sel_ref = (K < low) | (K > high)
        band = (np.abs(K - low) <= tol(low)) | (np.abs(K - high) <= tol(high))
        sel = np.zeros(K.shape[0], bool)
        sel[verts] = True
        differ = sel != sel_ref
        assert not (differ & ~band).any()
        assert np.allclose(K_fast, K, rtol=2e-5, atol=1e-7 * max(1.0, float(np.abs(K).max())))
        # all twelve outputs with an explicit jitter, still on the fast path
        jit = np.random.default_rng(len(checks)).random((pos.shape[0], 3))
        got = device_outputs(m, m.curvature_grad_c(dN=0.1, jitter=jit))
        assert m._native.mesh_key == key
        ref = oracle_curvature(pos, nrm, valid, nbr, nxt, area, jit, 0.1, float(m.kc), float(m.kg), float(m.c0))
        dev = deviations(got, ref)
        checks.append(dict(iteration=m._neck_iteration, selected=int(sel.sum()), near_threshold=int(band.sum()), differ=int(differ.sum())))
        print('\nfit boundary %d: %d selected, %d near a threshold, %d decided differently; %s'
              % (m._neck_iteration, sel.sum(), band.sum(), differ.sum(), ', '.join('%s %.2e' % (n, dev[n][0]) for n in NAMES)))
        assert_close(got, ref, 'fit boundary %d' % m._neck_iteration)
        return verts

    m.neck_vertices = checked_neck_vertices
    m.neck_remover = lambda mesh, ids: removed.append(np.array(ids))   # (selection seen by the hook; the mesh is not changed)
    m.shrink_wrap(c['points'], c['sigma'])
    assert [r['iteration'] for r in checks] == [5, 10, 15, 20]
    assert sum(r['near_threshold'] for r in checks) <= 1e-3 * m.vertices.shape[0] * len(checks)
    assert all(r['differ'] <= r['near_threshold'] for r in checks)


def test_curvature_after_a_fit_sees_positions_edited_by_the_caller():
    """After a fit the device copy is stale: editing mesh.vertices in place and reading the curvature must give the edited mesh's curvature."""
    from ch_shrinkwrap_amd.synth import sphere_cloud
    v, f = icosphere(4, 100.0)
    pts = sphere_cloud(20000, 100.0, 5.0, seed=2)
    m = MembraneMesh(v.copy(), f, kc=1.0, step_size=20.0, max_iter=5, remesh_frequency=0, delaunay_remesh_frequency=0)
    m.shrink_wrap(pts, np.full(pts.shape, 5.0, 'f4'))
    m.vertices[:] *= F32(1.1)
    K = np.array(m.curvature_gaussian)
    ref = oracle_of_mesh(m, None, 0.1)
    assert np.allclose(K, ref['K'], rtol=2e-5, atol=1e-7 * max(1.0, float(np.abs(ref['K']).max())))
    assert abs(np.mean(K) * 110.0 ** 2 - 1.0) < 0.15                # a sphere of radius 110 now
