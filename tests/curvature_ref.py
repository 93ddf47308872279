"""The oracle's restatement of the block-boundary curvature kernel (oracle/nw_oracle.c: nwo_curvature_grad), bound for tests that compare
the HIP kernel with it (tests/test_curvature.py, tests/test_hip_curvature_corpus.py).  Its ring tables are built here from the half-edge
records with NumPy, independently of the library's table builders."""
import ctypes
import numpy as np

NAMES = ['k0', 'k1', 'e0', 'e1', 'H', 'K', 'dH', 'dK', 'E', 'pE', 'dEn', 'dEdN']
ATTRS = dict(k0='_k_0', k1='_k_1', e0='_e_0', e1='_e_1', H='_H', K='_K', dH='_dH', dK='_dK', E='_E', pE='_pE', dEn='_dE_neighbors')


def tables(m):
    """(1-ring vertex ids, vertex the next half-edge points to, area of the half-edge's face): (M, NB) each, -1 / 0 padded"""
    he, nb = m._halfedges, m._vertices['neighbors']
    ok = nb != -1
    safe = np.where(ok, nb, 0)
    ring = he['vertex'][safe]
    ring[~ok] = -1
    nxt = he['vertex'][he['next'][safe]]
    nxt[~ok] = -1
    area = m._faces['area'][he['face'][safe]]
    area[~ok] = 0
    return np.ascontiguousarray(ring, 'i4'), np.ascontiguousarray(nxt, 'i4'), np.ascontiguousarray(area, 'f4')


def oracle_curvature(pos, nrm, valid, nbr, nxt, area, jitter, dN, kc, kg, c0):
    """nwo_curvature_grad on host arrays; jitter (M,3) float64 or None (the counter hash the kernel also uses).  Returns the twelve outputs."""
    from oracle import nanowrap_oracle as O
    M, NB = nbr.shape
    shp = {'e0': (M, 3), 'e1': (M, 3), 'dEdN': (M, 3)}
    o = {n: np.zeros(shp.get(n, (M,)), 'f4') for n in NAMES}
    L = O.lib()
    f32 = ctypes.c_float
    L.nwo_curvature_grad.restype = None
    L.nwo_curvature_grad.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int, ctypes.c_int, f32, f32, f32, f32] + [ctypes.c_void_p] * 12
    keep = [np.ascontiguousarray(pos, 'f4'), np.ascontiguousarray(nrm, 'f4'), np.ascontiguousarray(valid, 'u1'), np.ascontiguousarray(nbr, 'i4'),
            np.ascontiguousarray(nxt, 'i4'), np.ascontiguousarray(area, 'f4'), None if jitter is None else np.ascontiguousarray(jitter, 'f8')]
    assert all(a.shape[0] == M for a in keep if a is not None)
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    L.nwo_curvature_grad(*[P(a) for a in keep], M, NB, dN, kc, kg, c0, *[P(o[n]) for n in NAMES])
    return o


def oracle_of_mesh(m, jitter, dN, pos=None, nrm=None):
    """the oracle on a TriMesh / MembraneMesh as it stands (positions, vertex normals, valid = slots with a half-edge)"""
    nbr, nxt, area = tables(m)
    pos = np.ascontiguousarray(m._vertices['position'] if pos is None else pos, 'f4')
    nrm = np.ascontiguousarray(m.vertex_normals if nrm is None else nrm, 'f4')
    valid = (m._vertices['halfedge'] != -1).astype('u1')
    return oracle_curvature(pos, nrm, valid, nbr, nxt, area, jitter, dN, float(m.kc), float(m.kg), float(m.c0))


def device_outputs(m, dEdN):
    out = {n: np.array(getattr(m, a)) for n, a in ATTRS.items()}
    out['dEdN'] = np.array(dEdN)
    return out


def deviations(got, ref):
    """{output: (largest |got - ref|, the tolerance it is held to)} at the golden test's tolerance: rtol 2e-5, atol 1e-7 max|ref|"""
    res = {}
    for n in NAMES:
        a, b = np.asarray(got[n], 'f8'), np.asarray(ref[n], 'f8')
        fin = np.isfinite(b)
        d = np.abs(a - b)[fin]
        res[n] = (float(d.max()) if d.size else 0.0, float(1e-7 * max(1.0, np.abs(b[fin]).max() if fin.any() else 0.0)))
    return res


def assert_close(got, ref, where=''):
    for n in NAMES:
        a, b = got[n], ref[n]
        assert np.allclose(a, b, rtol=2e-5, atol=1e-7 * max(1.0, np.nanmax(np.abs(b)) if np.isfinite(b).any() else 1.0), equal_nan=True), '%s %s' % (where, n)
