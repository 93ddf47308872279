"""CPU test: libnanowrap_hip.so exports every function include/nw_distance.h declares, the binding names the same set, the unit is built
without fma contraction, its kernels stay within their budgets without scratch, and the calls check their arguments before they touch a
GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_md_query', 'k_md_sum_final']              # (the set-up kernels are the face grid's: k_bq_face_setup, k_bq_rho_reduce of nw_bq.o)


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_distance.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwd_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_distance_header():
    from ch_shrinkwrap_amd import build, _lib, distance
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) == 6
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(distance.SYMBOLS) == names
    assert distance.load().nwd_abi_version() == distance.ABI_VERSION == 1
    # the constants the binding repeats
    txt = open(os.path.join(ROOT, 'include', 'nw_distance.h')).read()
    for name, value in (('NWD_SIGNED', distance.NWD_SIGNED), ('NWD_RINGS', distance.NWD_RINGS), ('NWD_FEATURE_MASK', distance.FEATURE_MASK),
                        ('NWD_FEATURE_CAPPED', distance.FEATURE_CAPPED)):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == value
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH'):
        assert int(re.search(r'NWD_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(distance, 'NWD_ERR_' + name)


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_DISTANCE]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_distance_core.h') in unit[0][2]             # rebuilt when the core changes
    assert build.OBJ_DISTANCE in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_DISTANCE)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert not [k for k in build.KERNEL_BUDGETS if k.startswith('k_md_') and k not in KERNELS]
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the mesh, of the twin table and of the query's arguments
    comes before the first use of the context."""
    from ch_shrinkwrap_amd import distance as D
    L = D.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros((4, 3), np.float32)
    pos[1, 0] = pos[2, 1] = pos[3, 2] = 10.0
    faces = np.array([[0, 2, 1], [0, 1, 3]], np.int32)
    twin = np.array([-1, -1, 3, 2, -1, -1], np.int32)
    twin[[2, 3]] = [3, 2]
    assert L.nwd_set_mesh(None, p(pos), 4, p(faces), 2, p(twin)) == D.NWD_ERR_BADARG                 # all is well but the context
    assert L.nwd_set_mesh(None, None, 4, p(faces), 2, None) == D.NWD_ERR_BADARG
    assert L.nwd_set_mesh(None, p(pos), 4, p(faces), 0, None) == D.NWD_ERR_BADARG
    assert L.nwd_set_mesh(None, p(pos), 4, p(np.array([[0, 1, 4], [0, 1, 2]], np.int32)), 2, None) == D.NWD_ERR_BADARG
    for bad in ([-1, -1, 3, 1, -1, -1], [-1, -1, 6, -1, -1, -1], [-1, -1, -2, -1, -1, -1], [1, 2, 0, -1, -1, -1]):
        assert L.nwd_set_mesh(None, p(pos), 4, p(faces), 2, p(np.array(bad, np.int32))) == D.NWD_ERR_BADARG
    nan = pos.copy()
    nan[2, 1] = np.nan
    assert L.nwd_set_mesh(None, p(nan), 4, p(faces), 2, None) == D.NWD_ERR_NONFINITE
    q = np.zeros((4, 3))
    s = ctypes.c_double()
    assert L.nwd_query(None, None, 4, 0, None, None, None, None, ctypes.byref(s)) == D.NWD_ERR_BADARG
    assert L.nwd_query(None, p(q), 0, 0, None, None, None, None, ctypes.byref(s)) == D.NWD_ERR_BADARG
    assert L.nwd_query(None, p(q), 4, 4, None, None, None, None, ctypes.byref(s)) == D.NWD_ERR_BADARG           # an unknown flag
    assert L.nwd_query(None, p(q), 4, 0, None, None, None, None, ctypes.byref(s)) == D.NWD_ERR_BADARG           # no context
    h = ctypes.c_void_p()
    assert L.nwd_create(-1, ctypes.byref(h)) == D.NWD_ERR_BADARG and L.nwd_create(0, None) == D.NWD_ERR_BADARG


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import distance as D
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    with pytest.raises(RuntimeError):
        D.distance_to_mesh(np.zeros((10, 3)), TriMesh(v, f))
    with pytest.raises(RuntimeError):
        TriMesh(v, f).signed_distance(np.zeros((10, 3)))
    with pytest.raises(RuntimeError):
        D.DistanceToMesh().execute({'membrane': TriMesh(v, f), 'filtered_localizations': {'x': np.zeros(3), 'y': np.zeros(3), 'z': np.zeros(3)}})
    with pytest.raises(AttributeError):
        D.DistanceToMesh(backend='host')


def test_twins_of_a_mesh_come_from_its_half_edges():
    from ch_shrinkwrap_amd import distance as D
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    import mesh_distance_ref as R
    v, f = icosphere(1, 10.0)
    pos, faces, twin = D._mesh_arrays(TriMesh(v, f), True)
    assert np.array_equal(twin, R.twins(f)) and np.array_equal(D._mesh_arrays((v, f), True)[2], twin)
    assert D._mesh_arrays((v, f), False)[2] is None
    v, f = R.disk()
    assert np.array_equal(D._mesh_arrays((v, f), True)[2], R.twins(f))
    # an edge with three faces has no twin table: the pairing's error is passed on, from a face array and from a TriMesh, whose sort-based
    # pairing of such faces is not mutual
    f3 = np.array([[0, 1, 2], [1, 0, 3], [1, 0, 4]], np.int32)
    v5 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    with pytest.raises(RuntimeError, match='nwr_halfedge_twins'):
        D._mesh_arrays((v5, f3), True)
    with pytest.raises(ValueError, match='non-manifold'):
        D._mesh_arrays(TriMesh(v5, f3), True)
    assert D._mesh_arrays(TriMesh(v5, f3), False)[2] is None
    # half-edge records without a 'twin' field (the multi-GPU layer's mesh has only 'vertex') are not trusted: the faces are paired
    v, f = icosphere(1, 10.0)
    duck = type('M', (), {'vertices': v, 'faces': f, '_halfedges': np.zeros(3 * len(f), [('vertex', 'i4')])})()
    assert np.array_equal(D._mesh_arrays(duck, True)[2], R.twins(f))
