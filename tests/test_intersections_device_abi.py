"""CPU test: libnanowrap_hip.so exports every function include/nw_intersections.h declares, the binding names the same set, the unit is
built without fma contraction, its kernels stay within their budgets without scratch, and the calls check their arguments before they
touch a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_mx_count', 'k_mx_emit', 'k_mx_stats', 'k_mx_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_intersections.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwx_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_intersections_header():
    from ch_shrinkwrap_amd import build, _lib, intersections
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) == 8
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(intersections.SYMBOLS) == names
    assert intersections.load().nwx_abi_version() == intersections.ABI_VERSION == 1
    # the constants the binding repeats
    txt = open(os.path.join(ROOT, 'include', 'nw_intersections.h')).read()
    for name in ('NWX_PAIRS', 'NWX_STATS', 'NWX_MAX_PAIRS'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(intersections, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH', 'TOOMANY', 'NOPAIRS'):
        assert int(re.search(r'NWX_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(intersections, 'NWX_ERR_' + name)
        assert getattr(intersections, 'NWX_ERR_' + name) in intersections.ERRORS


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_INTERSECTIONS]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    deps = unit[0][2]
    assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_intersections_core.h') in deps          # rebuilt when the core changes
    assert os.path.join(ROOT, 'include', 'nw_intersections.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_INTERSECTIONS in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_INTERSECTIONS)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert not [k for k in build.KERNEL_BUDGETS if k.startswith('k_mx_') and k not in KERNELS]
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)


def test_the_distance_unit_is_left_alone():
    """the check is a unit of its own: nothing of it is in nw_distance.o, and its core includes no other unit's"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    assert not [k for k in build.kernel_resources(build.OBJ_DISTANCE) if k.startswith('k_mx_')]
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_intersections_core.h')).read()
    # HIP-free: the standard headers and the query units' shared HIP-free core (the one definition of a face's centroid and radius)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['cmath', 'cstdint', 'nw_bq_core.h']
    shared = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_bq_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', shared) == ['cstdint', 'cmath', 'algorithm']


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the mesh and of the flags comes before the first use of
    the context."""
    from ch_shrinkwrap_amd import intersections as X
    L = X.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros((4, 3), np.float32)
    pos[1, 0] = pos[2, 1] = pos[3, 2] = 10.0
    faces = np.array([[0, 2, 1], [0, 1, 3]], np.int32)
    assert L.nwx_set_mesh(None, p(pos), 4, p(faces), 2) == X.NWX_ERR_BADARG                              # all is well but the context
    assert L.nwx_set_mesh(None, None, 4, p(faces), 2) == X.NWX_ERR_BADARG
    assert L.nwx_set_mesh(None, p(pos), 4, None, 2) == X.NWX_ERR_BADARG
    assert L.nwx_set_mesh(None, p(pos), 4, p(faces), 0) == X.NWX_ERR_BADARG
    assert L.nwx_set_mesh(None, p(pos), 2, p(faces), 2) == X.NWX_ERR_BADARG
    assert L.nwx_set_mesh(None, p(pos), 4, p(np.array([[0, 1, 4], [0, 1, 2]], np.int32)), 2) == X.NWX_ERR_BADARG
    assert L.nwx_set_mesh(None, p(pos), 4, p(np.array([[0, 1, -1], [0, 1, 2]], np.int32)), 2) == X.NWX_ERR_BADARG
    nan = pos.copy()
    nan[2, 1] = np.inf
    assert L.nwx_set_mesh(None, p(nan), 4, p(faces), 2) == X.NWX_ERR_NONFINITE
    n = ctypes.c_int64()
    assert L.nwx_find(None, 4, None, ctypes.byref(n), ctypes.byref(n)) == X.NWX_ERR_BADARG               # an unknown flag
    assert L.nwx_find(None, 0, None, ctypes.byref(n), ctypes.byref(n)) == X.NWX_ERR_BADARG               # no context
    out = np.full((4, 2), -7, np.int32)
    assert L.nwx_get_pairs(None, p(out), 4) == X.NWX_ERR_BADARG and (out == -7).all()
    assert L.nwx_get_stats(None, p(np.zeros(2, np.int64))) == X.NWX_ERR_BADARG
    h = ctypes.c_void_p()
    assert L.nwx_create(-1, ctypes.byref(h)) == X.NWX_ERR_BADARG and L.nwx_create(0, None) == X.NWX_ERR_BADARG


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import intersections as X
    from ch_shrinkwrap_amd import evaluation
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    with pytest.raises(RuntimeError):
        X.self_intersections((v, f))
    with pytest.raises(RuntimeError):
        TriMesh(v, f).self_intersections()
    with pytest.raises(RuntimeError):
        evaluation.mesh_properties(TriMesh(v, f), self_intersections=True)
