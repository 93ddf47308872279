"""CPU test: libnanowrap_hip.so exports every function include/nw_evaluation.h declares, the binding names the same set, the kernels of
csrc/nw_evaluation.hip and of the point grid it shares with hole punching (csrc/nw_bq.hip) stay within their budgets, and the calls check
their arguments before they touch a GPU."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_ev_face_setup', 'k_ev_node_test', 'k_ev_emit', 'k_ev_nearest', 'k_ev_sum_final']
# the grid's kernels, once this unit's and hole punching's own (k_ev_* / k_hp_bbox, _cell_count, _scatter), with the budgets they had there
GRID_KERNELS = {'k_bq_bbox_f64': (48, 0), 'k_bq_cell_count_f64': (48, 0), 'k_bq_scatter_f64': (16, 0),
                'k_bq_bbox_f32': (32, 0), 'k_bq_cell_count_f32': (32, 0), 'k_bq_scatter_f32': (32, 0)}
SCAN_KERNELS = ['k_bq_scan_tiles', 'k_bq_scan_bsums', 'k_bq_scan_final']
FACE_KERNELS = ['k_bq_face_setup', 'k_bq_rho_reduce']           # the mesh query units' face grid


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_evaluation.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwe_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_evaluation_header():
    from ch_shrinkwrap_amd import build, _lib, evaluation
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) == 8
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(evaluation.SYMBOLS) == names
    assert evaluation.load().nwe_abi_version() == evaluation.ABI_VERSION == 1


def test_evaluation_kernels_are_budgeted_and_within_budget():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    assert build.OBJ_EVALUATION in build.BUDGETED_OBJECTS and build.OBJ_BQ in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_EVALUATION)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert sorted(build.kernel_resources(build.OBJ_BQ)) == sorted(list(GRID_KERNELS) + SCAN_KERNELS + FACE_KERNELS)
    assert not [k for k in build.KERNEL_BUDGETS if k.startswith('k_ev_') and k not in KERNELS]
    for k, budget in GRID_KERNELS.items():
        assert build.KERNEL_BUDGETS[k] == budget, k
    res = build.check_kernel_budgets()
    for k in KERNELS + list(GRID_KERNELS):
        assert k in build.KERNEL_BUDGETS
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every argument check comes before the first use of the context."""
    from ch_shrinkwrap_amd import evaluation as E
    L = E.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros((3, 3), np.float32)
    pos[1, 0] = pos[2, 1] = 10.0
    faces = np.array([[0, 1, 2]], np.int32)
    n = ctypes.c_int64()
    assert L.nwe_sample_mesh(None, p(pos), 3, p(faces), 1, 5.0, ctypes.byref(n)) == E.NWE_ERR_BADARG            # no context
    for dx in (0.0, -1.0, float('nan'), float('inf')):
        assert L.nwe_sample_mesh(None, p(pos), 3, p(faces), 1, dx, ctypes.byref(n)) == E.NWE_ERR_BADARG
    assert L.nwe_sample_mesh(None, p(pos), 3, p(faces), 1, 5.0, None) == E.NWE_ERR_BADARG
    assert L.nwe_sample_mesh(None, p(pos), 3, p(np.array([[0, 1, 3]], np.int32)), 1, 5.0, ctypes.byref(n)) == E.NWE_ERR_BADARG
    cloud = np.zeros((4, 3))
    s = ctypes.c_double()
    assert L.nwe_nearest(None, p(cloud), 0, p(cloud), 4, None, None, ctypes.byref(s)) == E.NWE_ERR_BADARG           # an empty cloud
    assert L.nwe_nearest(None, p(cloud), 4, None, 4, None, None, ctypes.byref(s)) == E.NWE_ERR_BADARG               # NULL with a size
    assert L.nwe_nearest(None, p(cloud), 4, p(cloud), 4, None, None, ctypes.byref(s)) == E.NWE_ERR_BADARG           # no context
    m0, m1 = ctypes.c_double(), ctypes.c_double()
    assert L.nwe_average_squared_distance(None, p(cloud), 4, p(cloud), 4, None, ctypes.byref(m1)) == E.NWE_ERR_BADARG
    assert L.nwe_average_squared_distance(None, p(cloud), 4, p(cloud), -3, ctypes.byref(m0), ctypes.byref(m1)) == E.NWE_ERR_BADARG
    assert L.nwe_get_samples(None, None, None) == E.NWE_ERR_BADARG
    h = ctypes.c_void_p()
    assert L.nwe_create(-1, ctypes.byref(h)) == E.NWE_ERR_BADARG and L.nwe_create(0, None) == E.NWE_ERR_BADARG


def test_the_device_backend_never_falls_back():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import evaluation as E
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    with pytest.raises(RuntimeError):
        E.fit_quality(TriMesh(v, f), np.zeros((10, 3)), backend='device')
    with pytest.raises(ValueError):
        E.fit_quality(TriMesh(v, f), np.zeros((10, 3)), backend='gpu')
