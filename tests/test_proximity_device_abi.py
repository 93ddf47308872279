"""CPU test: libnanowrap_hip.so exports every function include/nw_proximity.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header and the two it includes, its kernels
stay within their budgets without scratch, the calls check their arguments before they touch a GPU, and nothing falls back to the host."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_mm_query', 'k_mm_finish', 'k_mm_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_proximity.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwm_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_proximity_header():
    from ch_shrinkwrap_amd import build, _lib, proximity
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ['nwm_abi_version', 'nwm_create', 'nwm_destroy', 'nwm_last_error', 'nwm_query', 'nwm_set_mesh']
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(proximity.SYMBOLS) == names
    assert proximity.load().nwm_abi_version() == proximity.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_proximity.h')).read()
    for name in ('NWM_KIND_PIERCED', 'NWM_KIND_EDGE_EDGE', 'NWM_INFO_WORDS', 'NWM_INFO_IN_BAND', 'NWM_INFO_AT_ZERO', 'NWM_INFO_RINGS', 'NWM_INFO_CENTROIDS',
                 'NWM_INFO_TESTS', 'NWM_INFO_CELLS', 'NWM_INFO_CELL_SIZE'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(proximity, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH'):
        assert int(re.search(r'NWM_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(proximity, 'NWM_ERR_' + name)
        assert getattr(proximity, 'NWM_ERR_' + name) in proximity.ERRORS


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_PROXIMITY]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_proximity.hip') and build.OBJ_PROXIMITY.endswith('nw_proximity.o')
    deps = unit[0][2]
    for core in ('nw_proximity_core.h', 'nw_distance_core.h', 'nw_intersections_core.h'):       # rebuilt when any of the three changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_proximity.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_PROXIMITY in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_PROXIMITY)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert not [k for k in build.KERNEL_BUDGETS if k.startswith('k_mm_') and k not in KERNELS]
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)
        assert build.KERNEL_BUDGETS[k][0] <= build.KERNEL_BUDGETS['k_mx_count'][0] == 168      # three waves per SIMD at the least


def test_the_unit_is_new_and_the_core_reuses_the_two_cores():
    """the point-triangle distance is nw_distance_core.h's, the segment-face test nw_intersections_core.h's, the centroid the shared
    face grid's (nw_bq_core.h, which nwd_face_centroid forwards to): included and not copied; the kernels are in an object of their own, and no other unit has gained or lost one"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_proximity_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_distance_core.h', 'nw_intersections_core.h']      # HIP-free
    assert not re.search(r'NW[DX]_HD\s+[\w ]+\bnw[dx]_\w+\s*\(', core)                                   # no nwd_ / nwx_ definition of its own
    assert len(re.findall(r'NWD_HD\s+[\w ]+\bnwm_\w+\s*\(', core)) >= 8
    for name in ('nwd_point_triangle', 'nwx_seg_tri', 'nwx_normal'):
        assert name + '(' in core
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_proximity.hip')).read()
    # the centroid and radius of A's and of B's faces come from the shared face grid's one kernel (nw_bq.hip), for both meshes the same
    code = re.sub(r'//.*', '', src)
    assert 'bq::face_setup(' in code and 'set_faces(' in code and '__global__' in code and 'face_setup(const' not in code
    bq_src = re.sub(r'//.*', '', open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_bq.hip')).read())
    assert 'bq::face_centroid(' in bq_src
    dist_core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_distance_core.h')).read()
    assert re.search(r'nwd_face_centroid\([^)]*\)\s*\{\s*return bq::face_centroid\(', dist_core)
    assert '"nw_proximity_core.h"' in src and '"nw_bq.h"' in src and 'atomic' not in re.sub(r'//.*', '', src)
    for obj in (build.OBJ_DISTANCE, build.OBJ_INTERSECTIONS, build.OBJ_RAYS, build.OBJ_VOLUME, build.OBJ_BQ):
        assert not [k for k in build.kernel_resources(obj) if k.startswith('k_mm_')]
    assert not [k for k in build.kernel_resources(build.OBJ_PROXIMITY) if not k.startswith('k_mm_')]
    assert 'what the eleven above share' in open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'build.py')).read()


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the two meshes, the cell size and the band comes before the
    first use of the context."""
    from ch_shrinkwrap_amd import proximity as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros((4, 3), np.float32)
    pos[1, 0] = pos[2, 1] = pos[3, 2] = 10.0
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    BAD = C.NWM_ERR_BADARG
    assert L.nwm_set_mesh(None, p(pos), 4, p(faces), 4, 0.0) == BAD                                      # all is well but the context
    assert L.nwm_set_mesh(None, None, 4, p(faces), 4, 0.0) == BAD
    assert L.nwm_set_mesh(None, p(pos), 4, None, 4, 0.0) == BAD
    assert L.nwm_set_mesh(None, p(pos), 4, p(faces), 0, 0.0) == BAD
    assert L.nwm_set_mesh(None, p(pos), 2, p(faces), 4, 0.0) == BAD
    assert L.nwm_set_mesh(None, p(pos), 4, p(np.array([[0, 1, 4], [0, 1, 2]], np.int32)), 2, 0.0) == BAD
    assert L.nwm_set_mesh(None, p(pos), 4, p(np.array([[0, 1, -1], [0, 1, 2]], np.int32)), 2, 0.0) == BAD
    for cell in (-1.0, np.nan, np.inf):
        assert L.nwm_set_mesh(None, p(pos), 4, p(faces), 4, cell) == BAD
    nan = pos.copy()
    nan[2, 1] = np.inf
    assert L.nwm_set_mesh(None, p(nan), 4, p(faces), 4, 0.0) == C.NWM_ERR_NONFINITE
    dist, partner, kind = np.full(4, -7.0), np.full(4, -7, np.int32), np.full(4, -7, np.int32)
    ca, cb, info = np.full((4, 3), -7.0), np.full((4, 3), -7.0), np.full(C.NWM_INFO_WORDS, -7, np.int64)
    q = lambda pos_, nv, faces_, nf, band: L.nwm_query(None, pos_, nv, faces_, nf, band, p(dist), p(partner), p(kind), p(ca), p(cb), p(info))
    assert q(p(pos), 4, p(faces), 4, 30.0) == BAD and q(p(pos), 4, p(faces), 4, np.inf) == BAD           # all is well but the context
    assert q(None, 4, p(faces), 4, 30.0) == BAD and q(p(pos), 4, None, 4, 30.0) == BAD
    assert q(p(pos), 4, p(faces), 0, 30.0) == BAD and q(p(pos), 2, p(faces), 4, 30.0) == BAD
    assert q(p(pos), 4, p(np.array([[0, 1, 4], [0, 1, 2]], np.int32)), 2, 30.0) == BAD
    for band in (0.0, -3.0, np.nan, -np.inf):
        assert q(p(pos), 4, p(faces), 4, band) == BAD
    assert q(p(nan), 4, p(faces), 4, 30.0) == C.NWM_ERR_NONFINITE
    assert (dist == -7.0).all() and (partner == -7).all() and (kind == -7).all() and (ca == -7.0).all() and (cb == -7.0).all() and (info == -7).all()
    h = ctypes.c_void_p()
    assert L.nwm_create(-1, ctypes.byref(h)) == BAD and L.nwm_create(0, None) == BAD
    assert L.nwm_last_error(None) == b'null ctx'


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import proximity as C
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    w = (v + np.float32(25.0)).astype(np.float32)
    with pytest.raises(RuntimeError):
        C.ProximityContext()
    with pytest.raises(RuntimeError):
        C.mesh_distance((v, f), (w, f))
    with pytest.raises(RuntimeError):
        C.mesh_distance(TriMesh(v, f), TriMesh(w, f), band=30.0, return_closest=True)
    with pytest.raises(RuntimeError):
        C.contact_sites((v, f), (w, f), 30.0)
    with pytest.raises(RuntimeError):
        TriMesh(v, f).distance_to_mesh_of(TriMesh(w, f), band=30.0)
    with pytest.raises(RuntimeError):
        C.MembraneContacts().execute({'membrane': TriMesh(v, f), 'membrane2': TriMesh(w, f)})
    assert not [n for n in dir(C) if 'scipy' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]


def test_the_recipe_class_has_the_written_down_defaults():
    from ch_shrinkwrap_amd import proximity as C
    m = C.MembraneContacts()
    assert (m.input_a, m.input_b, m.contact_distance, m.output) == ('membrane', 'membrane2', 30.0, 'contacts')
    assert C.MembraneContacts(contact_distance=12.0).contact_distance == 12.0
    with pytest.raises(AttributeError):
        C.MembraneContacts(contact_distanse=3.0)
