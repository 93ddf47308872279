"""CPU test: libnanowrap_hip.so exports every function include/nw_geodesic.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header and the one under it, its kernels stay
within their budgets without scratch at eight waves per SIMD, the calls check their arguments before they touch a GPU and write nothing
when they refuse, and nothing falls back to the host."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_gd_weights', 'k_gd_seed', 'k_gd_relax', 'k_gd_labels', 'k_gd_finish', 'k_gd_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_geodesic.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwt_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_geodesic_header():
    from ch_shrinkwrap_amd import build, _lib, geodesic
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ['nwt_abi_version', 'nwt_create', 'nwt_destroy', 'nwt_distances', 'nwt_last_error', 'nwt_set_mesh']
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(geodesic.SYMBOLS) == names
    assert geodesic.load().nwt_abi_version() == geodesic.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_geodesic.h')).read()
    for name in ('NWT_INFO_WORDS', 'NWT_INFO_HALFEDGES', 'NWT_INFO_DIAGONALS', 'NWT_INFO_REACHED', 'NWT_INFO_IN_BAND', 'NWT_INFO_ROUNDS',
                 'NWT_INFO_LABEL_ROUNDS', 'NWT_INFO_LAUNCHES', 'NWT_INFO_LOWERED', 'NWT_INFO_RELAXED', 'NWT_INFO_BATCH', 'NWT_FLAG_DIAGONALS'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(geodesic, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH', 'INTERNAL'):
        assert int(re.search(r'NWT_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(geodesic, 'NWT_ERR_' + name)
        assert getattr(geodesic, 'NWT_ERR_' + name) in geodesic.ERRORS
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_geodesic_core.h')).read()
    assert int(re.search(r'#define NWT_BATCH\s+(\d+)', core).group(1)) == geodesic.BATCH == 16
    assert int(re.search(r'#define NWT_SWEEPS\s+(\d+)', core).group(1)) == geodesic.SWEEPS
    assert 'nobody has measured' in core                          # the batch and the sweeps are first choices, and say so
    assert '#define NWT_MAX_N (1ll << 30)' in core and geodesic.MAX_N == 1 << 30
    assert '#define NWT_MAX_FACES (1ll << 29)' in core and geodesic.MAX_FACES == 1 << 29
    # the scheduling-dependent info words are named as such, in the header and in the binding
    assert 'NOT DETERMINISTIC' in txt and set(geodesic.NOT_DETERMINISTIC) == {'rounds', 'label_rounds', 'launches', 'lowered', 'relaxed'}


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_GEODESIC]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_geodesic.hip') and build.OBJ_GEODESIC.endswith('nw_geodesic.o')
    deps = unit[0][2]
    for core in ('nw_geodesic_core.h', 'nw_neighbours_core.h'):                                  # rebuilt when either changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_geodesic.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_GEODESIC in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_GEODESIC)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert sorted(k for k in build.KERNEL_BUDGETS if k.startswith('k_gd_')) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] <= 64 and r['lds'] <= build.KERNEL_BUDGETS[k][1] <= 2048, (k, r)      # eight waves per SIMD


def test_the_unit_is_new_and_the_core_reuses_the_neighbour_core():
    """the squared distance is nw_neighbours_core.h's: included and not copied; the kernels are in an object of their own, no other unit
    has gained or lost one, and the prefix is this unit's alone"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_geodesic_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_neighbours_core.h']                   # HIP-free
    assert not re.search(r'NWK_HD\s+[\w ]+\bnwk_\w+\s*\(', core)                                          # no nwk_ definition of its own
    assert len(re.findall(r'NWK_HD\s+[\w ]+\bnwt_\w+\s*\(', core)) >= 10
    for name in ('nwk_dist2(', 'Proof', 'UPPER BOUND', 'no MMP', 'least fixed point'):
        assert name in core
    assert 'fma(' not in core and 'hip' not in re.sub(r'//.*', '', core).lower()
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_geodesic.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert '"nw_geodesic_core.h"' in src and '"nw_bq.h"' in src
    for name in ('nwt_halfedge_setup(', 'nwt_lane_arc(', 'nwt_relax(', 'nwt_tight(', 'nwt_start_value(', 'atomicMin('):
        assert name in code
    # no workgroup waits on another: no cooperative launch, no grid barrier, no loop on a flag
    for name in ('cooperative', 'grid_group', 'this_grid', 'while (', 'while(', 'atomicCAS', 'sleep'):
        assert name not in code, name
    for obj in build.BUDGETED_OBJECTS:
        names = build.kernel_resources(obj)
        if obj == build.OBJ_GEODESIC:
            assert not [k for k in names if not k.startswith('k_gd_')]
        else:
            assert not [k for k in names if k.startswith('k_gd_')], obj
    for tree in ('include', 'ch_shrinkwrap_amd'):
        for d, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith(('.h', '.hip', '.cpp', '.py')) and 'geodesic' not in fn:
                    assert not re.search(r'\bnwt_\w+', open(os.path.join(d, fn), errors='replace').read()), fn


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the mesh, the sources and the cap comes before the first use of
    the context, and a refused call writes nothing."""
    from ch_shrinkwrap_amd import geodesic as C
    L = C.load()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    BAD = C.NWT_ERR_BADARG
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    twin = np.array([-1, 3, -1, 1, -1, -1], np.int32)

    def m(P=pos, nv=4, F=faces, nf=2, T=twin, dev=0):
        return L.nwt_set_mesh(None, p(P), nv, p(F), nf, p(T), dev)
    assert m() == BAD and m(T=None) == BAD                                                              # all is well but the context
    assert m(P=None) == BAD and m(F=None) == BAD and m(nv=0) == BAD and m(nf=0) == BAD and m(dev=2) == BAD
    assert m(nv=(1 << 30) + 1) == BAD and m(nf=(1 << 30) + 1) == BAD
    for bad in (np.nan, np.inf, -np.inf):
        q = pos.copy()
        q[3, 1] = bad
        assert m(P=q) == C.NWT_ERR_NONFINITE
    for bad in (4, -1):
        f = faces.copy()
        f[1, 2] = bad
        assert m(F=f) == BAD
    for h, t in ((1, 4), (1, 6), (1, -2), (0, 0)):                                                      # a twin table that is not mutual
        tw = twin.copy()
        tw[h] = t
        assert m(T=tw) == BAD

    dist, src, info = np.full(4, 7.0), np.full(4, 7, np.int32), np.full(C.NWT_INFO_WORDS, -7, np.int64)
    ids, d0 = np.array([0, 3], np.int32), np.array([0.0, 1.0])

    def d(i=ids, s=d0, n=2, cap=np.inf, flags=C.NWT_FLAG_DIAGONALS, out=dist, lab=src, inf=info):
        return L.nwt_distances(None, p(i), p(s), n, float(cap), flags, p(out), p(lab), p(inf))
    assert d() == BAD and d(s=None) == BAD and d(flags=0, lab=None) == BAD                              # all is well but the context
    assert d(i=None) == BAD and d(n=0) == BAD and d(n=(1 << 30) + 1) == BAD and d(out=None) == BAD and d(inf=None) == BAD and d(flags=2) == BAD
    assert d(i=np.array([0, -1], np.int32)) == BAD
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        assert d(s=np.array([0.0, bad])) == BAD
    for bad in (0.0, -1.0, np.nan, -np.inf):
        assert d(cap=bad) == BAD
    assert (dist == 7).all() and (src == 7).all() and (info == -7).all()                                # nothing was written
    h = ctypes.c_void_p()
    assert L.nwt_create(-1, ctypes.byref(h)) == BAD and L.nwt_create(0, None) == BAD
    assert L.nwt_last_error(None) == b'null ctx'


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import geodesic as C
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    with pytest.raises(RuntimeError):
        C.GeodesicContext()
    with pytest.raises(RuntimeError):
        C.geodesic_distance((v, f), [0])
    with pytest.raises(RuntimeError):
        C.geodesic_distance((v, f), [0, 3], d0=[0.0, 1.0], max_distance=5.0, diagonals=False, labels=True)
    with pytest.raises(RuntimeError):
        TriMesh(v, f).geodesic_distance([0])
    with pytest.raises(RuntimeError):
        C.GeodesicDistance(input_sources='marks').execute({'membrane': TriMesh(v, f), 'marks': {'source': np.arange(v.shape[0]) < 3}})
    assert not [n for n in dir(C) if 'scipy' in n.lower() or 'heapq' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]
    src = open(C.__file__).read()
    assert 'scipy' not in src and 'heapq' not in src and 'dijkstra' not in src.lower()


def test_signatures_docstrings_and_what_runs_on_the_host():
    from ch_shrinkwrap_amd import geodesic as C
    from ch_shrinkwrap_amd.trimesh import TriMesh
    assert list(inspect.signature(C.geodesic_distance).parameters)[:7] == ['mesh', 'sources', 'd0', 'max_distance', 'diagonals', 'labels', 'context']
    sig = inspect.signature(C.geodesic_distance).parameters
    assert sig['d0'].default is None and sig['max_distance'].default == np.inf and sig['diagonals'].default is True and sig['labels'].default is False
    assert list(inspect.signature(C.GeodesicContext.set_mesh).parameters) == ['self', 'vertices', 'faces', 'twin']
    assert list(inspect.signature(C.GeodesicContext.distances).parameters) == ['self', 'sources', 'd0', 'max_distance', 'labels']
    assert list(inspect.signature(C.surface_profile).parameters) == ['distance', 'values', 'area', 'edges']
    assert list(inspect.signature(C.sources_from_faces).parameters) == ['faces', 'face_mask_or_labels']
    assert list(inspect.signature(TriMesh.geodesic_distance).parameters)[:2] == ['self', 'sources']
    for doc in (C.__doc__, C.geodesic_distance.__doc__, C.GeodesicContext.distances.__doc__):
        flat = re.sub(r'\s+', ' ', doc)
        assert 'graph distance with one level of unfolding' in flat.lower() and 'not an exact polyhedral geodesic' in flat.lower()
    assert 'no exactness claim' in C.surface_profile.__doc__
    assert 'NOT DETERMINISTIC' in C.GeodesicContext.distances.__doc__
    m = C.GeodesicDistance()
    assert (m.input_mesh, m.output, m.max_distance, m.diagonals) == ('membrane', 'geodesic_distances', np.inf, True) and hasattr(m, 'input_sources')
    assert C.GeodesicDistance(max_distance=200.0).max_distance == 200.0
    with pytest.raises(AttributeError):
        C.GeodesicDistance(max_distanse=3.0)
    # sources_from_faces and surface_profile are host code
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4]], np.int32)
    ids, patch = C.sources_from_faces(faces, np.array([True, False, True]))
    assert ids.tolist() == [0, 1, 2, 3, 4] and patch.tolist() == [0] * 5 and ids.dtype == np.int32
    ids, patch = C.sources_from_faces(faces, np.array([1, -1, 0]))
    assert ids.tolist() == [0, 1, 2, 3, 4] and patch.tolist() == [1, 0, 1, 0, 0]
    ids, patch = C.sources_from_faces(faces, np.array([-1, -1, -1]))
    assert ids.size == 0
    with pytest.raises(ValueError):
        C.sources_from_faces(faces, np.array([True, False]))
    r_mid, mean, area, n = C.surface_profile([0.0, 0.5, 1.5, 2.0, np.inf, 3.0], [1.0, 3.0, 5.0, 7.0, 9.0, 11.0], [1.0, 3.0, 1.0, 1.0, 1.0, 1.0], [0.0, 1.0, 2.0])
    assert r_mid.tolist() == [0.5, 1.5] and mean.tolist() == [2.5, 6.0] and area.tolist() == [4.0, 2.0] and n.tolist() == [2, 2]
    assert np.isnan(C.surface_profile([5.0], [1.0], [1.0], [0.0, 1.0])[1]).all()
    with pytest.raises(ValueError):
        C.surface_profile([0.0], [1.0], [1.0], [1.0, 1.0])
