"""CPU test: libnanowrap_hip.so exports every function include/nw_structure.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header and the one under it, its kernels stay
within their budgets without scratch, the calls check their arguments before they touch a GPU, and nothing falls back to the host."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_st_moments', 'k_st_eigen', 'k_st_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_structure.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwf_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_structure_header():
    from ch_shrinkwrap_amd import build, _lib, structure
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ['nwf_abi_version', 'nwf_create', 'nwf_destroy', 'nwf_last_error', 'nwf_query', 'nwf_set_cloud']
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(structure.SYMBOLS) == names
    assert structure.load().nwf_abi_version() == structure.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_structure.h')).read()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_structure_core.h')).read()
    for name in ('NWF_INFO_WORDS', 'NWF_INFO_TESTS', 'NWF_INFO_CELLS_READ', 'NWF_INFO_CELL_SIZE', 'NWF_INFO_CELLS', 'NWF_INFO_NEIGHBOURS', 'NWF_INFO_FEW',
                 'NWF_INFO_N_QUERIES', 'NWF_INFO_N_CLOUD', 'NWF_MOMENT_WORDS'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(structure, name)
    for name in ('VALID', 'EMPTY', 'FEW', 'POINT', 'TURNED'):                                          # the flags: in both headers and in the binding
        for t in (txt, core):
            assert int(re.search(r'#define NWF_FLAG_%s\s+(\d+)' % name, t).group(1)) == getattr(structure, 'NWF_FLAG_' + name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOCLOUD'):
        assert int(re.search(r'NWF_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(structure, 'NWF_ERR_' + name)
        assert getattr(structure, 'NWF_ERR_' + name) in structure.ERRORS
    assert float(re.search(r'#define NWF_CELL_OF_R\s+([0-9.]+)', core).group(1)) == structure.CELL_OF_R == 0.5
    assert 'nobody has measured' in core                                                                 # the 0.5 is a first choice, and says so
    assert '#define NWF_MAX_N (1ll << 26)' in core and structure.MAX_N == 1 << 26
    assert float(re.search(r'#define NWF_MAX_R\s+([0-9.]+)', core).group(1)) == structure.MAX_R == 2.0 ** 40
    assert float(re.search(r'#define NWF_Q_ONE\s+([0-9.]+)', core).group(1)) == structure.Q_ONE == 2.0 ** 18
    assert int(re.search(r'#define NWF_Q_BITS\s+(\d+)', core).group(1)) == 18
    assert int(re.search(r'#define NWF_SWEEPS\s+(\d+)', core).group(1)) == structure.SWEEPS
    assert int(re.search(r'#define NWF_MOMENTS\s+(\d+)', core).group(1)) == structure.NWF_MOMENT_WORDS == 10
    assert structure.quantum(2.0) == 2.0 ** -17 and structure.quantum(3.0) == 2.0 ** -16 and structure.quantum(30.0) == 2.0 ** -13


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_STRUCTURE]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_structure.hip') and build.OBJ_STRUCTURE.endswith('nw_structure.o')
    deps = unit[0][2]
    for core in ('nw_structure_core.h', 'nw_neighbours_core.h'):                                   # rebuilt when either changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_structure.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_STRUCTURE in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_STRUCTURE)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert sorted(k for k in build.KERNEL_BUDGETS if k.startswith('k_st_')) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] <= 64 and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)      # eight waves per SIMD
        assert build.KERNEL_BUDGETS[k][0] % 8 == 0 and build.KERNEL_BUDGETS[k][0] - r['vgpr'] < 8, (k, r)            # the budget is the next multiple of 8
    assert res['k_st_moments']['lds'] == 2 * 4 * 8                                                       # the two waves' four counters: no column
    assert res['k_st_eigen']['lds'] == 0


def test_the_unit_is_new_and_the_core_reuses_the_neighbour_core():
    """the squared distance and the cell slack are nw_neighbours_core.h's: included and not copied; the kernels are in an object of their
    own, and no other unit has gained or lost one"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_structure_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_neighbours_core.h']                   # HIP-free
    assert not re.search(r'NWK_HD\s+[\w ]+\bnwk_\w+\s*\(', core) and '#define NWK_CELL_SLACK' not in core  # no nwk_ definition of its own
    assert len(re.findall(r'NWK_HD\s+[\w ]+\bnwf_\w+\s*\(', core)) >= 10
    for name in ('nwk_dist2(', 'NWK_CELL_SLACK', 'Proof.', 'Proof that', 'rint(', '2^62', '2^44', '(long long)ux * uy'):
        assert name in core
    assert 'fma(' not in core
    assert not re.search(r'\[\s*[a-z]\w*\s*\]', re.sub(r'//.*', '', core).replace('pts[p]', ''))          # nothing but the cloud is indexed at run time
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_structure.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert '"nw_structure_core.h"' in src and '"nw_bq.h"' in src and '"nw_neighbours.h"' not in src and '"nw_pairs_core.h"' not in src
    assert 'bq::CloudGrid grid;' in code and 'grid.set_cloud(' in code and 'grid.bin(' in code and 'nwf_walk(' in code and 'nwf_visit(' in code and 'nwf_shape(' in code
    assert 'build_grid' not in code and 'bq::bounds' not in code and 'cursor' not in code                # the unit holds the cloud grid ...
    shared = re.sub(r'//.*', '', open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_bq.hip')).read())
    assert 'build_grid<float>(stream, cloud.as<float>()' in shared and 'bounds<float>(stream, mm, cloud.as<float>()' in shared     # ... which bins with the shared grid
    assert shared.count('atomicAdd(&cursor[cell[i]], 1)') == 1 and 'sorted[slot] = point_of(xyz + 3 * (int64_t)i, i)' in shared     # the one scatter, index and all
    assert 'atomicAdd' not in code and 'atomicCAS' not in code                                           # the unit has no scatter of its own, and the results need no atomics
    for obj in build.BUDGETED_OBJECTS:
        names = build.kernel_resources(obj)
        if obj == build.OBJ_STRUCTURE:
            assert not [k for k in names if not k.startswith('k_st_')]
        else:
            assert not [k for k in names if k.startswith('k_st_')], obj
    for tree in ('include', 'ch_shrinkwrap_amd'):                                                         # the prefix is this unit's alone
        for d, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith(('.h', '.hip', '.cpp', '.py')) and 'structure' not in fn and fn != 'build.py':
                    assert not re.search(r'\bnwf_\w+\s*\(', open(os.path.join(d, fn), errors='replace').read()), fn


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the cloud, the queries, the radius and the viewpoint comes
    before the first use of the context."""
    from ch_shrinkwrap_amd import structure as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    BAD = C.NWF_ERR_BADARG
    xyz = np.ones((5, 3), np.float32)
    assert L.nwf_set_cloud(None, p(xyz), 5, 0) == BAD                                                    # all is well but the context
    assert L.nwf_set_cloud(None, None, 5, 0) == BAD and L.nwf_set_cloud(None, p(xyz), 0, 0) == BAD
    assert L.nwf_set_cloud(None, p(xyz), (1 << 26) + 1, 0) == BAD and L.nwf_set_cloud(None, p(xyz), 5, 2) == BAD
    for bad in (np.nan, np.inf, -np.inf):
        q = xyz.copy()
        q[3, 1] = bad
        assert L.nwf_set_cloud(None, p(q), 5, 0) == C.NWF_ERR_NONFINITE

    mom, lam, vec = np.full((5, 10), 7, np.int64), np.full((5, 3), 7.0), np.full((5, 9), 7.0)
    flags, info, view = np.full(5, 7, np.uint8), np.full(C.NWF_INFO_WORDS, -7, np.int64), np.array([0.0, 1.0, 2.0])

    def c(q=p(xyz), nq=5, dev=0, r=1.0, v=p(view), i=p(info)):
        return L.nwf_query(None, q, nq, dev, r, v, p(mom), p(lam), p(vec), p(flags), i)
    assert c() == BAD and c(q=None, nq=0) == BAD and c(v=None) == BAD                                    # all is well but the context
    assert c(i=None) == BAD and c(dev=2) == BAD and c(dev=-1) == BAD
    assert c(nq=0) == BAD and c(nq=(1 << 26) + 1) == BAD and c(q=None, nq=-1) == BAD
    for r in (0.0, -1.0, np.nan, np.inf, -np.inf, 2.0 ** 40 * 1.0000001, 1e-170, 1e200):
        assert c(r=float(r)) == BAD, r
    q = xyz.copy()
    q[2, 2] = np.nan
    assert c(q=p(q)) == C.NWF_ERR_NONFINITE
    for bad in (np.nan, np.inf, -np.inf):
        v = view.copy()
        v[1] = bad
        assert c(v=p(v)) == C.NWF_ERR_NONFINITE
    assert (mom == 7).all() and (lam == 7).all() and (vec == 7).all() and (flags == 7).all() and (info == -7).all()   # nothing was written
    h = ctypes.c_void_p()
    assert L.nwf_create(-1, ctypes.byref(h)) == BAD and L.nwf_create(0, None) == BAD
    assert L.nwf_last_error(None) == b'null ctx'


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import structure as C
    pts = np.random.default_rng(0).normal(size=(40, 3)).astype(np.float32)
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2]}
    with pytest.raises(RuntimeError):
        C.StructureContext()
    with pytest.raises(RuntimeError):
        C.local_moments(pts, 1.0)
    with pytest.raises(RuntimeError):
        C.local_moments(pts[:5], 1.0, other=pts)
    with pytest.raises(RuntimeError):
        C.local_shape(pts, 1.0)
    with pytest.raises(RuntimeError):
        C.local_shape(pts, 1.0, viewpoint=(0.0, 0.0, 5.0))
    with pytest.raises(RuntimeError):
        C.cloud_normals(pts, 1.0)
    with pytest.raises(RuntimeError):
        C.radius_from_k(pts, k=5)
    with pytest.raises(RuntimeError):
        C.LocalShape(radius=1.0).execute({'filtered_localizations': table})
    with pytest.raises(RuntimeError):
        C.LocalShape(k=5).execute({'filtered_localizations': table})
    assert not [n for n in dir(C) if 'sklearn' in n.lower() or 'scipy' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]
    src = open(C.__file__).read()
    assert 'scipy' not in src and 'cKDTree' not in src and 'sklearn' not in src and 'linalg' not in src


def test_the_python_surface_says_what_it_is():
    import inspect
    from ch_shrinkwrap_amd import structure as C
    assert list(inspect.signature(C.local_moments).parameters)[:4] == ['points', 'radius', 'other', 'context']
    assert list(inspect.signature(C.local_shape).parameters)[:5] == ['points', 'radius', 'other', 'viewpoint', 'context']
    assert list(inspect.signature(C.cloud_normals).parameters)[:3] == ['points', 'radius', 'viewpoint']
    sig = inspect.signature(C.radius_from_k).parameters
    assert list(sig)[:3] == ['points', 'k', 'factor'] and sig['k'].default == 20 and sig['factor'].default == 1.5
    assert 'no exactness claim' in C.radius_from_k.__doc__ and 'no exactness claim' in C.shape_features.__doc__
    m = C.LocalShape()
    assert (m.input, m.output, m.radius, m.k, m.viewpoint) == ('filtered_localizations', 'shape_localizations', None, 20, None)
    assert C.LocalShape(radius=12.0, viewpoint=(0, 0, 1)).radius == 12.0
    with pytest.raises(AttributeError):
        C.LocalShape(radiuss=3.0)
    with pytest.raises(ValueError):
        C.radius_from_k(np.zeros((5, 3), np.float32), k=20)                     # fewer points than neighbours: before anything touches a GPU
    with pytest.raises(ValueError):
        C.radius_from_k(np.zeros((50, 3), np.float32), k=40)
    # the features from given numbers: host arithmetic on the device's output, NaN where not valid
    M = np.array([[4, 0, 0, 0, 8, 0, 0, 4, 0, 0], [2, 4, 0, 0, 8, 0, 0, 0, 0, 0], [0] * 10], np.int64)
    lam = np.array([[4.0, 1.0, -1e-17], [1.0, 0.0, 0.0], [np.nan] * 3])
    F = C.shape_features(M, lam, np.array([1, 4, 2], np.uint8), 2.0)
    assert F['valid'].tolist() == [True, False, False]
    assert (F['linearity'][0], F['planarity'][0], F['scattering'][0], F['surface_variation'][0], F['centroid_offset'][0]) == (0.75, 0.25, 0.0, 0.0, 0.0)
    assert all(np.isnan(F[k][1:]).all() for k in ('linearity', 'planarity', 'scattering', 'surface_variation', 'centroid_offset'))
