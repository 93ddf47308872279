"""CPU test: libnanowrap_hip.so exports every function include/nw_clustering.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header and the one under it, its kernels stay
within their budgets without scratch, the calls check their arguments before they touch a GPU, and nothing falls back to the host."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_pc_count', 'k_pc_hook', 'k_pc_compress', 'k_pc_number', 'k_pc_border', 'k_pc_stats', 'k_pc_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_clustering.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwp_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_clustering_header():
    from ch_shrinkwrap_amd import build, _lib, clustering
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ['nwp_abi_version', 'nwp_cluster_stats', 'nwp_create', 'nwp_dbscan', 'nwp_destroy', 'nwp_last_error', 'nwp_set_cloud', 'nwp_set_shortcuts']
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(clustering.SYMBOLS) == names
    assert clustering.load().nwp_abi_version() == clustering.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_clustering.h')).read()
    for name in ('NWP_INFO_WORDS', 'NWP_INFO_N_CORE', 'NWP_INFO_N_BORDER', 'NWP_INFO_N_NOISE', 'NWP_INFO_N_CLUSTERS', 'NWP_INFO_CELLS', 'NWP_INFO_CELL_SIZE',
                 'NWP_INFO_TESTS', 'NWP_INFO_SHORTCUT_A', 'NWP_INFO_SHORTCUT_B', 'NWP_INFO_GUARD', 'NWP_INFO_TESTS_COUNT', 'NWP_INFO_TESTS_HOOK'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(clustering, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOCLOUD'):
        assert int(re.search(r'NWP_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(clustering, 'NWP_ERR_' + name)
        assert getattr(clustering, 'NWP_ERR_' + name) in clustering.ERRORS
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_clustering_core.h')).read()
    assert float(re.search(r'#define NWP_CELL_OF_EPS\s+([0-9.]+)', core).group(1)) == clustering.CELL_OF_EPS == 0.57
    assert '#define NWP_MAX_N (1ll << 30)' in core and clustering.MAX_N == 1 << 30
    assert float(re.search(r'#define NWP_MAX_EPS\s+([0-9.]+)', core).group(1)) == clustering.MAX_EPS == 2.0 ** 40
    # the starting cell has the shortcuts, one widening step (a tenth) has not
    s = np.sqrt(3.0) * (1.0 + 2.0 / 1024.0)
    assert clustering.CELL_OF_EPS * s < 1.0 < 1.1 * clustering.CELL_OF_EPS * s


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_CLUSTERING]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_clustering.hip') and build.OBJ_CLUSTERING.endswith('nw_clustering.o')
    deps = unit[0][2]
    for core in ('nw_clustering_core.h', 'nw_neighbours_core.h'):                                 # rebuilt when either changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_clustering.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_CLUSTERING in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_CLUSTERING)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert sorted(k for k in build.KERNEL_BUDGETS if k.startswith('k_pc_')) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] <= 64 and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)      # eight waves per SIMD


def test_the_unit_is_new_and_the_core_reuses_the_neighbour_core():
    """the squared distance, the ring bound and the cell slack are nw_neighbours_core.h's: included and not copied; the kernels are in an
    object of their own, and no other unit has gained or lost one"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_clustering_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_neighbours_core.h']                   # HIP-free
    assert not re.search(r'NWK_HD\s+[\w ]+\bnwk_\w+\s*\(', core) and '#define NWK_CELL_SLACK' not in core  # no nwk_ definition of its own
    for name in ('nwk_dist2(', 'nwk_ring_lbd(', 'NWK_CELL_SLACK'):
        assert name in core
    assert 'sqrt' not in re.sub(r'//.*', '', core)
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_clustering.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert '"nw_clustering_core.h"' in src and '"nw_bq.h"' in src and '"nw_neighbours.h"' not in src
    assert 'bq::CloudGrid grid;' in code and 'grid.set_cloud(' in code and 'grid.bin(' in code and 'bq::scan_total' in code and 'sqrt' not in code
    assert 'build_grid' not in code and 'bq::bounds' not in code and 'cursor' not in code                # the unit holds the cloud grid ...
    shared = re.sub(r'//.*', '', open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_bq.hip')).read())
    assert 'build_grid<float>(stream, cloud.as<float>()' in shared and 'bounds<float>(stream, mm, cloud.as<float>()' in shared     # ... which bins with the shared grid
    assert shared.count('atomicAdd(&cursor[cell[i]], 1)') == 1 and 'sorted[slot] = point_of(xyz + 3 * (int64_t)i, i)' in shared     # the one scatter, index and all
    assert not re.search(r'atomicAdd\(\s*\(?(float|double)', code)                                        # integer atomics only
    for obj in build.BUDGETED_OBJECTS:
        names = build.kernel_resources(obj)
        if obj == build.OBJ_CLUSTERING:
            assert not [k for k in names if not k.startswith('k_pc_')]
        else:
            assert not [k for k in names if k.startswith('k_pc_')], obj
    for tree in ('include', 'ch_shrinkwrap_amd'):                                                         # the prefix is this unit's alone
        for d, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith(('.h', '.hip', '.cpp', '.py')) and 'clustering' not in fn and fn != 'build.py':
                    assert not re.search(r'\bnwp_\w+\s*\(', open(os.path.join(d, fn), errors='replace').read()), fn


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the cloud and of eps, min_points and count_cap comes before the
    first use of the context."""
    from ch_shrinkwrap_amd import clustering as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    BAD = C.NWP_ERR_BADARG
    xyz = np.ones((5, 3), np.float32)
    assert L.nwp_set_cloud(None, p(xyz), 5, 0) == BAD                                                    # all is well but the context
    assert L.nwp_set_cloud(None, None, 5, 0) == BAD and L.nwp_set_cloud(None, p(xyz), 0, 0) == BAD
    assert L.nwp_set_cloud(None, p(xyz), (1 << 30) + 1, 0) == BAD and L.nwp_set_cloud(None, p(xyz), 5, 2) == BAD
    for bad in (np.nan, np.inf, -np.inf):
        q = xyz.copy()
        q[3, 1] = bad
        assert L.nwp_set_cloud(None, p(q), 5, 0) == C.NWP_ERR_NONFINITE
    outs = [np.full(5, -7, np.int32), np.full(5, -7, np.int32), np.full(5, -7, np.int32), np.full(5, 7, np.uint8)]
    nc, info = np.full(1, -7, np.int32), np.full(C.NWP_INFO_WORDS, -7, np.int64)

    def d(eps=1.0, mp=3, cap=3, nc_=p(nc), info_=p(info)):
        return L.nwp_dbscan(None, eps, mp, cap, *[p(o) for o in outs], nc_, info_)
    assert d() == BAD                                                                                    # all is well but the context
    assert d(nc_=None) == BAD and d(info_=None) == BAD
    for eps in (0.0, -1.0, np.nan, np.inf, -np.inf, 2.0 ** 40 * 1.5):
        assert d(eps=eps) == BAD
    assert d(mp=0, cap=3) == BAD and d(mp=-2, cap=3) == BAD and d(mp=4, cap=3) == BAD
    assert d(mp=(1 << 30) + 1, cap=(1 << 30) + 1) == BAD and d(mp=3, cap=(1 << 30) + 1) == BAD
    assert all((o == o.flat[0]).all() and abs(int(o.flat[0])) == 7 for o in outs + [nc, info])           # nothing was written
    assert L.nwp_cluster_stats(None, None, None, None, None) == BAD and L.nwp_set_shortcuts(None, 1) == BAD
    h = ctypes.c_void_p()
    assert L.nwp_create(-1, ctypes.byref(h)) == BAD and L.nwp_create(0, None) == BAD
    assert L.nwp_last_error(None) == b'null ctx'


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import clustering as C
    pts = np.random.default_rng(0).normal(size=(40, 3)).astype(np.float32)
    with pytest.raises(RuntimeError):
        C.ClusterContext()
    with pytest.raises(RuntimeError):
        C.dbscan(pts, 1.0, 3)
    with pytest.raises(RuntimeError):
        C.split_objects(pts, 1.0, 3)
    with pytest.raises(RuntimeError):
        C.denoise(pts, 1.0, 3)
    with pytest.raises(RuntimeError):
        C.k_distance_curve(pts, 3)
    with pytest.raises(RuntimeError):
        C.DBSCANClustering().execute({'filtered_localizations': {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2]}})
    assert not [n for n in dir(C) if 'sklearn' in n.lower() or 'scipy' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]
    assert 'sklearn' not in open(C.__file__).read().replace('scikit-learn', '')


def test_the_recipe_class_has_the_written_down_defaults():
    import inspect
    from ch_shrinkwrap_amd import clustering as C
    m = C.DBSCANClustering()
    assert (m.input, m.search_radius, m.min_clump_size, m.clump_column, m.output) == (
        'filtered_localizations', 25.0, 10, 'dbscanClumpID', 'clustered_localizations')
    assert C.DBSCANClustering(search_radius=12.0).search_radius == 12.0
    with pytest.raises(AttributeError):
        C.DBSCANClustering(search_radiuss=3.0)
    sig = inspect.signature(C.dbscan)                             # eps and min_points have no defaults
    assert sig.parameters['eps'].default is inspect.Parameter.empty and sig.parameters['min_points'].default is inspect.Parameter.empty
    assert 'not a recommendation' in C.DBSCANClustering.__doc__ and 'Nothing chooses eps automatically' in C.k_distance_curve.__doc__
