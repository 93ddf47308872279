"""CPU test: libnanowrap_hip.so exports every function include/nw_pairs.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header and the one under it, its kernels stay
within their budgets without scratch, the calls check their arguments before they touch a GPU, and nothing falls back to the host."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_pq_pairs<false>', 'k_pq_pairs<true>', 'k_pq_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_pairs.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwq_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_pairs_header():
    from ch_shrinkwrap_amd import build, _lib, pairs
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ['nwq_abi_version', 'nwq_count', 'nwq_create', 'nwq_destroy', 'nwq_last_error', 'nwq_set_cloud', 'nwq_set_edges']
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(pairs.SYMBOLS) == names
    assert pairs.load().nwq_abi_version() == pairs.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_pairs.h')).read()
    for name in ('NWQ_INFO_WORDS', 'NWQ_INFO_TESTS', 'NWQ_INFO_CELLS_READ', 'NWQ_INFO_CELL_SIZE', 'NWQ_INFO_CELLS', 'NWQ_INFO_VARIANT', 'NWQ_INFO_N_QUERIES',
                 'NWQ_INFO_N_CLOUD', 'NWQ_INFO_BINS'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(pairs, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOCLOUD'):
        assert int(re.search(r'NWQ_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(pairs, 'NWQ_ERR_' + name)
        assert getattr(pairs, 'NWQ_ERR_' + name) in pairs.ERRORS
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_pairs_core.h')).read()
    assert float(re.search(r'#define NWQ_CELL_OF_RMAX\s+([0-9.]+)', core).group(1)) == pairs.CELL_OF_RMAX == 0.5
    assert 'nobody has measured' in core                                                                 # the 0.5 is a first choice, and says so
    assert '#define NWQ_MAX_N (1ll << 30)' in core and pairs.MAX_N == 1 << 30
    assert float(re.search(r'#define NWQ_MAX_R\s+([0-9.]+)', core).group(1)) == pairs.MAX_R == 2.0 ** 40
    for t in (core, txt):
        assert int(re.search(r'#define NWQ_MAX_BINS\s+(\d+)', t).group(1)) == pairs.MAX_BINS == 64
    assert int(re.search(r'#define NWQ_NARROW_BINS\s+(\d+)', core).group(1)) == pairs.NARROW_BINS == 16


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_PAIRS]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_pairs.hip') and build.OBJ_PAIRS.endswith('nw_pairs.o')
    deps = unit[0][2]
    for core in ('nw_pairs_core.h', 'nw_neighbours_core.h'):                                      # rebuilt when either changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_pairs.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_PAIRS in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_PAIRS)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert sorted(k for k in build.KERNEL_BUDGETS if k.startswith('k_pq_')) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] <= 64 and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)      # eight waves per SIMD
    assert build.KERNEL_BUDGETS['k_pq_pairs<false>'][1] <= 8 * 1024 and build.KERNEL_BUDGETS['k_pq_pairs<true>'][1] <= 32 * 1024
    assert res['k_pq_pairs<false>']['lds'] == 16 * 128 * 4                                               # the columns and nothing else
    assert res['k_pq_pairs<true>']['lds'] == 64 * 64 * 4 + 64 * 8                                        # the columns and the copy of the edges


def test_the_unit_is_new_and_the_core_reuses_the_neighbour_core():
    """the squared distance and the cell slack are nw_neighbours_core.h's: included and not copied; the kernels are in an object of their
    own, and no other unit has gained or lost one"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_pairs_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_neighbours_core.h']                   # HIP-free
    assert not re.search(r'NWK_HD\s+[\w ]+\bnwk_\w+\s*\(', core) and '#define NWK_CELL_SLACK' not in core  # no nwk_ definition of its own
    assert len(re.findall(r'NWK_HD\s+[\w ]+\bnwq_\w+\s*\(', core)) >= 6
    for name in ('nwk_dist2(', 'NWK_CELL_SLACK', 'Proof.'):
        assert name in core
    assert 'sqrt' not in core and 'fma(' not in core
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_pairs.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert '"nw_pairs_core.h"' in src and '"nw_bq.h"' in src and '"nw_neighbours.h"' not in src and '"nw_clustering_core.h"' not in src
    assert 'bq::CloudGrid grid;' in code and 'grid.set_cloud(' in code and 'grid.bin(' in code and 'nwq_walk(' in code and 'nwq_dist2(' in code and 'sqrt' not in code
    assert 'build_grid' not in code and 'bq::bounds' not in code and 'cursor' not in code                # the unit holds the cloud grid ...
    shared = re.sub(r'//.*', '', open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_bq.hip')).read())
    assert 'build_grid<float>(stream, cloud.as<float>()' in shared and 'bounds<float>(stream, mm, cloud.as<float>()' in shared     # ... which bins with the shared grid
    assert shared.count('atomicAdd(&cursor[cell[i]], 1)') == 1 and 'sorted[slot] = point_of(xyz + 3 * (int64_t)i, i)' in shared     # the one scatter, index and all
    assert 'atomicAdd' not in code and 'atomicCAS' not in code                                           # the unit has no scatter of its own, and the counts need no atomics
    for obj in build.BUDGETED_OBJECTS:
        names = build.kernel_resources(obj)
        if obj == build.OBJ_PAIRS:
            assert not [k for k in names if not k.startswith('k_pq_')]
        else:
            assert not [k for k in names if k.startswith('k_pq_')], obj
    for tree in ('include', 'ch_shrinkwrap_amd'):                                                         # the prefix is this unit's alone
        for d, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith(('.h', '.hip', '.cpp', '.py')) and 'pairs' not in fn and fn != 'build.py':
                    assert not re.search(r'\bnwq_\w+\s*\(', open(os.path.join(d, fn), errors='replace').read()), fn


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the cloud, the radii and the queries comes before the first use
    of the context."""
    from ch_shrinkwrap_amd import pairs as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    BAD = C.NWQ_ERR_BADARG
    xyz = np.ones((5, 3), np.float32)
    assert L.nwq_set_cloud(None, p(xyz), 5, 0) == BAD                                                    # all is well but the context
    assert L.nwq_set_cloud(None, None, 5, 0) == BAD and L.nwq_set_cloud(None, p(xyz), 0, 0) == BAD
    assert L.nwq_set_cloud(None, p(xyz), (1 << 30) + 1, 0) == BAD and L.nwq_set_cloud(None, p(xyz), 5, 2) == BAD
    for bad in (np.nan, np.inf, -np.inf):
        q = xyz.copy()
        q[3, 1] = bad
        assert L.nwq_set_cloud(None, p(q), 5, 0) == C.NWQ_ERR_NONFINITE

    def e(radii, m=None):
        r = np.ascontiguousarray(radii, np.float64)
        return L.nwq_set_edges(None, p(r) if len(r) else None, len(r) if m is None else m)
    assert e([1.0, 2.0]) == BAD                                                                          # all is well but the context
    assert e([1.0], m=0) == BAD and e([]) == BAD                                                         # m = 0
    assert e(np.arange(1.0, 66.0)) == BAD                                                                # m = 65
    assert e([1.0, np.nan]) == BAD and e([np.nan]) == BAD and e([1.0, np.inf]) == BAD                    # NaN, infinity
    assert e([2.0, 1.0]) == BAD and e([1.0, 3.0, 2.0]) == BAD                                            # descending radii
    assert e([-1.0, 1.0]) == BAD and e([-0.5]) == BAD                                                    # negative radii
    assert e([1.0, 1.0]) == BAD and e([1e-200, 2e-200]) == BAD                                           # equal squares
    assert e([2.0 ** 40 * 1.0000001]) == BAD
    assert L.nwq_set_edges(None, None, 3) == BAD

    hist, local, info = np.full(4, 7, np.uint64), np.full((5, 4), 7, np.uint32), np.full(C.NWQ_INFO_WORDS, -7, np.int64)

    def c(q=p(xyz), nq=5, dev=0, h=p(hist), i=p(info)):
        return L.nwq_count(None, q, nq, dev, h, p(local), i)
    assert c() == BAD and c(q=None, nq=0) == BAD                                                         # all is well but the context
    assert c(h=None) == BAD and c(i=None) == BAD and c(dev=2) == BAD
    assert c(nq=0) == BAD and c(nq=(1 << 30) + 1) == BAD and c(q=None, nq=-1) == BAD
    q = xyz.copy()
    q[2, 2] = np.nan
    assert c(q=p(q)) == C.NWQ_ERR_NONFINITE
    assert (hist == 7).all() and (local == 7).all() and (info == -7).all()                              # nothing was written
    h = ctypes.c_void_p()
    assert L.nwq_create(-1, ctypes.byref(h)) == BAD and L.nwq_create(0, None) == BAD
    assert L.nwq_last_error(None) == b'null ctx'


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import pairs as C
    pts = np.random.default_rng(0).normal(size=(40, 3)).astype(np.float32)
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2]}
    with pytest.raises(RuntimeError):
        C.PairContext()
    with pytest.raises(RuntimeError):
        C.pair_counts(pts, [0.5, 1.0])
    with pytest.raises(RuntimeError):
        C.pair_counts(pts[:5], [0.5, 1.0], other=pts, local=True)
    with pytest.raises(RuntimeError):
        C.ripley(pts, [0.5, 1.0])
    with pytest.raises(RuntimeError):
        C.pair_correlation(pts, 2.0, 8)
    with pytest.raises(RuntimeError):
        C.PairwiseDistanceHistogram().execute({'filtered_localizations': table})
    with pytest.raises(RuntimeError):
        C.RipleysK(local_radius=1.0).execute({'filtered_localizations': table})
    assert not [n for n in dir(C) if 'sklearn' in n.lower() or 'scipy' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]
    src = open(C.__file__).read()
    assert 'scipy' not in src and 'cKDTree' not in src and 'sklearn' not in src


def test_the_normalisations_say_what_they_are_and_check_their_arguments():
    import inspect
    from ch_shrinkwrap_amd import pairs as C
    for f in (C.ripley, C.pair_correlation):
        assert 'NO EDGE CORRECTION' in f.__doc__ and 'no exactness claim' in f.__doc__
    assert list(inspect.signature(C.pair_counts).parameters)[:5] == ['points', 'edges', 'other', 'local', 'context']
    assert list(inspect.signature(C.ripley).parameters)[:6] == ['points', 'radii', 'other', 'dim', 'volume', 'local']
    flat = np.zeros((10, 3), np.float32)
    flat[:, :2] = np.random.default_rng(1).normal(size=(10, 2))
    with pytest.raises(ValueError, match='volume'):              # a zero extent asks for volume, before anything touches a GPU
        C.ripley(flat, [1.0])
    with pytest.raises(ValueError, match='volume'):
        C.pair_correlation(flat, 1.0, 4)
    with pytest.raises(ValueError):
        C.ripley(flat, [1.0], dim=4)
    with pytest.raises(ValueError):
        C.pair_correlation(flat, 1.0, 65, volume=1.0)
    m = C.RipleysK()
    assert (m.input, m.output, m.output_local, m.local_radius, m.dim) == ('filtered_localizations', 'ripleys_k', 'ripley_localizations', None, 3)
    assert C.PairwiseDistanceHistogram(n_bins=12).n_bins == 12 and C.PairwiseDistanceHistogram().output == 'pair_histogram'
    with pytest.raises(AttributeError):
        C.RipleysK(r_maxx=3.0)
