"""CPU tests of the k-th-neighbour unit: libnanowrap_hip.so exports what include/nw_neighbours.h declares and the binding names the same
set; the unit is built without fma contraction and its kernels stay within their budgets without scratch; arguments are refused before
any HIP call; the NumPy restatement (tests/neighbours_ref.py) agrees with scipy's cKDTree; every input of the GPU module reaches the
branch it is named for; and the restatement's level sets have the topology the feature exists for."""
import ctypes
import os
import re

import numpy as np
import pytest

from ch_shrinkwrap_amd import neighbours as N
import isosurface_ref as IR
import neighbours_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_kn_queries', 'k_kn_nodes']
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _declared(header, prefix):
    txt = open(os.path.join(ROOT, 'include', header)).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-zA-Z0-9_]+)\s*\(' % prefix, txt)))


def test_library_exports_the_neighbours_header():
    from ch_shrinkwrap_amd import build, _lib
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared('nw_neighbours.h', 'nwk_')
    assert len(names) == 8
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(N.SYMBOLS) == names
    assert N.load().nwk_abi_version() == N.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_neighbours.h')).read()
    for name, value in (('NWK_MAX_K', N.MAX_K), ('NWK_FIELD_SHIFT', N.FIELD_SHIFT), ('NWK_ABI_VERSION', N.ABI_VERSION)):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == value
    assert N.MAX_K == R.MAX_K == 32
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOCLOUD'):
        assert int(re.search(r'NWK_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(N, 'NWK_ERR_' + name)
    assert N.load().nwk_field_ptr.restype is ctypes.c_void_p            # a pointer, not the int of the other entry points


def test_set_field_is_an_addition_to_the_isosurface_abi():
    from ch_shrinkwrap_amd import isosurface as I
    assert 'nwi_set_field' in I.SYMBOLS and sorted(I.SYMBOLS) == _declared('nw_isosurface.h', 'nwi_')
    L = I.load()
    assert L.nwi_abi_version() == 1
    lo, dims, f = np.zeros(3, np.float32), np.array([4, 4, 4], np.int32), np.zeros((4, 4, 4), np.uint64)
    BAD = I.NWI_ERR_BADARG
    assert L.nwi_set_field(None, None, 0, P(lo), 1.0, P(dims)) == BAD
    assert L.nwi_set_field(None, P(f), 2, P(lo), 1.0, P(dims)) == BAD
    assert L.nwi_set_field(None, P(f), 0, None, 1.0, P(dims)) == BAD
    assert L.nwi_set_field(None, P(f), 0, P(lo), 0.0, P(dims)) == BAD
    assert L.nwi_set_field(None, P(f), 0, P(lo), float('nan'), P(dims)) == BAD
    assert L.nwi_set_field(None, P(f), 0, P(lo), 1.0, None) == BAD
    assert L.nwi_set_field(None, P(f), 0, P(lo), 1.0, P(np.array([2, 4, 4], np.int32))) == BAD
    assert L.nwi_set_field(None, P(f), 0, P(lo), 1.0, P(np.array([2048, 1024, 1024], np.int32))) == BAD
    assert L.nwi_set_field(None, P(f), 0, P(np.array([0, np.inf, 0], np.float32)), 1.0, P(dims)) == BAD
    assert L.nwi_set_field(None, P(f), 0, P(lo), 1.0, P(dims)) == BAD                  # all valid: the NULL context is what is left


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_NEIGHBOURS]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_neighbours_core.h') in unit[0][2]            # rebuilt when the core changes
    assert build.OBJ_NEIGHBOURS in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_NEIGHBOURS)
    assert sorted(in_object) == sorted(KERNELS)                 # every kernel of the unit has a row, and no row is stale
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_neighbours.hip')).read()
    assert sorted(re.findall(r'__global__[^;{]*?void\s+(\w+)\s*\(', src)) == sorted(KERNELS)
    assert sorted(k for k in build.KERNEL_BUDGETS if k.startswith('k_kn_')) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)
        assert r['lds'] == 128 * N.MAX_K * 8                    # the lists are in LDS: [slot][lane] doubles
        assert r['lds'] <= 64 * 1024


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check comes before the first use of the context."""
    L = N.load()
    BAD = N.NWK_ERR_BADARG
    pts = np.zeros((4, 3), np.float32)
    out = np.zeros(4)
    inf = float('inf')
    assert L.nwk_set_cloud(None, None, 4, 0) == BAD
    assert L.nwk_set_cloud(None, P(pts), 0, 0) == BAD
    assert L.nwk_set_cloud(None, P(pts), (1 << 30) + 1, 0) == BAD
    assert L.nwk_set_cloud(None, P(pts), 4, 2) == BAD
    nan = pts.copy()
    nan[2, 1] = np.nan
    assert L.nwk_set_cloud(None, P(nan), 4, 0) == N.NWK_ERR_NONFINITE
    assert L.nwk_set_cloud(None, P(pts), 4, 0) == BAD                                 # all is well but the context
    assert L.nwk_kth_distance(None, None, 4, 0, 1, inf, P(out)) == BAD
    assert L.nwk_kth_distance(None, P(pts), 4, 0, 1, inf, None) == BAD
    assert L.nwk_kth_distance(None, P(pts), 0, 0, 1, inf, P(out)) == BAD
    assert L.nwk_kth_distance(None, P(pts), 4, 3, 1, inf, P(out)) == BAD
    for k in (0, -1, N.MAX_K + 1):
        assert L.nwk_kth_distance(None, P(pts), 4, 0, k, inf, P(out)) == BAD
    for cap in (0.0, -1.0, float('nan')):
        assert L.nwk_kth_distance(None, P(pts), 4, 0, 1, cap, P(out)) == BAD
    assert L.nwk_kth_distance(None, P(nan), 4, 0, 1, inf, P(out)) == N.NWK_ERR_NONFINITE
    assert L.nwk_kth_distance(None, P(pts), 4, 0, N.MAX_K, inf, P(out)) == BAD        # the NULL context
    lo, dims = np.zeros(3, np.float32), np.array([4, 4, 4], np.int32)
    assert L.nwk_node_field(None, None, 1.0, P(dims), 1, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), 1.0, None, 1, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), 0.0, P(dims), 1, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), float('nan'), P(dims), 1, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), 1.0, P(dims), 0, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), 1.0, P(dims), N.MAX_K + 1, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), 1.0, P(dims), 1, inf, None) == BAD            # the field needs a finite cap ...
    assert L.nwk_node_field(None, P(lo), 1.0, P(dims), 1, 2.0 ** 41, None) == BAD      # ... of at most 2^40
    assert L.nwk_node_field(None, P(lo), 1.0, P(np.array([2, 4, 4], np.int32)), 1, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), 1.0, P(np.array([2048, 1024, 1024], np.int32)), 1, 5.0, None) == BAD
    assert L.nwk_node_field(None, P(lo), 1.0, P(dims), 1, 5.0, None) == BAD            # the NULL context
    assert L.nwk_field_ptr(None) is None
    h = ctypes.c_void_p()
    assert L.nwk_create(-1, ctypes.byref(h)) == BAD and L.nwk_create(0, None) == BAD


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import isosurface as I
    h = ctypes.c_void_p()
    assert N.load().nwk_create(0, ctypes.byref(h)) == N.NWK_ERR_HIP and h.value is None
    pts = R.sphere_cloud(300, 1)
    for call in (lambda: N.kth_distance(pts, k=3), lambda: N.local_density(pts), lambda: I.knn_isosurface(pts, 10.0),
                 lambda: I.start_surface(pts, 10.0, method='knn'),
                 lambda: I.DensitySurface(method='knn').execute({'filtered_localizations': {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2]}})):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        I.start_surface(pts, 10.0, method='octree')
    with pytest.raises(ValueError):
        N.local_density(pts[:20], 20)                           # n <= k: no k-th neighbour, said before any context is made
    d = I.DensitySurface()
    assert d.method == 'grid' and d.n_points_min == 20          # the defaults are today's path


def test_python_side_rules():
    from ch_shrinkwrap_amd import isosurface as I
    assert np.array_equal(N.knn_density(np.array([0.0, 1.0, 2.0]), 3), [np.inf, 3 / (4 / 3 * np.pi), 3 / (4 / 3 * np.pi * 8)])
    for h, k, td in ((10.0, 20, 2e-3), (8.0, 20, 5e-6), (7.3, 5, 1.234e-4)):
        assert I.knn_threshold(h, k, td) == R.knn_threshold(h, k, td)
        R_thr, r_cap, pad, thr = I.knn_threshold(h, k, td)
        assert r_cap == R_thr + 2 * h and (pad - 0.5) * h > R_thr + h and thr == int(np.floor((r_cap - R_thr) * 2 ** 20))
        assert abs(k / (4 / 3 * np.pi * R_thr ** 3) - td) < 1e-12 * td
    # upstream's sweep at n_points_min = 20: smoothing radii from 13 nm to 98 nm, whatever the voxel size
    assert 13 < I.knn_threshold(10.0, 20, 2e-3)[0] < 14 and 98 < I.knn_threshold(10.0, 20, 5e-6)[0] < 99
    with pytest.raises(ValueError):
        I.knn_threshold(10.0, 20, np.inf)


def test_restatement_agrees_with_ckdtree():
    from scipy.spatial import cKDTree
    pts = R.random_cloud(3000, 11)
    q = R.queries_around(pts, 700, 12)
    tree = cKDTree(pts.astype(np.float64))
    for k in (1, 2, 20, 32):
        d = tree.query(q.astype(np.float64), k=k)[0].reshape(q.shape[0], -1)[:, -1]
        r = R.kth_distance(pts, q, k)
        nz = d > 0
        assert (np.abs(r[nz] - d[nz]) <= 1e-12 * d[nz]).all() and (r[~nz] == 0).all() and (~nz).sum() >= (175 if k == 1 else 0)
        assert np.array_equal(R.kth_distance(pts, q, k, 50.0), np.minimum(r, 50.0))
    assert np.isinf(R.kth_distance(pts[:5], q[:3], 6)).all() and (R.kth_distance(pts[:5], q[:3], 6, 9.0) == 9.0).all()
    # the order of the cloud does not show
    assert np.array_equal(R.kth_distance(pts[::-1], q, 20), R.kth_distance(pts, q, 20))
    # local density: the point itself is the first neighbour
    dens = R.local_density(pts, 20)
    d21 = tree.query(pts.astype(np.float64), k=21)[0][:, -1]
    assert np.allclose(dens, 20 / (4 / 3 * np.pi * d21 ** 3), rtol=1e-11)


# ---- every input of tests/test_hip_neighbours.py reaches the branch it is named for ---------------------------------------------------------
def test_lattice_queries_tie():
    pts, q = R.lattice_case()
    d2 = R.dist2(pts, q.astype(np.float64))
    d2.sort(axis=1)
    ties_first = (d2 == d2[:, :1]).sum(1)
    assert set(ties_first.tolist()) == {8, 4, 2}               # cell centres, face centres, edge centres
    for k in (1, 2, 20, 32):
        kth = d2[:, k - 1]
        # at many queries the k-th smallest distance is shared with the (k+1)-th: a rule that broke ties by order would show
        assert (d2[:, k] == kth).sum() > q.shape[0] // 3


def test_copies_flat_far_and_cap_inputs():
    p, q = R.copies_case()
    assert p.shape[0] == 300 and len(np.unique(p, axis=0)) == 1
    assert (R.kth_distance(p, q, 32) == [0.0, 1.0, np.sqrt(12.5 ** 2 + 7.25 ** 2 + 9.0)]).all()
    for kind, flat_axes in (('plane', 1), ('axis', 2), ('diagonal', 0)):
        p, q = R.flat_case(kind)
        ext = p.max(0) - p.min(0)
        assert (ext == 0).sum() == flat_axes                    # the cell grid is one cell thick along these axes
        if kind == 'diagonal':
            assert (p[:, 0] == p[:, 1]).all() and (p[:, 0] == p[:, 2]).all()
        assert (R.kth_distance(p, q[:40], 1) == 0).all()
    p, q, diag = R.far_case()
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    out = np.linalg.norm(q - np.clip(q, lo, hi), axis=1)
    assert (out > 10 * diag).all()
    res = {}
    for where in ('below', 'at', 'above'):
        p, q, k, r_cap = R.cap_case(where)
        d = np.sort(np.sqrt(R.dist2(p, q.astype(np.float64))[0]))
        assert (d[:19] < 1.0).all() and d[19] == 40.0 and d[20] > 80.0
        res[where] = (float(R.kth_distance(p, q, k, r_cap)[0]), r_cap)
    assert res['below'][0] == 40.0 < res['below'][1] and abs(40.0 / res['below'][1] - 0.999) < 1e-15
    assert res['at'][0] == 40.0 == res['at'][1]                 # the twentieth at exactly the cap: unclamped and clamped agree
    assert res['above'][0] == res['above'][1] < 40.0            # clamped
    # with the cap out of the way the same cloud gives 40 in all three
    assert R.kth_distance(p, q, 20)[0] == 40.0 and R.kth_distance(p, q, 21)[0] > 80.0


def test_node_inputs():
    for name, shape in R.NODE_GRIDS.items():
        p, lo, h, dims = R.node_case(name)
        assert tuple(dims) == shape and IR.inside_grid(p, lo, h, dims).all()
        f = R.node_field(p, lo, h, dims, 3, 4.0)
        assert f.shape == shape[::-1] and (f == 0).any() and (f > 0).any()             # clamped nodes and unclamped ones
    p, lo, h, dims, index = R.coincident_node_case()
    x = R.node_positions(lo, h, dims).reshape(dims[2], dims[1], dims[0], 3)[index[2], index[1], index[0]]
    assert np.array_equal(x, p[17].astype(np.float64))          # the node is a cloud point, bit for bit
    assert R.node_field(p, lo, h, dims, 1, 6.0)[index[2], index[1], index[0]] == 6 << 20


# ---- what the feature exists for ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,chi', [('sphere', 2), ('torus', 0)])
@pytest.mark.parametrize('n', [300, 1000, 5000])
def test_level_set_of_the_restatement_has_the_shapes_topology(shape, chi, n):
    """k = 20, threshold 0.3 x the median local density, fixed voxels (10 nm sphere, 8 nm torus): the outer component is a sphere resp. a
    torus at every N, while R_thr moves by itself.  The seeds in neighbours_ref.TOPOLOGY_CASES were chosen with this restatement alone,
    and it was checked on it that each of them gives what is asserted here (most seeds do; the 300-point torus closes its hole at one
    of the three tried, where R_thr exceeds the hole's radius)."""
    v, f, keys, info = R.topology_reference(shape, n)
    got, vol = R.outer_component(v, f)
    print(shape, n, 'R_thr %.1f nm, outer component: Euler characteristic %d, volume %.3g nm^3' % (info['R_thr'], got, vol))
    assert got == chi and vol > 0
    assert (IR.edge_use(f) == 2).all() and IR.directed_edges_balanced(f)
    lo, hi = {300: (60, 90), 1000: (35, 55), 5000: (15, 30)}[n]                        # the bandwidth follows the cloud
    assert lo < info['R_thr'] < hi
    # no node of the outermost layer is inside, and the outer node of every crossed edge is below the cap (so no crossing is clamped)
    field = info['field']
    inside = field > np.uint64(info['thr'])
    for ax in range(3):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        crossed = inside[tuple(a)] != inside[tuple(b)]
        assert (np.minimum(field[tuple(a)], field[tuple(b)])[crossed] > 0).all()


def test_grid_chain_fails_where_the_knn_chain_holds():
    """The 300-point sphere at h = 10 nm: two rounds of [1 2 1] at this voxel size do not bridge the gaps between the localizations."""
    pts = R.topology_cloud('sphere', 300)
    v, f, _, _ = IR.isosurface(pts, R.TOPOLOGY_H['sphere'], passes=2, fraction=0.3)
    chi, vol = R.outer_component(v, f)
    print('grid chain on the 300-point sphere: Euler characteristic %d' % chi)
    assert chi != 2
    assert R.outer_component(*R.topology_reference('sphere', 300)[:2])[0] == 2
