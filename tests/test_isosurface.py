"""Density isosurface (include/nw_isosurface.h), what can be checked without a GPU: the C-ABI's exports and argument checks, the absence of a
CPU fallback, and the NumPy restatement (tests/isosurface_ref.py) against the true surfaces and against synth.isosurface_mesh."""
import ctypes
import os
import re

import numpy as np
import pytest

import isosurface_ref as R
from isosurface_ref import scene, reference
from ch_shrinkwrap_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 10.0


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------
def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_isosurface.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwi_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_binding_matches_its_header():
    from ch_shrinkwrap_amd import build, isosurface as I
    build.build_hip_library()
    assert sorted(I.SYMBOLS) == _declared()
    L = I.load()
    assert L.nwi_abi_version() == I.ABI_VERSION == 1
    hdr = open(os.path.join(ROOT, 'include', 'nw_isosurface.h')).read()
    assert int(re.search(r'#define NWI_ABI_VERSION (\d+)', hdr).group(1)) == I.ABI_VERSION
    assert int(re.search(r'#define NWI_MAX_PASSES (\d+)', hdr).group(1)) == I.MAX_PASSES
    # the status codes of the binding are the header's
    for name, val in re.findall(r'(NWI_[A-Z_]+) = (-?\d+)', hdr):
        assert getattr(I, name) == int(val), name


def test_nothing_was_added_to_the_main_header():
    assert 'nwi_' not in open(os.path.join(ROOT, 'include', 'nanowrap.h')).read()


def test_every_kernel_of_the_unit_is_budgeted():
    from ch_shrinkwrap_amd import build
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_isosurface.hip')).read()
    kernels = re.findall(r'__global__[^;{]*?void\s+(\w+)\s*\(', src)
    assert len(kernels) >= 9 and len(set(kernels)) == len(kernels)
    for k in kernels:
        assert k in build.KERNEL_BUDGETS, k
    assert build.OBJ_ISOSURFACE in build.BUDGETED_OBJECTS
    assert any(u[1] == build.OBJ_ISOSURFACE and '-ffp-contract=off' in u[3] for u in build.UNITS)


def test_binding_checks_its_arguments_before_it_touches_a_gpu():
    """NULL pointers, h <= 0, an oversize grid, a point outside the grid and a NaN point come back with their status with no context at
    all, i.e. before any HIP call; with valid arguments and no GPU there is no context to be had: no CPU fallback."""
    from ch_shrinkwrap_amd import isosurface as I
    L = I.load()
    P = lambda a: a.ctypes.data
    pts = np.array([[5.0, 5.0, 5.0], [25.0, 15.0, 35.0]], np.float32)
    lo = np.zeros(3, np.float32)
    dims = np.array([4, 4, 4], np.int32)
    BAD = I.NWI_ERR_BADARG
    assert L.nwi_density(None, None, 2, 0, P(lo), 10.0, P(dims), 2, None, None) == BAD
    assert L.nwi_density(None, P(pts), 2, 0, None, 10.0, P(dims), 2, None, None) == BAD
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), 10.0, None, 2, None, None) == BAD
    assert L.nwi_density(None, P(pts), 0, 0, P(lo), 10.0, P(dims), 2, None, None) == BAD
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), 0.0, P(dims), 2, None, None) == BAD                    # h <= 0
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), -1.0, P(dims), 2, None, None) == BAD
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), float('nan'), P(dims), 2, None, None) == BAD
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), 10.0, P(dims), I.MAX_PASSES + 1, None, None) == BAD
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), 10.0, P(dims), -1, None, None) == BAD
    big = np.array([1025, 1024, 1024], np.int32)                                                           # more than 2^30 voxels
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), 10.0, P(big), 2, None, None) == BAD
    thin = np.array([4, 2, 4], np.int32)
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), 10.0, P(thin), 2, None, None) == BAD
    outside = pts.copy()
    outside[1, 0] = 40.0                                                                                   # voxel 4 of 4
    assert L.nwi_density(None, P(outside), 2, 0, P(lo), 10.0, P(dims), 2, None, None) == I.NWI_ERR_OUTSIDE
    outside[1, 0] = -0.5
    assert L.nwi_density(None, P(outside), 2, 0, P(lo), 10.0, P(dims), 2, None, None) == I.NWI_ERR_OUTSIDE
    nan = pts.copy()
    nan[0, 2] = np.nan
    assert L.nwi_density(None, P(nan), 2, 0, P(lo), 10.0, P(dims), 2, None, None) == I.NWI_ERR_NONFINITE
    assert L.nwi_density(None, P(pts), 2, 0, P(lo), 10.0, P(dims), 2, None, None) == BAD                    # all valid: the NULL context is what is left
    # the table
    tab = I.sheet_table()
    assert tab.shape == (256, 12) and tab.dtype == np.int8
    assert L.nwi_set_sheet_table(None, None) == BAD
    wrong = tab.copy()
    wrong[1, 0] = -1                                                                                        # pattern 1 crosses edge 0
    assert L.nwi_set_sheet_table(None, P(wrong)) == BAD
    wrong = tab.copy()
    wrong[0, 3] = 3                                                                                         # pattern 0 crosses nothing
    assert L.nwi_set_sheet_table(None, P(wrong)) == BAD
    assert L.nwi_set_sheet_table(None, P(tab)) == BAD                                                       # a good table, no context
    thr = ctypes.c_uint64()
    assert L.nwi_threshold_auto(None, 0.3, None, None, None, None) == BAD
    assert L.nwi_threshold_auto(None, -1.0, None, ctypes.byref(thr), None, None) == BAD
    assert L.nwi_threshold_auto(None, float('nan'), None, ctypes.byref(thr), None, None) == BAD
    n = ctypes.c_int64()
    assert L.nwi_extract(None, 5, None, ctypes.byref(n)) == BAD
    assert L.nwi_extract(None, 5, ctypes.byref(n), ctypes.byref(n)) == BAD
    assert L.nwi_get(None, None, None, None) == BAD
    assert L.nwi_create(-1, ctypes.byref(ctypes.c_void_p())) == BAD
    assert L.nwi_create(0, None) == BAD


def test_without_a_gpu_there_is_no_fallback():
    import torch
    from ch_shrinkwrap_amd import isosurface as I
    with pytest.raises(AttributeError):
        I.DensitySurface(no_such_parameter=1)
    mod = I.DensitySurface()
    assert (mod.input, mod.output, mod.threshold_density, mod.remesh, mod.voxel_size, mod.passes, mod.cull_inner_surfaces) == \
        ('filtered_localizations', 'surf', None, True, None, 2, True)
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        assert I.load().nwi_create(0, ctypes.byref(h)) == I.NWI_ERR_HIP and h.value is None
        with pytest.raises(RuntimeError):
            I.IsosurfaceContext()
        pts = scene('c1')[0]
        ns = {'filtered_localizations': {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': np.full(pts.shape[0], 10.0, 'f4')}}
        with pytest.raises(RuntimeError):
            mod.execute(ns)
        assert 'surf' not in ns


def test_shrinkwrap_membrane_still_needs_its_surface():
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    with pytest.raises(KeyError):
        ShrinkwrapMembrane().execute({'filtered_localizations': {}})


# ---- the grid and the voxel-size rule ---------------------------------------------------------------------------------------------------
def test_grid_holds_the_cloud_with_its_padding():
    from ch_shrinkwrap_amd import isosurface as I
    for name, shift in (('c1', (0, 0, 0)), ('c1', (5e3, -3e3, 1e3))):
        pts = scene(name)[0] + np.array(shift, 'f4')
        lo, dims = I.grid_for(pts, 10.0, 5)
        assert lo.dtype == np.float32 and dims.dtype == np.int32
        v = R.voxels(pts, lo, 10.0, dims)
        assert v.min() >= 4 and (v.max(0) <= dims - 5).all()
    assert I.pick_voxel_size(pts, np.full(7, 10.0)) == 10.0
    h = I.pick_voxel_size(scene('c1')[0])
    assert 5.0 < h < 40.0


# ---- the reference alone, against the truth -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,chi', [('c1', 2), ('c1_background', 2), ('c4', -2)])
def test_reference_gives_one_outer_sheet_of_the_right_genus_just_outside_the_truth(name, chi):
    pts, sdf, h = scene(name)
    v, f, keys, info = reference(name)
    assert (R.edge_use(f) == 2).all()                                         # closed 2-manifold: every edge used exactly twice
    assert (np.diff(keys) > 0).all()
    comps = R.components(v, f)
    outer = [c for c in comps if c[2] > 0]
    print(name, 'h', h, 'vertices/faces', v.shape[0], f.shape[0], 'components (faces, chi, volume)', [(c[0].size, c[1], c[2]) for c in comps])
    assert len(outer) == 1
    ids, got_chi, vol = outer[0]
    assert got_chi == chi
    d = sdf(v[np.unique(f[ids])].astype('f8'))
    print(name, 'true SDF of the outer sheet: %.1f ... %.1f nm, bound %.0f' % (d.min(), d.max(), 4 * h + 2 * SIGMA))
    assert d.min() > 0.0 and d.max() <= 4 * h + 2 * SIGMA
    if name == 'c1_background':                                               # isolated points stay below the threshold: nothing new appears
        assert len(comps) == len(R.components(*reference('c1')[:2]))


def test_integer_field_keeps_the_mass_and_the_median_rule():
    pts, sdf, h = scene('c1')
    info = reference('c1')[3]
    assert info['field'].dtype == np.uint64 and info['counts'].dtype == np.uint32
    assert int(info['counts'].sum()) == pts.shape[0]
    assert int(info['field'].sum()) == pts.shape[0] * 4 ** 6                  # nothing reaches the border: the weights sum to 4^(3 passes)
    vals = np.sort(info['field'][info['counts'] > 0])
    assert info['median'] == vals[(vals.size - 1) // 2] and info['thr'] == int(np.floor(0.3 * float(info['median'])))
    with pytest.raises(ValueError):
        R.count(pts, info['lo'], h, info['dims'] - np.array([8, 0, 0]))
    # a threshold of 0 on a grid padded by `passes` only does touch the outermost layer
    from ch_shrinkwrap_amd.isosurface import grid_for
    lo, dims = grid_for(pts, h, 2)
    f2, _ = R.density(pts, lo, h, dims, 2)
    with pytest.raises(ValueError):
        R.surface_nets(f2, 0, lo, h)


# ---- the reference against the package's other mesher ------------------------------------------------------------------------------------
def _lattice_sdf(field, lo, h):
    """-field at the lattice node nearest to a point, 0 (outside) beyond the lattice: isosurface_mesh(level=-thr) then sees `field > thr`
    as inside and places its crossings at (f0 - thr) / (f0 - f1)."""
    nz, ny, nx = field.shape
    origin = np.asarray(lo, 'f8') + 0.5 * h

    def sdf(p):
        g = np.rint((np.asarray(p, 'f8') - origin[None, :]) / h).astype(np.int64)
        ok = (g >= 0).all(1) & (g[:, 0] < nx) & (g[:, 1] < ny) & (g[:, 2] < nz)
        out = np.zeros(g.shape[0])
        out[ok] = -field[g[ok, 2], g[ok, 1], g[ok, 0]].astype('f8')
        return out
    return sdf, origin


@pytest.mark.parametrize('name', ['c1', 'c4'])
def test_reference_agrees_with_isosurface_mesh_on_the_same_field(name):
    """Same vertex and face counts, same keys, same Euler characteristic; positions to 8 float32 ulp of the largest coordinate: a vertex
    is a mean of at most 12 float32 terms in [0, 1] (each within a few 2^-24) added to a cell index and scaled, four roundings of at most
    half an ulp of the coordinate each, against the same mean in float64 rounded to float32 once."""
    v, f, keys, info = reference(name)
    h, dims = info['h'], info['dims']
    sdf, origin = _lattice_sdf(info['field'], info['lo'], h)
    mv, mf = synth.isosurface_mesh(sdf, origin, origin + (dims - 1.5) * h, h, level=-float(info['thr']), slack=1e30, project=0)
    assert mv.shape == v.shape and mf.shape == f.shape
    tol = 8 * float(np.spacing(np.float32(np.abs(v).max())))
    err = float(np.abs(mv.astype('f8') - v.astype('f8')).max())
    print(name, 'max position difference %.3g nm, bound %.3g nm' % (err, tol))
    assert err <= tol                                                          # (isosurface_mesh's vertices are in key order as well)
    from ch_shrinkwrap_amd.surgery import euler_characteristic
    assert euler_characteristic(mf) == euler_characteristic(f)
    assert (R.edge_use(mf) == 2).all()


def test_two_sheets_through_one_cell_do_not_share_a_vertex():
    """Two inside nodes at opposite corners of one cell: plain surface nets would join the two blobs at one vertex."""
    field = np.zeros((6, 6, 6), np.uint64)
    field[2, 2, 2] = field[3, 3, 3] = 100
    v, f, keys = R.surface_nets(field, 50, np.zeros(3, 'f4'), 1.0)
    comps = R.components(v, f)
    assert (R.edge_use(f) == 2).all() and len(comps) == 2 and all(c[1] == 2 and c[2] > 0 for c in comps)
    cell = ((2 * 5) + 2) * 5 + 2
    assert sorted(keys[(keys // 16) == cell] % 16) == [0, 3]                    # the middle cell carries two vertices
    assert v.shape[0] == 2 * 8 and f.shape[0] == 2 * 12


def test_gpu_tests_read_nothing_outside_the_repository():
    for name in ('test_hip_isosurface.py', 'isosurface_ref.py'):
        src = open(os.path.join(ROOT, 'tests', name)).read()
        assert '/root/' + 'reference' not in src and 'oracle/' + '_ref' not in src and '_' + 'ref/' not in src, name
