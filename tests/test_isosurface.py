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


# ---- the premises of the edge cases (tests/test_hip_isosurface_edges.py), on the reference alone ----------------------------------------
NOISE_SEEDS = (0, 1, 2)


@pytest.mark.parametrize('seed', NOISE_SEEDS)
def test_noise_fields_reach_every_pattern_and_every_sheet_count(seed):
    """Counts uniform in 0..3 at thr = 1: all 256 patterns, cells with two, three and four sheets, a quarter of the nodes equal to thr.
    The nets of such a field are closed and oriented but not manifold: an edge is used twice or four times (README, start surface)."""
    pts, lo, h, dims, counts = R.noise_case(seed)
    assert np.array_equal(R.count(pts, lo, h, dims), counts) and counts[1:-1, 1:-1, 1:-1].max() == 3
    assert len(set(int(d) for d in dims)) == 3 and int(np.prod(dims - 1)) > 2048
    field = R.smooth(counts, 0)
    patterns, sheets = R.sheet_census(field, 1)
    print('seed', seed, 'points', pts.shape[0], 'cells with 0..4 sheets', sheets.tolist(), 'nodes equal to thr', int((field == 1).sum()))
    assert patterns == set(range(256)) and (sheets[2:] >= 1).all()
    assert 0.2 < (field[1:-1, 1:-1, 1:-1] == 1).mean() < 0.3
    v, f, keys = R.surface_nets(field, 1, lo, h)
    use = R.edge_use(f)
    assert (use % 2 == 0).all() and set(use.tolist()) == {2, 4}
    assert R.directed_edges_balanced(f)
    assert not R.directed_edges_balanced(f[:-1])                               # (the measure does tell)
    # one voxel earlier along x: the same surface, the other diagonal of every quad
    pts1, lo1, _, dims1, counts1 = R.noise_case(seed, shifted=True)
    assert np.array_equal(R.count(pts1, lo1, h, dims1), counts1)
    v1, f1, _ = R.surface_nets(R.smooth(counts1, 0), 1, lo1, h)
    assert f1.shape == f.shape and float(np.abs(v1.astype('f8') - v.astype('f8')).max()) <= R.position_bound(v)     # (lo - 1 + (i + 1) rounds apart from lo + i)
    assert np.array_equal(f1[0::2, 0], f[0::2, 0]) and (f1[0::2, 2] != f[0::2, 2]).all()


@pytest.mark.parametrize('seed', NOISE_SEEDS)
def test_reference_agrees_with_isosurface_mesh_on_every_pattern(seed):
    """The noise fields through the package's other mesher, as test_reference_agrees_with_isosurface_mesh_on_the_same_field does for the
    smooth scenes (same bound, same derivation).  Both use an edge four times where two cells share an ambiguous face."""
    pts, lo, h, dims, counts = R.noise_case(seed)
    field = R.smooth(counts, 0)
    v, f, keys = R.surface_nets(field, 1, lo, h)
    sdf, origin = _lattice_sdf(field, lo, h)
    mv, mf = synth.isosurface_mesh(sdf, origin, origin + (dims - 1.5) * h, h, level=-1.0, slack=1e30, project=0)
    assert mv.shape == v.shape and mf.shape == f.shape
    tol = R.position_bound(v)
    err = float(np.abs(mv.astype('f8') - v.astype('f8')).max())
    print('seed', seed, 'vertices/faces', v.shape[0], f.shape[0], 'max position difference %.3g, bound %.3g' % (err, tol))
    assert err <= tol
    from ch_shrinkwrap_amd.surgery import euler_characteristic
    assert euler_characteristic(mf) == euler_characteristic(f)
    assert np.array_equal(np.sort(R.edge_use(mf)), np.sort(R.edge_use(f)))


@pytest.mark.parametrize('name', sorted(R.BORDER_GRIDS))
def test_border_grids_lose_mass_at_the_border(name):
    pts, lo, h, dims, counts = R.border_case(name)
    assert np.array_equal(R.count(pts, lo, h, dims), counts)
    n = pts.shape[0]
    assert counts[0, 0, 0] > 0 and counts[-1, -1, -1] > 0                       # two corners of the grid
    for passes in (0, 1, 5):
        field = R.smooth(counts, passes)
        mass = n * 4 ** (3 * passes)
        assert int(field.sum()) == mass if passes == 0 else int(field.sum()) < mass
        if name == '3x3x3' and passes == 5:
            assert (int(field.sum()), mass) == (1023641088, 11811160064)
        with pytest.raises(ValueError, match='outermost'):
            R.surface_nets(field, 0, lo, h)


def test_hash_cases_must_overflow_the_table_and_wrap_it():
    lin = np.arange(64 ** 3)
    assert int(R.home_slot(1)) == 2654435761 >> 21 and int(R.home_slot(123457)) == ((123457 * 2654435761) % 2 ** 32) >> 21
    per_slot = np.bincount(R.home_slot(lin).astype(np.int64), minlength=2048)
    assert per_slot.min() == 126 and per_slot.max() == 131
    for slots, per in (((1000,), 8), ((2047,), 8), ((2045, 2046, 2047), 3)):
        pts, lo, h, dims, vox = R.hash_case(slots, per)
        assert np.unique(vox).size == vox.size == per * len(slots)
        assert sorted(set(R.home_slot(vox).tolist())) == list(slots)
        xyz = np.stack([vox % 64, (vox // 64) % 64, vox // 4096], 1)
        assert xyz.min() >= 1 and xyz.max() <= 62                               # interior
        assert R.table_must_overflow(vox)
        first = R.voxels(pts[:1024], lo, h, dims)
        assert np.unique((first[:, 2] * 64 + first[:, 1]) * 64 + first[:, 0]).size == vox.size      # all of them in the first workgroup
        assert np.array_equal(np.flatnonzero(R.count(pts, lo, h, dims).ravel()), np.sort(vox))
    assert (R.home_slot(R.interior_voxels_with_home(R.HASH_DIMS, (2047,), 1000)) == 2047).sum() == 112
    assert not R.table_must_overflow(R.interior_voxels_with_home(R.HASH_DIMS, (1000,), 4))
    # two voxels of home slot 2047 cannot both stay there: one probes slot 0
    assert (R.home_slot(R.hash_case((2045, 2046, 2047), 3)[4]) == 2047).sum() >= 2


FACE_H = (0.1, 7.3, 12.0)
FACE_LO = ((0.0, 0.0, 0.0), (5e3, -3e3, 1e3))


@pytest.mark.parametrize('h', FACE_H)
@pytest.mark.parametrize('lo', FACE_LO)
def test_points_on_voxel_faces_mostly_stay_inside(h, lo):
    """The reference alone says which of the face points fall outside the 40^3 grid; fewer than 5 % do."""
    dims = np.array([40, 40, 40], np.int32)
    pts = R.face_points(lo, h, 40)
    keep = R.inside_grid(pts, lo, h, dims)
    v = R.voxel_coords(pts, lo, h)
    print('h', h, 'lo', lo, 'dropped', int((~keep).sum()), 'of', pts.shape[0], 'voxel coordinates', v.min(), '...', v.max())
    assert pts.shape == (360, 3) and (~keep).mean() < 0.05
    R.count(pts[keep], lo, h, dims)
    # one ulp below a face is the voxel before it, except where rounding says otherwise (at lo = 0 and h = 7.3 the point one ulp below
    # zero scales to -0 and stays in voxel 0); 1 / h is inexact in float32 for every h here
    k = np.arange(40)
    below, on = v[:40, 0], v[40:80, 0]
    assert (below <= on).all() and (below < on).any() and np.abs(on - k).max() <= 1
    assert float(np.float32(1.0) / np.float32(h)) != 1.0 / float(np.float32(h))
    for edge, ok in ((dims - 1, True), (dims, False), (np.array([-1, -1, -1]), False)):
        for d in range(3):
            p, coord = R.boundary_point(lo, h, dims, d, int(edge[d]))
            assert coord == edge[d] and bool(R.inside_grid(p, lo, h, dims)[0]) == ok


def test_select_cases_have_the_medians_they_are_named_for():
    want = {'one': 5, 'two': 3, 'all_equal': 6, 'odd': 4, 'even': 4, 'even_tie': 4, 'byte_ff': 255, 'ff_100': 255, 'three_bytes': 65536,
            'three_bytes_ffff': 65535, 'many': 255}
    assert sorted(want) == sorted(R.SELECT_VALUES)
    for name, med in want.items():
        pts, lo, h, dims, counts = R.select_case(name)
        assert np.array_equal(R.count(pts, lo, h, dims), counts)
        assert sorted(counts[counts > 0].tolist()) == sorted(R.SELECT_VALUES[name])
        assert counts[0].max() == counts[-1].max() == counts[:, 0].max() == counts[:, -1].max() == counts[:, :, 0].max() == counts[:, :, -1].max() == 0
        thr, m, occ = R.threshold_auto(R.smooth(counts, 0), counts, 1.0)
        assert (thr, m, occ) == (med, med, len(R.SELECT_VALUES[name])), name
        if name.startswith('three_bytes'):
            assert pts.shape[0] >= 65536                                        # the select starts at shift 16
    sv = sorted(R.SELECT_VALUES['even'])
    assert sv[(len(sv) - 1) // 2] != sv[len(sv) // 2]
    pts, lo, h, dims, counts = R.excluded_case()
    field = R.smooth(counts, 2)
    assert field[counts == 0].max() > field[counts > 0].min()                   # an empty voxel denser than an occupied one
    assert R.threshold_auto(field, counts, 1.0)[1:] == (int(np.sort(field[counts > 0])[1]), 3)
    assert int(np.sort(field[field > 0])[(int((field > 0).sum()) - 1) // 2]) != R.threshold_auto(field, counts, 1.0)[1]


def test_big_field_case_is_above_32_bits_and_smooth():
    pts, lo, h, dims, counts = R.big_field_case()
    field, c = R.density(pts, lo, h, dims, 5)
    assert np.array_equal(c, counts) and int(field.max()) > 2 ** 32
    peaks = sorted(int(x) for x in field[counts > 0])
    assert peaks[0] > 5000 * 252 ** 3 and peaks[1] > 6000 * 252 ** 3 and peaks[0] < peaks[1]
    thr = R.threshold_auto(field, counts, 0.3)[0]
    assert thr > 2 ** 32
    for t, ncomp in ((thr, None), ((peaks[0] + peaks[1]) // 2, 1)):
        v, f, k = R.surface_nets(field, t, lo, h)
        assert (R.edge_use(f) == 2).all() and R.directed_edges_balanced(f)
        if ncomp:
            assert len(R.components(v, f)) == ncomp


def test_carry_case_has_cells_past_two_to_the_21():
    import time
    pts, lo, h, dims, counts = R.carry_case()
    assert np.array_equal(R.count(pts, lo, h, dims), counts)
    t0 = time.time()
    v, f, keys = R.surface_nets(R.smooth(counts, 0), 1, lo, h)
    print('reference on 130^3: %.2f s, %d vertices' % (time.time() - t0, v.shape[0]))
    cells = keys // 16
    assert int(np.prod(dims - 1)) > 2 ** 21 and (cells < 2 ** 21).any() and (cells > 2 ** 21).any()


def test_gpu_tests_read_nothing_outside_the_repository():
    for name in ('test_hip_isosurface.py', 'test_hip_isosurface_edges.py', 'isosurface_ref.py'):
        src = open(os.path.join(ROOT, 'tests', name)).read()
        assert '/root/' + 'reference' not in src and 'oracle/' + '_ref' not in src and '_' + 'ref/' not in src, name
