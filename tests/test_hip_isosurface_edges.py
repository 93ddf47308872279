"""The density isosurface kernels (csrc/nw_isosurface.hip) at their edges, each case against the NumPy restatement (tests/isosurface_ref.py):
counts, field, median, threshold, occupied count, vertex keys and faces bit for bit, positions to 8 float32 ulp of the largest coordinate.
The inputs are built in isosurface_ref.py, and tests/test_isosurface.py checks on the reference alone that each one reaches what it is
named for.

    noise blocks        all 256 corner patterns, cells with two, three and four sheets, nodes equal to the threshold, both parities
    border grids        values in the outermost layer of 3 x 3 x 3 and of thin grids: the truncation branches of k_iso_smooth
    table cases         voxels that must overflow the LDS table of k_iso_count, and wrap it; point counts around its block sizes
    face points         points on voxel faces and one ulp beside them, host and device path; the first voxel outside is refused
    select cases        the radix select of nwi_threshold_auto: ties, even counts, a byte of 0xFF, a prefix over three bytes
    big field           extraction where field and threshold are above 2^32
    reuse, carry        one context over grids of different sizes; a grid whose cells pass the first carry of the scan's tile sums

One branch stays unreached: `shift >= 56` in k_iso_hist and the select starting there need field values of 2^56, i.e. 2^26 localizations
at five passes; no cloud of that size is built here.
"""
import functools

import numpy as np
import pytest

import isosurface_ref as R
from isosurface_ref import device_chain, compare_mesh
from ch_shrinkwrap_amd import isosurface as I

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    c = I.IsosurfaceContext()
    yield c
    c.close()


def on_device(pts):
    """(the tensor that owns the memory, (pointer, n) for IsosurfaceContext.density)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
    torch.cuda.synchronize()
    return t, (t.data_ptr(), t.shape[0])


def check_density(ctx, pts, lo, h, dims, passes, counts=None, device_path=False):
    """density on the device against the reference, bit for bit; returns the reference's (field, counts)"""
    ref_field, ref_counts = R.density(pts, lo, h, dims, passes)
    if counts is not None:
        assert np.array_equal(ref_counts, counts)
    keep, src = on_device(pts) if device_path else (None, pts)
    field, cnt = ctx.density(src, lo, h, dims, passes, return_field=True, return_counts=True)
    del keep
    assert field.dtype == np.uint64 and cnt.dtype == np.uint32
    assert np.array_equal(cnt, ref_counts)
    assert np.array_equal(field, ref_field)
    return ref_field, ref_counts


def check_threshold(ctx, ref_field, ref_counts, fraction):
    thr, med, occ = R.threshold_auto(ref_field, ref_counts, fraction)
    t = ctx.threshold_auto(fraction)
    assert (t['median'], t['thr'], t['n_occupied']) == (med, thr, occ)
    return thr


def check_extract(name, ctx, ref_field, thr, lo, h):
    """extract against the reference: the same mesh, or the status that answers the reference's refusal.  Returns the device mesh or None."""
    try:
        rv, rf, rk = R.surface_nets(ref_field, thr, lo, h)
    except ValueError as e:
        with pytest.raises(RuntimeError, match='border' if 'outermost' in str(e) else 'nothing above'):
            ctx.extract(thr)
        return None
    v, f, k = ctx.extract(thr, return_keys=True)
    compare_mesh(name, v, f, k, rv, rf, rk)
    return v, f, k


def closed_and_oriented(f):
    return bool((R.edge_use(f) % 2 == 0).all()) and R.directed_edges_balanced(f)


# ---- 1. every pattern -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise_reference(seed, shifted):
    pts, lo, h, dims, counts = R.noise_case(seed, shifted)
    return R.surface_nets(R.smooth(counts, 0), 1, lo, h)


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_noise_block_reaches_every_pattern(seed, shifted, ctx):
    """passes = 0, thr = 1 on counts uniform in 0..3: the rank lookup of k_iso_quads, the per-sheet sums of k_iso_vertices and vcnt of
    k_iso_cell_counts on all 256 patterns; the strict `>` and crossings at t = 0 on the nodes equal to thr.  shifted: the grid starts one
    voxel earlier along x, which takes every quad through the other branch of the parity split."""
    pts, lo, h, dims, counts = R.noise_case(seed, shifted)
    ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, 0, counts)
    check_threshold(ctx, ref_field, ref_counts, 0.3)
    patterns, sheets = R.sheet_census(ref_field, 1)
    assert patterns == set(range(256)) and (sheets[2:] >= 1).all()
    rv, rf, rk = noise_reference(seed, shifted)
    v, f, k = ctx.extract(1, return_keys=True)
    compare_mesh('noise %d%s' % (seed, ' shifted' if shifted else ''), v, f, k, rv, rf, rk)
    # closed and oriented on both sides; an edge is used four times where two cells share an ambiguous face (README), so not manifold
    assert closed_and_oriented(rf) and closed_and_oriented(f)


# ---- 2. the grid's border -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('passes', [0, 1, I.MAX_PASSES])
@pytest.mark.parametrize('name', sorted(R.BORDER_GRIDS))
def test_values_on_the_border_are_truncated_not_wrapped(name, passes, ctx):
    pts, lo, h, dims, counts = R.border_case(name)
    ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, passes, counts)
    mass = pts.shape[0] * 4 ** (3 * passes)
    total = int(ref_field.sum())
    print(name, 'passes', passes, 'sum of the field', total, 'of', mass)
    assert total == mass if passes == 0 else total < mass                      # mass left the grid
    if name == '3x3x3' and passes == 5:
        assert (total, mass) == (1023641088, 11811160064)
    thr = check_threshold(ctx, ref_field, ref_counts, 0.3)
    with pytest.raises(RuntimeError, match='border'):
        ctx.extract(0)
    check_extract(name, ctx, ref_field, thr, lo, h)
    # the context still answers
    pts, lo, h, dims, counts = R.noise_case(0)
    check_density(ctx, pts, lo, h, dims, 1, counts)


# ---- 3. the counting kernel's table and block edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('device_path', [False, True])
@pytest.mark.parametrize('slots,per_slot', [((1000,), 8), ((2047,), 8), ((2045, 2046, 2047), 3)])
def test_voxels_that_overflow_the_table(slots, per_slot, device_path, ctx):
    """More voxels in one workgroup than the table slots they can reach: at least one goes to the direct global atomic, whatever the
    order of arrival.  Home slots 2045..2047 probe on into slots 0..2."""
    pts, lo, h, dims, vox = R.hash_case(slots, per_slot)
    assert R.table_must_overflow(vox) and pts.shape[0] <= 1024
    assert sorted(set(R.home_slot(vox).tolist())) == list(slots)
    _, ref_counts = check_density(ctx, pts, lo, h, dims, 0, device_path=device_path)
    assert ref_counts.ravel()[vox].tolist() == [100] * vox.size


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_point_counts_around_the_block_sizes(n, ctx):
    pts, lo, h, dims = R.spread_points(n)
    _, ref_counts = check_density(ctx, pts, lo, h, dims, 0)
    assert int(ref_counts.sum()) == n


# ---- 4. voxel assignment in float32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [0.1, 7.3, 12.0])
@pytest.mark.parametrize('lo', [(0.0, 0.0, 0.0), (5e3, -3e3, 1e3)])
def test_points_on_voxel_faces(h, lo, ctx):
    """Points at lo + k h and one float32 ulp to either side.  The reference says which fall outside (tests/test_isosurface.py: fewer
    than 5 %); the others are counted as the reference counts them, on both input paths, and the full set is refused on both."""
    lo = np.array(lo, np.float32)
    dims = np.array([40, 40, 40], np.int32)
    pts = R.face_points(lo, h, 40)
    keep = R.inside_grid(pts, lo, h, dims)
    assert keep.mean() > 0.95
    for device_path in (False, True):
        check_density(ctx, pts[keep], lo, h, dims, 0, device_path=device_path)
        if not keep.all():
            t, src = on_device(pts) if device_path else (None, pts)
            with pytest.raises(RuntimeError, match='outside'):
                ctx.density(src, lo, h, dims, 0)


@pytest.mark.parametrize('device_path', [False, True])
def test_first_voxel_outside_is_refused_last_inside_accepted(device_path, ctx):
    dims = np.array([40, 23, 11], np.int32)
    good, good_lo, good_h, good_dims, good_counts = R.noise_case(1)
    for h in (0.1, 7.3, 12.0):
        for lo in ((0.0, 0.0, 0.0), (5e3, -3e3, 1e3)):
            lo = np.array(lo, np.float32)
            inside = np.zeros((0, 3), np.float32)
            for axis in range(3):
                p, coord = R.boundary_point(lo, h, dims, axis, int(dims[axis]) - 1)
                assert coord == dims[axis] - 1
                inside = np.concatenate([inside, p])
            base = np.concatenate([inside, R.boundary_point(lo, h, dims, 0, 0)[0]])
            check_density(ctx, base, lo, h, dims, 0, device_path=device_path)
            for axis in range(3):
                for edge in (int(dims[axis]), -1):
                    p, coord = R.boundary_point(lo, h, dims, axis, edge)
                    assert coord == edge
                    bad = np.concatenate([base, p, base])
                    with pytest.raises(ValueError, match='outside'):
                        R.count(bad, lo, h, dims)
                    t, src = on_device(bad) if device_path else (None, bad)
                    with pytest.raises(RuntimeError, match='outside'):
                        ctx.density(src, lo, h, dims, 0)
                    del t
    if device_path:
        # the counting kernel had begun: the context holds no field now
        with pytest.raises(RuntimeError, match='out of order'):
            ctx.threshold_auto(0.3)
    check_density(ctx, good, good_lo, good_h, good_dims, 2, good_counts, device_path=device_path)
    fresh = I.IsosurfaceContext()
    try:
        p, _ = R.boundary_point(good_lo, good_h, good_dims, 1, -1)
        t, src = on_device(p) if device_path else (None, p)
        with pytest.raises(RuntimeError, match='outside'):
            fresh.density(src, good_lo, good_h, good_dims, 0)
        with pytest.raises(RuntimeError, match='out of order'):
            fresh.threshold_auto(0.3)
        with pytest.raises(RuntimeError, match='out of order'):
            fresh.extract(1)
        check_density(fresh, good, good_lo, good_h, good_dims, 0, good_counts)
    finally:
        fresh.close()


# ---- 5. the radix select ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.SELECT_VALUES))
def test_median_select(name, ctx):
    """passes = 0: the field values are the counts, so each case is exact by construction."""
    pts, lo, h, dims, counts = R.select_case(name)
    ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, 0, counts)
    for fraction in (0.3, 1.0, 0.0):
        thr = check_threshold(ctx, ref_field, ref_counts, fraction)
        if fraction == 0.0:
            assert thr == 0
        if fraction == 1.0:
            assert thr == ctx.threshold_auto(1.0)['median']
    with pytest.raises(RuntimeError, match='bad argument'):
        ctx.threshold_auto(1e30)
    check_threshold(ctx, ref_field, ref_counts, 0.5)                           # (and the refusal left the context as it was)


def test_median_is_over_the_occupied_voxels_only(ctx):
    pts, lo, h, dims, counts = R.excluded_case()
    ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, 2, counts)
    assert ref_field[ref_counts == 0].max() > ref_field[ref_counts > 0].min()
    for fraction in (0.3, 1.0):
        check_threshold(ctx, ref_field, ref_counts, fraction)
    assert ctx.threshold_auto(1.0)['n_occupied'] == 3


# ---- 6. fields above 2^32 -----------------------------------------------------------------------------------------------------------------
def test_extraction_from_a_field_above_32_bits(ctx):
    """(float)(long long)(f0 - thr) in k_iso_vertices goes through a wrapped unsigned difference wherever f0 < thr: here with f0, thr and
    their difference all beyond 32 bits."""
    pts, lo, h, dims, counts = R.big_field_case()
    ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, 5, counts)
    assert int(ref_field.max()) > 2 ** 32
    peaks = sorted(int(x) for x in ref_field[ref_counts > 0])
    thr = check_threshold(ctx, ref_field, ref_counts, 0.3)
    assert thr > 2 ** 32
    for name, t in (('auto', thr), ('between the peaks', (peaks[0] + peaks[1]) // 2)):
        v, f, k = check_extract('big field, thr ' + name, ctx, ref_field, t, lo, h)
        assert (R.edge_use(f) == 2).all()                                      # a smooth field: manifold
    assert len(R.components(v, f)) == 1                                        # the larger blob alone


# ---- 7. reuse, and the scan's first carry -------------------------------------------------------------------------------------------------
def _chain(case, passes, thr, ctx=None):
    pts, lo, h, dims = case[:4]
    return device_chain(pts, h, passes, ctx=ctx, grid=(lo, dims), thr=thr)


def _same(a, b):
    assert a['t'] == b['t']
    for key in ('field', 'counts', 'v', 'f', 'k'):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key


def test_one_context_over_grids_of_different_sizes(ctx):
    """ensure() keeps the larger buffers: a smaller grid after a larger one must not see its tails.  Each result equals a fresh
    context's, and the first the reference's."""
    c1 = R.scene('c1')
    steps = [('noise', lambda c: _chain(R.noise_case(0), 0, 1, c)),
             ('3x3x3', None),
             ('c1', lambda c: device_chain(c1[0], c1[2], 2, ctx=c)),
             ('noise', lambda c: _chain(R.noise_case(0), 0, 1, c))]
    fresh = {}
    for name, run in steps:
        if run is None:
            pts, lo, h, dims, counts = R.border_case(name)
            ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, 1, counts)
            check_threshold(ctx, ref_field, ref_counts, 0.3)
            with pytest.raises(RuntimeError, match='border'):
                ctx.extract(0)
            continue
        if name not in fresh:
            fresh[name] = run(None)
        _same(run(ctx), fresh[name])
    rv, rf, rk = noise_reference(0, False)
    compare_mesh('noise, fresh context', fresh['noise']['v'], fresh['noise']['f'], fresh['noise']['k'], rv, rf, rk)
    rv, rf, rk, _ = R.reference('c1')
    compare_mesh('c1, fresh context', fresh['c1']['v'], fresh['c1']['f'], fresh['c1']['k'], rv, rf, rk)


def test_two_extractions_of_one_density(ctx):
    pts, lo, h, dims, counts = R.big_field_case()
    ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, 3, counts)
    peaks = sorted(int(x) for x in ref_field[ref_counts > 0])
    big = check_extract('low threshold', ctx, ref_field, peaks[0] // 50, lo, h)
    small = check_extract('high threshold', ctx, ref_field, (peaks[0] + peaks[1]) // 2, lo, h)
    assert small[0].shape[0] < big[0].shape[0]
    again = check_extract('low threshold again', ctx, ref_field, peaks[0] // 50, lo, h)
    for a, b in zip(big, again):
        assert np.array_equal(a, b)


def test_cells_past_the_first_carry_of_the_scan(ctx):
    """130^3 nodes, 129^3 = 2 146 689 cells: the scan of the active flags carries over its tile sums once.  One noise block has cell
    indices below 2^21, the other above.  The whole mesh is compared (the reference takes about a second here)."""
    pts, lo, h, dims, counts = R.carry_case()
    ref_field, ref_counts = check_density(ctx, pts, lo, h, dims, 0, counts)
    check_threshold(ctx, ref_field, ref_counts, 0.3)
    v, f, k = check_extract('130^3', ctx, ref_field, 1, lo, h)
    assert (k // 16 < 2 ** 21).any() and (k // 16 > 2 ** 21).any()
    assert closed_and_oriented(f)
