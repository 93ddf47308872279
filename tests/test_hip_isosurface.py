"""Density isosurface on the device (csrc/nw_isosurface.hip) against its NumPy restatement (tests/isosurface_ref.py): the integer field and
the threshold bit for bit, the extracted mesh array for array (positions to a derived bound), run-to-run and thread-to-thread identity,
and the whole recipe -- cloud -> DensitySurface -> ShrinkwrapMembrane -- against the same fit started from the generator's surface."""
import threading

import numpy as np
import pytest

import isosurface_ref as R
from isosurface_ref import scene, reference, device_chain, position_bound, compare_mesh as _compare_mesh
from ch_shrinkwrap_amd import isosurface as I
from ch_shrinkwrap_amd import synth

pytestmark = pytest.mark.gpu

OFFSET = np.array([5e3, -3e3, 1e3], 'f4')                 # a cloud off the origin


def cloud(name):
    """(points, h, passes)"""
    if name == 'c1_translated':
        return scene('c1')[0] + OFFSET[None, :], 10.0, 2
    if name == 'one_voxel':                                # 2 x 10^5 localizations in one voxel: every atomic of a workgroup on one LDS slot
        pts = np.array([[35.0, 55.0, 55.0]]) + np.random.default_rng(3).uniform(-4.0, 4.0, size=(200000, 3))
        return pts.astype('f4'), 10.0, 4
    pts, _, h = scene(name)
    return pts, h, 2


@pytest.mark.parametrize('name', ['c1', 'c4', 'c1_translated', 'one_voxel'])
def test_field_and_threshold_are_bit_identical(name):
    pts, h, passes = cloud(name)
    lo, dims = I.grid_for(pts, h, passes + 3)
    ref_field, ref_counts = R.density(pts, lo, h, dims, passes)
    ctx = I.IsosurfaceContext()
    try:
        field, counts = ctx.density(pts, lo, h, dims, passes, return_field=True, return_counts=True)
        t = ctx.threshold_auto(0.3)
    finally:
        ctx.close()
    assert field.dtype == np.uint64 and counts.dtype == np.uint32
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(field, ref_field)
    if name == 'one_voxel':
        assert int(counts.max()) == 200000 and int((counts > 0).sum()) == 1
        assert int(field.max()) == 200000 * 70 ** 3 > 2 ** 32        # the centre weight of four rounds of [1 2 1] is C(8, 4) = 70 per axis
    thr, med, occ = R.threshold_auto(ref_field, ref_counts, 0.3)
    print(name, 'dims', dims, 'median', med, 'thr', thr, 'occupied', occ)
    assert (t['median'], t['thr'], t['n_occupied']) == (med, thr, occ)
    assert np.isclose(t['threshold_density'], thr / I.field_scale(h, passes), rtol=1e-12)


@pytest.mark.parametrize('name', ['c1', 'c4', 'c1_translated'])
def test_extraction_equals_the_reference(name):
    pts, h, passes = cloud(name)
    d = device_chain(pts, h, passes)
    if name in ('c1', 'c4'):
        rv, rf, rk, _ = reference(name)
    else:
        rv, rf, rk = R.surface_nets(d['field'], d['t']['thr'], d['lo'], h)
    _compare_mesh(name, d['v'], d['f'], d['k'], rv, rf, rk)
    assert (R.edge_use(d['f']) == 2).all()


def test_two_sheets_through_one_cell():
    """Two occupied voxels at opposite corners of one cell, no smoothing: the cell carries two vertices, the result is two closed blobs."""
    pts = np.concatenate([np.full((100, 3), 2.5, 'f4'), np.full((100, 3), 3.5, 'f4')])
    lo, dims = np.zeros(3, 'f4'), np.array([6, 6, 6], np.int32)
    ctx = I.IsosurfaceContext()
    try:
        field = ctx.density(pts, lo, 1.0, dims, 0, return_field=True)
        v, f, k = ctx.extract(50, return_keys=True)
        with pytest.raises(RuntimeError):
            ctx.extract(1000)                                                  # nothing above the threshold
    finally:
        ctx.close()
    ref_field = np.zeros((6, 6, 6), np.uint64)
    ref_field[2, 2, 2] = ref_field[3, 3, 3] = 100
    assert np.array_equal(field, ref_field)
    rv, rf, rk = R.surface_nets(ref_field, 50, lo, 1.0)
    _compare_mesh('two sheets', v, f, k, rv, rf, rk)
    comps = R.components(v, f)
    assert (R.edge_use(f) == 2).all() and len(comps) == 2 and all(c[1] == 2 and c[2] > 0 for c in comps)
    cell = ((2 * 5) + 2) * 5 + 2
    assert sorted(k[(k // 16) == cell] % 16) == [0, 3]


def test_errors_come_back_as_statuses():
    pts = scene('c1')[0]
    lo, dims = I.grid_for(pts, 10.0, 5)
    ctx = I.IsosurfaceContext()
    try:
        with pytest.raises(RuntimeError, match='out of order'):
            ctx.threshold_auto(0.3)
        with pytest.raises(RuntimeError, match='outside'):
            ctx.density(pts, lo, 10.0, dims - np.array([8, 0, 0], np.int32), 2)
        lo2, dims2 = I.grid_for(pts, 10.0, 2)
        ctx.density(pts, lo2, 10.0, dims2, 2)
        with pytest.raises(RuntimeError, match='border'):
            ctx.extract(0)                                                     # the smoothed field reaches the outermost layer of a grid padded by `passes`
        # a device pointer is checked by the counting kernel
        import torch
        bad = torch.from_numpy(pts.copy()).cuda()
        bad[17, 1] = float('nan')
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='non-finite'):
            ctx.density((bad.data_ptr(), bad.shape[0]), lo, 10.0, dims, 2)
        good = torch.from_numpy(pts.copy()).cuda()
        torch.cuda.synchronize()
        field = ctx.density((good.data_ptr(), good.shape[0]), lo, 10.0, dims, 2, return_field=True)
        assert np.array_equal(field, R.density(pts, lo, 10.0, dims, 2)[0])
    finally:
        ctx.close()


def test_two_runs_and_two_threads_give_the_same_arrays():
    pts, h, passes = cloud('c4')
    a = device_chain(pts, h, passes)
    b = device_chain(pts[::-1].copy(), h, passes)                              # the other order of arrival as well: integer sums
    out = [None, None]
    err = []

    def work(slot):
        try:
            out[slot] = device_chain(pts, h, passes)
        except Exception as e:                                                 # noqa: BLE001 (reported below)
            err.append(e)
    th = [threading.Thread(target=work, args=(s,)) for s in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for other in (b, out[0], out[1]):
        assert a['t'] == other['t']
        for key in ('field', 'counts', 'v', 'f', 'k'):
            assert np.array_equal(a[key], other[key]), key


def _closed_stats(v, f):
    comps = R.components(v, f)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    ue = np.unique(e, axis=0)
    mean_edge = float(np.linalg.norm(v[ue[:, 0]].astype('f8') - v[ue[:, 1]].astype('f8'), axis=1).mean())
    return bool((R.edge_use(f) == 2).all()), comps, mean_edge


def test_dust_goes_and_inner_sheets_go():
    """C1 plus a blob of 20 localizations far from the sphere: the raw isosurface has the outer sheet, the inverted inner sheet and the blob;
    start_surface keeps the outer sheet alone."""
    pts = scene('c1')[0].copy()
    pts[:20] = (np.array([[260.0, 0.0, 0.0]]) + np.random.default_rng(2).normal(scale=3.0, size=(20, 3))).astype('f4')
    v, f, info = I.density_isosurface(pts, voxel_size=10.0, threshold_fraction=0.3)
    raw = R.components(v, f)
    print('raw components (faces, chi, volume):', [(c[0].size, c[1], c[2]) for c in raw])
    assert len(raw) == 3 and sum(c[2] < 0 for c in raw) == 1
    s = I.start_surface(pts, voxel_size=10.0, remesh=False, min_component_faces=int(min(c[0].size for c in raw)) + 1)
    closed, comps, _ = _closed_stats(s.vertices, s.faces)
    assert closed and len(comps) == 1 and comps[0][1] == 2 and comps[0][2] > 0
    assert s.info['n_components'] == 3 and len(s.info['removed']) == 2
    d = synth.sdf_sphere(s.vertices.astype('f8'), 100.0)
    assert d.min() > 0 and d.max() <= 60.0


def test_recipe_from_the_cloud_alone():
    """C4 x 0.1: DensitySurface then ShrinkwrapMembrane (39 iterations, the module's defaults) against the same fit started from the
    generator's +20 nm surface, in the reference's metric.  Bound: no worse than 1.1 x (the start surface sits up to ~15 nm further out)."""
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    from ch_shrinkwrap_amd.evaluation import fit_quality
    cfg = synth.make_config('c4', scale=0.1)
    truth = synth.truth_cloud(cfg)
    p = cfg['points']
    table = {'x': p[:, 0], 'y': p[:, 1], 'z': p[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    ns = {'filtered_localizations': table}
    surf = I.DensitySurface(voxel_size=12.0).execute(ns)
    assert ns['surf'] is surf
    closed, comps, mean_edge = _closed_stats(surf.vertices, surf.faces)
    target = surf.info['target_edge_length']
    print('start surface: %d vertices, %d faces, chi %s, mean edge %.2f (target %.2f), removed %s' %
          (surf.vertices.shape[0], surf.faces.shape[0], [c[1] for c in comps], mean_edge, target, surf.info['removed']))
    assert closed and len(comps) == 1 and comps[0][1] == -2 and comps[0][2] > 0
    assert abs(mean_edge - target) < 0.15 * target
    mesh = ShrinkwrapMembrane().execute(ns)
    closed, comps, _ = _closed_stats(np.asarray(mesh.vertices), np.asarray(mesh.faces))
    q = fit_quality(mesh, truth)

    class Surf(object):
        vertices, faces = cfg['vertices'], cfg['faces']
    base = ShrinkwrapMembrane().execute({'surf': Surf, 'filtered_localizations': table})
    q0 = fit_quality(base, truth)
    print('mse_rms from the cloud %.3f nm, from the generator\'s surface %.3f nm, ratio %.3f' % (q['mse_rms'], q0['mse_rms'], q['mse_rms'] / q0['mse_rms']))
    assert closed and len(comps) == 1 and comps[0][1] == -2
    assert q['mse_rms'] <= 1.1 * q0['mse_rms']
