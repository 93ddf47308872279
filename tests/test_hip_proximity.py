"""The mesh-to-mesh distance on the device (csrc/nw_proximity.hip) against its NumPy restatement (tests/mesh_proximity_ref.py, brute force
over all pairs of faces): distance, partner, kind and closest points bit for bit and the band's counters exactly -- the equalities the
compiled core owes it in tests/test_proximity_core_cpu.py -- on face counts around the wave and the block, bands at and one ulp below a
gap, crossing, mis-shaped, flat and far-away meshes, through one context; then against the distance unit, which knows nothing of it;
both directions against each other; and the Python surface on top.  Every mesh is at most icosphere(2)-sized."""
import functools

import numpy as np
import pytest

import mesh_proximity_ref as P
from ch_shrinkwrap_amd import proximity as C
from ch_shrinkwrap_amd.distance import distance_to_mesh
from ch_shrinkwrap_amd.trimesh import TriMesh

pytestmark = pytest.mark.gpu

ULP_BELOW_3 = float(np.nextafter(3.0, 0.0))


@pytest.fixture(scope='module')
def ctx():
    c = C.ProximityContext()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def scene(name):
    """(va, fa, vb, fb) by name"""
    if name.startswith('counts '):                                # 'counts <faces of A> <faces of B>': the first faces of two spheres
        na, nb = (int(t) for t in name.split()[1:])
        va, fa, vb, fb = P.two_spheres()
        return va, fa[:na].copy(), vb, fb[:nb].copy()
    if name == 'spheres':
        return P.two_spheres()
    if name == 'crossing':
        return P.crossing_spheres()
    if name == 'cubes':
        return P.two_cubes(3.0)[:4]
    if name == 'far':
        return P.nested_spheres()
    if name == 'oversize a':
        va, fa, vb, fb = P.two_spheres()
        return P.with_oversize_face(va, fa) + (vb, fb)
    if name == 'oversize b':
        va, fa, vb, fb = P.two_spheres()
        return (va, fa) + P.with_oversize_face(vb, fb)
    if name == 'flat':
        va, fa, vb, fb = P.two_spheres()
        return P.with_flat_faces(va, fa) + P.with_flat_faces(vb, fb)
    if name == 'million':
        va, fa, vb, fb = P.two_spheres()
        return (va + np.float32(1e6)).astype(np.float32), fa, (vb + np.float32(1e6)).astype(np.float32), fb
    if name == 'copies':
        return P.soup([P.FLOOR]) + P.soup([[[0, 0, 2], [4, 0, 2], [0, 4, 2]]] * 300)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def nearest(name):
    return P.nearest(*scene(name))                                # all pairs, once a scene


@functools.lru_cache(maxsize=None)
def reference(name, band):
    return P.with_band(nearest(name), band)


def device(ctx, name, band, cell_size=0.0):
    va, fa, vb, fb = scene(name)
    ctx.set_mesh(vb, fb, cell_size=cell_size)
    r = ctx.query(va, fa, band=band, return_closest=True)
    assert r['distance'].shape == (len(fa),) and r['closest_a'].shape == r['closest_b'].shape == (len(fa), 3)
    return r


def check(ctx, name, band, cell_size=0.0):
    ref, dev = reference(name, band), device(ctx, name, band, cell_size)
    P.same_as_restatement(dev, ref)
    info = dev['info']
    assert (info['in_band'], info['at_zero'], info['faces']) == (ref['n_in_band'], ref['n_zero'], len(ref['d2']))
    assert info['tests'] >= info['in_band'] and info['centroids'] >= info['tests'] and info['rings'] >= 0 and info['cells'] >= 1
    return dev, ref


# ---- parity and exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('na', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('nb', [1, 2, 320])
def test_face_counts_around_the_wave_and_the_block(ctx, na, nb):
    for band in (np.inf, 30.0):
        dev, ref = check(ctx, 'counts %d %d' % (na, nb), band)
    assert (ref['partner'] < nb).all()


@pytest.mark.parametrize('band', [np.inf, 30.0, 3.0, ULP_BELOW_3])
def test_bands_at_the_gap_and_one_ulp_below(ctx, band):
    dev, ref = check(ctx, 'cubes', band)
    va, fa = scene('cubes')[:2]
    touching = (va[fa][:, :, 0] == 4).any(1)
    if band == ULP_BELOW_3:
        assert dev['info']['in_band'] == 0 and (dev['partner'] == -1).all() and np.isinf(dev['distance']).all() and np.isnan(dev['closest_b']).all()
    else:
        assert (dev['distance'][touching] == 3.0).all() and (dev['partner'][touching] >= 0).all()
    if band == 3.0:
        assert np.array_equal(dev['partner'] >= 0, touching)


def test_a_mesh_wholly_out_of_band_ends_every_walk_at_its_ring_bound(ctx):
    """The device returns the rings summed over the faces, so what is asserted here is the sum: at least five rings a face and at most the
    sum of the per-face bounds.  One over-long walk could hide in that sum; that every single face keeps its own bound is asserted
    where the rings come back per face, on the same core header and the same scene, in tests/test_proximity_core_cpu.py."""
    dev, ref = check(ctx, 'far', 30.0, cell_size=10.0)
    va, fa, vb, fb = scene('far')
    info = dev['info']
    assert info['cell_size'] == 10.0                                                       # (the grid of 320 centroids needs no widening)
    assert info['in_band'] == 0 and info['tests'] == 0 and (dev['partner'] == -1).all() and (dev['kind'] == -1).all()
    # ceil((d_cap + rho_f + rho_max) / h) + 1 rings a face at the most, with the radii a hair enlarged
    bound = np.ceil((30.0 + (P.face_rho(va, fa) + P.face_rho(vb, fb).max()) * (1 + 1e-9)) / 10.0) + 1
    assert 5 * info['faces'] <= info['rings'] <= int(bound.sum()) and bound.max() < 9        # no walk crosses the grid's 19 or more cells an axis
    assert info['cells'] >= 19 ** 3


@pytest.mark.parametrize('name', ['spheres', 'crossing', 'oversize a', 'oversize b', 'flat', 'million', 'copies'])
def test_scenes_equal_the_restatement(ctx, name):
    for band in (np.inf, 30.0):
        dev, ref = check(ctx, name, band)
    if name == 'crossing':
        assert dev['info']['at_zero'] > 20 and (dev['kind'][dev['distance'] == 0] == 0).all()
        assert np.array_equal(dev['closest_a'][dev['kind'] == 0], dev['closest_b'][dev['kind'] == 0])
    if name == 'oversize b':
        assert (dev['partner'] == len(scene(name)[3]) - 1).sum() > 3
    if name == 'copies':
        assert dev['partner'][0] == 0 and dev['distance'][0] == 2.0                       # the smallest id of 300 equally near faces
    if name in ('spheres', 'million'):
        assert 0 < dev['info']['in_band'] < dev['info']['faces']


def test_cell_sizes_one_context_and_two_runs_give_the_same_bytes(ctx):
    auto = device(ctx, 'crossing', 30.0)
    keys = ('distance', 'partner', 'kind', 'closest_a', 'closest_b')
    cells = {auto['info']['cells']}
    for cell_size in (4.0, 17.0, 250.0):
        other = device(ctx, 'crossing', 30.0, cell_size)
        cells.add(other['info']['cells'])
        for k in keys:
            assert auto[k].tobytes() == other[k].tobytes()
        assert (other['info']['in_band'], other['info']['at_zero']) == (auto['info']['in_band'], auto['info']['at_zero'])
    assert len(cells) >= 3                                                                 # the grids did differ
    again = device(ctx, 'crossing', 30.0)
    for k in keys:
        assert auto[k].tobytes() == again[k].tobytes()
    # (the centroids were binned anew: within a cell their order is the shared grid's scatter's, which is not fixed, and how many exact
    # tests the bounds spare depends on it -- nothing else does)
    assert {k: v for k, v in auto['info'].items() if k != 'tests'} == {k: v for k, v in again['info'].items() if k != 'tests'}
    va, fa, vb, fb = scene('crossing')
    twice = ctx.query(va, fa, band=30.0, return_closest=True)                              # the grid at hand: every counter again
    for k in keys:
        assert again[k].tobytes() == twice[k].tobytes()
    assert again['info'] == twice['info']
    # a band that asks for another cell size bins the centroids again, in the same context, and the next one binds them back
    wide = device(ctx, 'crossing', np.inf)
    P.same_as_restatement(wide, reference('crossing', np.inf))
    P.same_as_restatement(device(ctx, 'crossing', 30.0), reference('crossing', 30.0))


# ---- against the distance unit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['spheres', 'crossing', 'oversize b'])
def test_against_the_point_to_mesh_distance_of_the_corners(ctx, name):
    """Each corner A_k of a face is a candidate against every face g of B (kinds 1-3), so the face's d2 is at most
    min over g of nwd_point_triangle(A_k, g), which is the squared distance nwd_query gives for the vertex A_k: distance <= the smallest
    of the three corners' values (0 <= everything for a pierced pair).  Where the kind is 1-3 the face's d2 IS
    nwd_point_triangle(A_k, partner), one of the values that minimum runs over, so it is at least the vertex's d2 as well: the two are
    equal, and both sides return the correctly rounded sqrt of the same double."""
    va, fa, vb, fb = scene(name)
    dev = device(ctx, name, np.inf)
    dv = distance_to_mesh(va.astype(np.float64), (vb, fb), signed=False)
    corners = dv[fa]                                                                       # (F, 3)
    assert (dev['distance'] <= corners.min(1)).all()
    by_corner = (dev['kind'] >= 1) & (dev['kind'] <= 3)
    assert by_corner.sum() > 10
    mine = corners[np.flatnonzero(by_corner), dev['kind'][by_corner] - 1]
    assert np.array_equal(P.bits(dev['distance'][by_corner]), P.bits(mine))
    assert (dev['distance'] < corners.min(1)).sum() > 10                                   # the faces the vertices overestimate


@pytest.mark.parametrize('name', ['spheres', 'cubes', 'million', 'oversize a'])
def test_both_directions_find_the_same_smallest_gap(ctx, name):
    """The global minimum is one pair of points; the two calls reach it through candidates whose roles swap, and whose interior points
    p + s u round at the size of the coordinates: 64 ulp of the largest coordinate magnitude, not a measured number."""
    va, fa, vb, fb = scene(name)
    ab = device(ctx, name, np.inf)['distance'].min()
    ctx.set_mesh(va, fa)
    ba = ctx.query(vb, fb)['distance'].min()
    assert abs(ab - ba) <= 64 * np.spacing(float(max(np.abs(va).max(), np.abs(vb).max())))


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contact_reference():
    va, fa, vb, fb = scene('spheres')
    return P.contact_side(va, fa, vb, fb, 30.0), P.contact_side(vb, fb, va, fa, 30.0)


def test_contact_sites_of_the_two_spheres():
    from ch_shrinkwrap_amd.distance import mesh_twins
    from ch_shrinkwrap_amd.surgery import SurgeryContext
    va, fa, vb, fb = scene('spheres')
    c = C.contact_sites(TriMesh(va, fa), (vb, fb), 30.0)
    sctx = SurgeryContext()
    try:
        for tag, ref, (v, f) in zip('ab', contact_reference(), ((va, fa), (vb, fb))):
            assert np.array_equal(c['faces_' + tag], ref['faces']) and np.array_equal(c['patches_' + tag], ref['patches'])
            assert np.array_equal(c['patch_faces_' + tag], ref['patch_faces']) and c['n_crossing_' + tag] == ref['n_crossing'] == 0
            assert np.array_equal(P.bits(c['patch_min_distance_' + tag]), P.bits(ref['patch_min_distance']))
            tw = mesh_twins(f, len(v))
            st = sctx.component_stats(v, f, tw, ref['patches'], len(ref['patch_area']))   # the areas as nws_component_stats gives them for that mask
            assert np.array_equal(P.bits(c['patch_area_' + tag]), P.bits(st['area'])) and c['area_' + tag] == float(st['area'].sum())
            assert c['area_' + tag] == pytest.approx(ref['area'], rel=1e-9)
            P.same_as_restatement(c['result_' + tag], ref['result'])
    finally:
        sctx.close()
    assert len(c['patch_area_a']) == 1 and 0 < c['faces_a'].sum() < len(fa)
    r = TriMesh(va, fa).distance_to_mesh_of(TriMesh(vb, fb), band=30.0, return_closest=True)
    P.same_as_restatement(r, reference('spheres', 30.0))


def test_membrane_contacts_emits_the_rows_of_that_scene():
    va, fa, vb, fb = scene('spheres')
    ref = contact_reference()[0]
    ns = {'membrane': TriMesh(va, fa), 'membrane2': TriMesh(vb, fb)}
    t = C.MembraneContacts(contact_distance=30.0).execute(ns)
    assert ns['contacts'] is t
    rows = np.flatnonzero(ref['faces'])
    r = ref['result']
    assert np.array_equal(P.bits(np.stack([t['x'], t['y'], t['z']], 1)), P.bits(r['closest_a'][rows]))
    assert np.array_equal(P.bits(t['distance']), P.bits(r['distance'][rows])) and np.array_equal(t['partner'], r['partner'][rows])
    assert np.array_equal(t['patch'], ref['patches'][rows]) and (t['patch'] == 0).all()
    md = t['metadata']
    assert md['area_a'] == pytest.approx(ref['area'], rel=1e-9) and md['area_b'] == pytest.approx(contact_reference()[1]['area'], rel=1e-9)
    assert md['contact_distance'] == 30.0 and md['n_crossing_a'] == 0
