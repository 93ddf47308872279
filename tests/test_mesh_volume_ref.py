"""
CPU test: the NumPy restatement of the banded signed-distance volume (tests/mesh_volume_ref.py) against ground truth that does not
come from it -- a box's closed-form distance on a lattice of integer nodes, lattices wholly inside and wholly outside a cube, a lattice
that cuts an L-shaped prism, nested shells -- the premise of the sweep (why d_cap < h is refused), the sign margins of every input
the other tests use, and three mutations that each turn an assertion red.
"""
import numpy as np
import pytest

import mesh_distance_ref as D
import mesh_volume_ref as V


def cube_checks(mutate=None):
    """the [0, 4]^3 cube on the 9 x 9 x 9 lattice of integer nodes, as a list of booleans by name"""
    v, f = V.cube4()
    lo, h, dims = V.CUBE_LATTICE
    p = V.nodes(lo, h, dims)
    assert np.array_equal(p, np.round(p)) and p.min() == -2 and p.max() == 6
    want = V.cube4_sdf(p)
    out = {}
    for d_cap in (1.0, 2.0, 2.5):
        r = V.volume(v, f, lo, h, dims, d_cap, mutate=mutate)
        near = np.abs(want) <= d_cap
        tag = 'cap%g_' % d_cap
        out[tag + 'band'] = bool(np.array_equal(r['in_band'], near) and np.array_equal(r['face'] >= 0, near))
        out[tag + 'exact'] = bool(np.abs(r['sd'][near] - want[near]).max() == 0.0)
        out[tag + 'clamped'] = bool(np.array_equal(r['sd'][~near], np.where(want[~near] < 0, -d_cap, d_cap)))
        out[tag + 'mask'] = bool(np.array_equal(r['mask'], want < 0))
        out[tag + 'field'] = bool(np.array_equal(r['field'], np.floor((d_cap - np.clip(want, -d_cap, d_cap)) * 2.0 ** 20).astype(np.uint64)))
    # a node at distance exactly 2: in band with d_cap = 2, out of it one ulp below
    at2 = np.flatnonzero(want == 2.0)
    assert at2.size > 0
    out['exactly_at_cap'] = bool((V.volume(v, f, lo, h, dims, 2.0, mutate=mutate)['face'][at2] >= 0).all())
    out['one_ulp_below'] = bool((V.volume(v, f, lo, h, dims, np.nextafter(2.0, 0.0), mutate=mutate)['face'][at2] == -1).all())
    return out


def position_checks(mutate=None):
    """lattices inside, outside and across a mesh"""
    v, f = D.cube()
    v = (v * 50.0).astype(np.float32)                                                      # side 100
    out = {}
    r = V.volume(v, f, [-10.5, -10.5, -10.5], 4.0, (5, 5, 5), 8.0, mutate=mutate)          # nodes within +-8 of the centre: 42 from a face
    out['inside'] = bool((r['sd'] == -8.0).all() and (r['face'] == -1).all() and r['mask'].all() and (r['field'] == 16 << 20).all())
    r = V.volume(v, f, [100.0, 90.0, -200.0], 4.0, (5, 5, 5), 8.0, mutate=mutate)
    out['outside'] = bool((r['sd'] == 8.0).all() and (r['face'] == -1).all() and not r['mask'].any() and (r['field'] == 0).all())
    # rows that start inside the L-shaped prism and end outside it, and the other way round
    v, f = D.l_prism()
    lo, h, dims = [0.3 - 0.125, 0.2 - 0.125, 0.1 - 0.125], 0.25, (12, 11, 6)
    r = V.volume(v, f, lo, h, dims, 0.25, mutate=mutate)
    inside = D.l_prism_inside(r['nodes'])
    assert inside[0] and not inside[-1] and 0.2 < inside.mean() < 0.8 and (~r['in_band']).sum() > 100
    out['cutting_mask'] = bool(np.array_equal(r['mask'], inside))
    out['cutting_far'] = bool(np.array_equal(r['sd'][~r['in_band']], np.where(inside[~r['in_band']], -0.25, 0.25)))
    return out


def test_the_cube_on_integer_nodes():
    c = cube_checks()
    assert all(c.values()), c


def test_lattices_inside_outside_and_across():
    c = position_checks()
    assert all(c.values()), c


def test_the_cutting_lattice_equals_the_box_distance():
    v, f = V.cube4()
    lo, h, dims = [1.0 - 0.375, 0.5 - 0.375, -1.0 - 0.375], 0.75, (9, 4, 8)                  # starts inside along x, outside along z
    r = V.volume(v, f, lo, h, dims, 0.75)
    want = V.cube4_sdf(r['nodes'])
    near = r['in_band']
    assert np.abs(r['sd'][near] - want[near]).max() < 1e-15 and np.array_equal(near, np.abs(want) <= 0.75)
    assert np.array_equal(r['mask'], want < 0) and (r['mask'].reshape(8, 4, 9)[:, :, 0].any())


def test_nested_shells_alternate_along_a_row():
    v, f = V.nested_shells()
    lo, h, dims = [-13.5, -1.6, -1.4], 1.0, (27, 3, 3)
    r = V.volume(v, f, lo, h, dims, 1.0)
    assert V.margins_clear(r)
    row = r['nodes'].reshape(3, 3, 27, 3)[1, 1]
    rad = np.linalg.norm(row, axis=1)
    clear = (np.abs(rad - 10.0) > 0.4) & (np.abs(rad - 5.0) > 0.4)                           # (the polyhedra lie a little inside the spheres)
    want = (rad < 10.0) & (rad > 5.0)
    got = r['mask'].reshape(3, 3, 27)[1, 1]
    assert np.array_equal(got[clear], want[clear])
    runs = got[clear][np.r_[True, np.diff(got[clear].astype(int)) != 0]]
    assert runs.tolist() == [False, True, False, True, False]


def test_the_premise_a_band_below_h_steps_over_a_thin_slab():
    """a slab thinner than h between two rows of nodes: with d_cap = 0.4 h no node is in band and the far side keeps the seed's sign"""
    v, f = D.cube()
    v = (v * np.array([50.0, 50.0, 0.05])).astype(np.float32)                                # |z| <= 0.05
    lo, h, dims = [-2.0, -2.0, -2.0], 1.0, (4, 4, 4)                                         # nodes at z = -1.5 .. 1.5
    with pytest.raises(ValueError):
        V.volume(v, f, lo, h, dims, 0.4)
    r = V.volume(v, f, lo, h, dims, 0.4, check_cap=False)
    assert not r['in_band'].any() and not r['mask'].any()                                    # right, but only because no node is inside
    v2 = (v + np.array([0.0, 0.0, 0.5], np.float32)).astype(np.float32)                      # the slab now holds the nodes at z = 0.5
    r = V.volume(v2, f, lo, h, dims, 0.4, check_cap=False)
    inside = np.abs(r['nodes'][:, 2] - 0.5) < 0.05
    assert inside.sum() == 16 and r['in_band'][inside].all() and r['mask'][inside].all()
    above = r['nodes'][:, 2] > 1.0
    # the z-line steps from the in-band inside node (0, 0, 2) to (0, 0, 3) beyond the slab: out of band, it inherits 'inside'
    assert r['mask'][above].any()
    ok = V.volume(v2, f, lo, h, dims, 1.0)                                                   # with d_cap = h the same lattice is right
    assert np.array_equal(ok['mask'], inside)


def every_input():
    """(name, vertices, faces, lo, h, dims, d_cap) of every signed input the tests of the core and of the device use"""
    from ch_shrinkwrap_amd.trimesh import icosphere
    out = []
    v, f = V.cube4()
    for d_cap in (1.0, 2.0, 2.5):
        out.append(('cube %g' % d_cap, v, f) + V.CUBE_LATTICE + (d_cap,))
    v, f = icosphere(2, 10.0)
    out.append(('sphere', v, f, [-12.3, -12.1, -11.9], 1.0, (24, 24, 24), 3.0))
    v, f = V.nested_shells()
    out.append(('shells', v, f, [-13.5, -4.6, -1.4], 1.0, (27, 9, 3), 2.0))
    v, f = V.two_spheres()
    out.append(('two', v, f, [-12.4, -5.2, -5.1], 1.0, (25, 10, 10), 1.5))
    return out


def test_margins_every_in_band_sign_is_clear():
    for name, v, f, lo, h, dims, d_cap in every_input():
        r = V.volume(v, f, lo, h, dims, d_cap)
        assert V.margins_clear(r), name
        assert 0 < r['in_band'].sum() < r['in_band'].size, name


def test_three_mutations_are_caught():
    assert sorted(V.MUTATIONS) == ['band_strict', 'seed_outside', 'successor']
    red = {m: [k for k, ok in dict(cube_checks(m), **position_checks(m)).items() if not ok] for m in V.MUTATIONS}
    assert 'exactly_at_cap' in red['band_strict'] and 'cap2_band' in red['band_strict']
    assert 'cutting_mask' in red['successor'] or 'cutting_far' in red['successor']
    assert 'inside' in red['seed_outside'] and 'outside' not in red['seed_outside']
    assert all(red.values())
