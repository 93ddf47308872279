"""The banded signed-distance volume on the device (csrc/nw_volume.hip) against its NumPy restatement (tests/mesh_volume_ref.py): the
magnitude of sd, the face, the mask and the field exactly, the signs by same_as_restatement's rule -- the equalities the compiled core
owes it in tests/test_volume_core_cpu.py -- on closed, open and mis-shaped meshes, on lattices around the wave and block sizes, through
one context; then against the merged units, which know nothing of it: distance_to_mesh bit for bit inside the band, rays.inside and
the winding number for the mask; and offset_surface against the surface nets' restatement and a sphere's closed form."""
import functools

import numpy as np
import pytest

import isosurface_ref as I
import mesh_distance_ref as D
import mesh_volume_ref as V
from ch_shrinkwrap_amd import volume as C
from ch_shrinkwrap_amd.isosurface import mean_edge_length
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
from test_volume_core_cpu import spanning_face

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    c = C.VolumeContext()
    yield c
    c.close()


def device(ctx, v, f, lo, h, dims, d_cap, signed=True):
    ctx.set_mesh(v, f, signed=signed)
    sd, face, mask = ctx.volume(lo, h, dims, d_cap, signed=signed, return_face=True, return_mask=True)
    shape = (int(dims[2]), int(dims[1]), int(dims[0]))
    assert sd.shape == face.shape == mask.shape == shape and mask.dtype == bool
    field = ctx.field()
    assert field.shape == shape
    return dict(sd=sd.ravel(), face=face.ravel(), mask=mask.ravel(), field=field.ravel(), info=dict(ctx.info))


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, lo, h, dims, d_cap, signed) by name; the restatement of each is computed once (reference)"""
    if name.startswith('cube '):
        return V.cube4() + V.CUBE_LATTICE + (float(name[5:]), True)
    if name.startswith('lattice '):
        dims = tuple(int(t) for t in name[8:].split('x'))
        if max(dims) == 70:                                       # the long axis crosses the cube, the others lie inside it
            lo = [-1.5 if d == 70 else 1.87 for d in dims]
            return V.cube4() + (np.float32(lo), 0.1, dims, 0.25, True)
        return V.cube4() + (np.float32([0.6, 0.7, -1.2]), 1.0, dims, 1.0, True)
    if name == 'sphere':
        return icosphere(2, 10.0) + (np.float32([-12.3, -12.1, -11.9]), 1.0, (24, 24, 24), 3.0, True)
    if name == 'shells':
        return V.nested_shells() + (np.float32([-13.5, -4.6, -1.4]), 1.0, (27, 9, 3), 2.0, True)
    if name == 'two':
        return V.two_spheres() + (np.float32([-12.4, -5.2, -5.1]), 1.0, (25, 10, 10), 1.5, True)
    if name in ('disk', 'disk unsigned'):
        return D.disk() + (np.float32([-2.6, -2.7, -1.3]), 0.5, (11, 11, 6), 0.75, name == 'disk')
    if name in ('needles', 'needles unsigned'):
        return D.needles() + (np.float32([-420.0, -410.0, -400.0]), 75.0, (12, 11, 12), 80.0, name == 'needles')
    if name == 'million':
        v, f = icosphere(2, 50.0)
        return (v + np.float32(1e6)).astype(np.float32), f, np.float32([1e6 - 66.0] * 3), 12.0, (11, 11, 11), 20.0, True
    if name == 'spanning':
        return spanning_face() + (np.float32([-13.3, -13.1, -12.9]), 2.0, (13, 13, 15), 3.0, False)
    if name == 'inside':
        v, f = D.cube()
        return (v * 50.0).astype(np.float32), f, np.float32([-10.5] * 3), 4.0, (5, 5, 5), 8.0, True
    if name == 'outside':
        v, f = D.cube()
        return (v * 50.0).astype(np.float32), f, np.float32([100.0, 90.0, -200.0]), 4.0, (5, 5, 5), 8.0, True
    if name == 'cutting':
        return D.l_prism() + (np.float32([0.3 - 0.125, 0.2 - 0.125, 0.1 - 0.125]), 0.25, (12, 11, 6), 0.25, True)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    v, f, lo, h, dims, d_cap, signed = case(name)
    return V.volume(v, f, lo, h, dims, d_cap, signed=signed)


def check(ctx, name):
    v, f, lo, h, dims, d_cap, signed = case(name)
    ref = reference(name)
    dev = device(ctx, v, f, lo, h, dims, d_cap, signed)
    n = V.same_as_restatement(dev, ref, signed)
    assert dev['info']['in_band'] == int(ref['in_band'].sum()) and dev['info']['nodes'] == ref['sd'].size
    assert not dev['info']['fan_capped']
    return dev, ref, n


CLOSED = ['cube 1', 'cube 2', 'cube 2.5', 'lattice 3x3x3', 'lattice 3x5x70', 'lattice 70x3x5', 'lattice 3x3x7', 'lattice 4x4x4', 'lattice 3x3x29',
          'lattice 4x8x8', 'sphere', 'shells', 'two', 'million', 'inside', 'outside', 'cutting']


# ---- parity and exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CLOSED)
def test_closed_meshes_equal_the_restatement_everywhere(ctx, name):
    dev, ref, n = check(ctx, name)
    assert V.margins_clear(ref) and n == ref['sd'].size                                    # every node compared in full
    v, f, lo, h, dims, d_cap, _ = case(name)
    assert (np.abs(dev['sd']) <= d_cap).all() and (np.abs(dev['sd'][dev['face'] == -1]) == d_cap).all()
    assert dev['info']['seed_face'] == int(np.argmin(D.point_triangles(ref['nodes'][:1], v, f)[0][0]))
    if name.startswith('cube '):
        want = V.cube4_sdf(ref['nodes'])
        near = np.abs(want) <= d_cap
        assert np.array_equal(dev['sd'][near], want[near]) and np.array_equal(dev['mask'], want < 0)
        on = want == 0                                                                       # nodes on vertices, edges and faces: +0.0
        assert on.sum() == 98 and (D.bits(dev['sd'][on]) == 0).all() and not dev['mask'][on].any()
        if d_cap == 2.0:
            assert (dev['face'][want == 2.0] >= 0).all() and (dev['face'][want == -2.0] >= 0).all()
    if name == 'inside':
        assert (dev['sd'] == -d_cap).all() and dev['mask'].all() and dev['info']['in_band'] == 0
    if name == 'outside':
        assert (dev['sd'] == d_cap).all() and not dev['mask'].any() and (dev['field'] == 0).all()
    if name == 'cutting':
        assert np.array_equal(dev['mask'], D.l_prism_inside(ref['nodes']))
    if name in ('lattice 3x5x70', 'lattice 70x3x5'):
        far = dev['face'] == -1
        assert (far & dev['mask']).sum() > 100 and (far & ~dev['mask']).sum() > 100          # both signs carried along lines of 70
    if name == 'shells':
        assert 0 < (dev['mask'] & (dev['face'] == -1)).sum() and dev['mask'].mean() < 0.9


@pytest.mark.parametrize('name', ['disk', 'disk unsigned', 'needles', 'needles unsigned', 'spanning'])
def test_open_and_mis_shaped_meshes(ctx, name):
    dev, ref, n = check(ctx, name)
    assert n > 50 and 0 < ref['in_band'].sum() < ref['sd'].size
    if name.endswith('unsigned') or name == 'spanning':
        assert n == ref['sd'].size and dev['info']['seed_face'] == -1 and (dev['sd'] >= 0).all()
    if name == 'spanning':
        assert (dev['face'] == len(case(name)[1]) - 1).sum() > 50


def test_an_exact_band_edge(ctx):
    v, f = V.cube4()
    lo, h, dims = V.CUBE_LATTICE
    at2 = np.flatnonzero(V.cube4_sdf(V.nodes(lo, h, dims)) == 2.0)
    cap = np.nextafter(2.0, 0.0)
    dev = device(ctx, v, f, lo, h, dims, cap)
    assert (dev['face'][at2] == -1).all() and (dev['sd'][at2] == cap).all()
    V.same_as_restatement(dev, V.volume(v, f, lo, h, dims, cap), True)


def test_one_context_across_meshes_lattices_and_bands(ctx):
    """the centroids are binned again when the band asks for another cell size; nothing of an earlier call shows"""
    first = check(ctx, 'sphere')[0]
    cells = first['info']['cells']
    check(ctx, 'lattice 3x3x3')
    check(ctx, 'needles unsigned')
    v, f, lo, h, dims, d_cap, _ = case('sphere')
    ctx.set_mesh(v, f)
    wide = ctx.volume(lo, h, dims, 9.0).ravel()                                             # a wider band on the mesh at hand: a coarser grid
    assert ctx.info['cells'] < cells
    again = device(ctx, v, f, lo, h, dims, d_cap)
    assert again['info']['cells'] == cells
    for k in ('sd', 'face', 'mask', 'field'):
        assert np.array_equal(again[k], first[k])
    near = first['face'] >= 0
    assert np.array_equal(D.bits(wide[near]), D.bits(first['sd'][near])) and np.array_equal(np.signbit(wide), np.signbit(first['sd']))


def test_the_host_output_path_and_the_field_pointer(ctx):
    v, f, lo, h, dims, d_cap, _ = case('two')
    ref = reference('two')
    ctx.set_mesh(v, f)
    assert ctx.volume(lo, h, dims, d_cap, return_sd=False) is None                           # nothing but info comes back
    assert ctx.info['in_band'] == int(ref['in_band'].sum()) and ctx.field_pointer() != 0
    assert np.array_equal(ctx.field().ravel(), ref['field'])
    sd, mask = ctx.volume(lo, h, dims, d_cap, return_mask=True)
    assert np.array_equal(mask.ravel(), ref['mask']) and np.array_equal(D.bits(sd.ravel()), D.bits(ref['sd']))
    out = C.signed_distance_volume((v, f), h, band=d_cap, lo=lo, dims=dims, context=ctx)
    assert np.array_equal(D.bits(out['sd']), D.bits(sd)) and np.array_equal(out['face'].ravel(), ref['face']) and out['d_cap'] == d_cap
    with pytest.raises(RuntimeError):
        ctx.volume(lo, h, dims, 0.5)                                                          # d_cap < h
    assert ctx.field_pointer() == 0
    with pytest.raises(RuntimeError):
        C.VolumeContext.set_mesh(ctx, v, f, signed=False).volume(lo, h, dims, d_cap, signed=True)   # no twin table in the context


# ---- against the merged units -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sphere', 'shells', 'million', 'cutting'])
def test_in_band_equals_distance_to_mesh_bit_for_bit(ctx, name):
    from ch_shrinkwrap_amd import distance
    v, f, lo, h, dims, d_cap, _ = case(name)
    dev = device(ctx, v, f, lo, h, dims, d_cap)
    p = V.nodes(lo, h, dims)
    dist, face = distance.distance_to_mesh(p, (v, f), signed=True, return_face=True)
    near = np.abs(dist) <= d_cap
    assert np.array_equal(dev['face'] >= 0, near) and near.sum() > 50
    assert np.array_equal(D.bits(dev['sd'][near]), D.bits(dist[near])) and np.array_equal(dev['face'][near], face[near])
    assert np.array_equal(dev['mask'][near], dist[near] < 0)


@pytest.mark.parametrize('name', ['sphere', 'shells', 'two'])
def test_the_mask_equals_ray_parity_and_the_winding_number(ctx, name):
    from ch_shrinkwrap_amd import rays, surgery
    v, f, lo, h, dims, d_cap, _ = case(name)
    dev = device(ctx, v, f, lo, h, dims, d_cap)
    ref = reference(name)
    p = ref['nodes']
    diag = float(np.linalg.norm(v.astype(np.float64).max(0) - v.astype(np.float64).min(0)))
    clear = ref['u'] > 1e-6 * diag
    assert clear.sum() > 0.99 * clear.size
    assert np.array_equal(dev['mask'][clear], rays.inside(p, (v, f))[clear])
    s = surgery.SurgeryContext()
    try:
        w = s.winding(v, f, np.zeros(len(f), np.int32), 1, p)[:, 0]
    finally:
        s.close()
    assert np.array_equal(dev['mask'][clear], (w >= 0.5)[clear])


def test_the_python_surface():
    mesh = TriMesh(*icosphere(2, 10.0))
    out = mesh.signed_distance_volume(2.0)
    assert out['d_cap'] == 6.0 and out['h'] == 2.0 and out['sd'].shape == tuple(out['dims'][::-1]) and out['info']['in_band'] > 0
    c = (np.asarray(out['dims']) // 2)[::-1]
    assert out['sd'][tuple(c)] == -6.0 and out['mask'][tuple(c)] and out['sd'][0, 0, 0] == 6.0 and out['face'][0, 0, 0] == -1
    m = mesh.voxelize(2.0)
    assert m.dtype == bool and m[tuple((np.asarray(m.shape) // 2))] and not m[0].any()
    vol = m.sum() * 8.0
    assert abs(vol / (4.0 / 3.0 * np.pi * 1000.0) - 1.0) < 0.15
    ns = {'membrane': mesh}
    sdf = C.MeshToVolume(voxel_size=2.0).execute(ns)
    assert ns['membrane_sdf'] is sdf and np.array_equal(D.bits(sdf['sd']), D.bits(out['sd']))
    un = C.signed_distance_volume(mesh, 2.0, signed=False)
    assert np.array_equal(un['sd'], np.abs(out['sd'])) and not un['mask'].any()
    v, f = D.cube()
    with pytest.raises(Exception):                                                           # a non-manifold edge has no twin table
        C.signed_distance_volume((np.concatenate([v, [[0, 0, 5]]]).astype(np.float32), np.concatenate([f, [[0, 1, 8]]]).astype(np.int32)), 0.5)


# ---- offset surfaces --------------------------------------------------------------------------------------------------------------------
def test_offset_surface_equals_the_surface_nets_of_the_restatement():
    v, f = icosphere(2, 10.0)
    for offset in (2.0, -1.5):
        s = C.offset_surface((v, f), offset, voxel_size=2.0, remesh=False)
        info = s.info
        assert info['d_cap'] == abs(offset) + 4.0 and info['pad'] == (3 if offset > 0 else 2) and info['thr'] == C.field_threshold(info['d_cap'], offset)
        ref = V.volume(v, f, info['lo'], info['h'], info['dims'], info['d_cap'])
        assert V.margins_clear(ref)
        dims = info['dims']
        rv, rf, rk = I.surface_nets(ref['field'].reshape(int(dims[2]), int(dims[1]), int(dims[0])), info['thr'], info['lo'], info['h'])
        I.compare_mesh('offset %g' % offset, s.vertices, s.faces, info['keys'], rv, rf, rk)


@functools.lru_cache(maxsize=None)
def sphere_offsets():
    v, f = icosphere(3, 50.0)
    return {o: C.offset_surface(TriMesh(v, f), o, voxel_size=4.0, remesh=False) for o in (-10.0, 0.0, 10.0)}


def test_offset_surfaces_of_a_sphere():
    R, h = 50.0, 4.0
    v, f = icosphere(3, R)
    # the polyhedron's distance from the sphere: R minus its distance from the centre (the deepest point of a face)
    s = R - float(np.sqrt(D.distance(np.zeros((1, 3)), v, f)['d2'][0]))
    assert 0.0 < s < 1.0
    tol = h * np.sqrt(3.0) + s              # a surface-net vertex lies in a cell the level set crosses: one cell diagonal, plus s
    volumes = []
    for o, surf in sorted(sphere_offsets().items()):
        sv, sf = surf.vertices, surf.faces
        assert (I.edge_use(sf) == 2).all() and I.directed_edges_balanced(sf)                 # closed, manifold, oriented
        comp = I.components(sv, sf)
        assert len(comp) == 1 and comp[0][1] == 2                                            # one component of genus 0
        volumes.append(comp[0][2])
        rad = np.linalg.norm(sv.astype(np.float64), axis=1)
        print('offset %g: radii %.3f .. %.3f, R + offset = %g, tolerance %.3f' % (o, rad.min(), rad.max(), R + o, tol))
        assert (np.abs(rad - (R + o)) <= tol).all()
    assert 0 < volumes[0] < volumes[1] < volumes[2]


def test_offset_surface_remeshed_and_as_a_recipe():
    mesh = TriMesh(*icosphere(3, 50.0))
    ns = {'membrane': mesh}
    surf = C.OffsetSurface(offset=10.0, voxel_size=4.0).execute(ns)
    assert ns['offset_membrane'] is surf and surf.info['target_edge_length'] > 0
    assert (I.edge_use(surf.faces) == 2).all()
    comp = I.components(surf.vertices, surf.faces)
    assert len(comp) == 1 and comp[0][1] == 2 and comp[0][2] > 4.0 / 3.0 * np.pi * 50.0 ** 3
    auto = mesh.offset_surface(5.0, remesh=False)                                            # the voxel size from the mesh's mean edge length
    assert abs(auto.info['h'] - mean_edge_length(np.asarray(mesh.vertices), np.asarray(mesh.faces))) < 1e-3 and (I.edge_use(auto.faces) == 2).all()

