"""The six mesh query units (distance, intersections, rays, volume, proximity, mapping) take a mesh in through one face grid
(bq::FaceGrid of csrc/nw_bq.h).  What their ABIs expose of it -- the volume unit's and the mapping unit's cell counts, the mapping and
proximity units' cell sizes, the proximity unit's cell count with and without a cell size of the caller's -- is compared here with the
sizing restated in NumPy from the float64 centroid restatement: rho_f enlarged by 1 + 1e-9, their sum in the reduction's own order (256
strided partial sums, a butterfly within each wave, the four waves in order), the centroids' box, the unit's candidate cell size, the
floor of a 1024th of the widest axis, and the widening by tenths.  A band unit called twice with one band must give the same bytes (the
grid at hand is kept); a third band wide enough that half of d_cap + rho_max exceeds twice the mean rho makes it bin anew, which shows
as another cell count wherever the restatement says the counts differ (a mesh of one or two faces has one cell whatever the band).
Every expected value is checked on the CPU, in the restatement, before the device is asked."""
import contextlib
import functools

import numpy as np
import pytest

from ch_shrinkwrap_amd import distance, intersections, mapping, proximity, rays, volume
from ch_shrinkwrap_amd.trimesh import icosphere
from test_face_grid_core_cpu import RULE, SLACK, cell_band, cell_fixed, cell_proximity, centroid_ref, size_grid_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
BANDS = (1.0, 1.0, 12.0)                      # the band, the same again (the grid is kept), a wide one (the grid is binned anew)
MESHES = ['icosphere', 'one face', 'two faces', 'flat sheet', 'icosphere at 1e6']


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == 'icosphere':
        v, f = icosphere(2, 10.0)
    elif name == 'icosphere at 1e6':
        v, f = icosphere(2, 10.0)
        v = v + F32(1e6)
    elif name == 'one face':
        v, f = F32([[0, 0, 0], [3, 0, 0], [0, 4, 1]]), np.int32([[0, 1, 2]])
    elif name == 'two faces':
        v, f = F32([[0, 0, 0], [3, 0, 0], [0, 4, 1], [3, 4, -1]]), np.int32([[0, 1, 2], [2, 1, 3]])
    elif name == 'flat sheet':                  # 8 x 8 quads, z constant: the centroids' box has no extent along z
        x, y = np.meshgrid(np.arange(9), np.arange(9), indexing='ij')
        v = np.stack([x.ravel(), y.ravel(), np.full(81, 5.0)], 1).astype(F32)
        q = (np.arange(8)[:, None] * 9 + np.arange(8)[None, :]).ravel()
        f = np.concatenate([np.stack([q, q + 9, q + 10], 1), np.stack([q, q + 10, q + 1], 1)]).astype(np.int32)
    else:
        raise KeyError(name)
    v, f = np.ascontiguousarray(v, F32), np.ascontiguousarray(f, np.int32)
    assert len(f) == {'icosphere': 320, 'icosphere at 1e6': 320, 'one face': 1, 'two faces': 2, 'flat sheet': 128}[name]
    return v, f


def reduce_rho(rho):
    """k_bq_rho_reduce's sum: thread t adds rho[t], rho[t + 256], ... in order; a butterfly within each wave of 64 (offsets 32 .. 1);
    then ((w0 + w1) + w2) + w3"""
    s = np.zeros(256)
    for j0 in range(0, len(rho), 256):
        part = rho[j0:j0 + 256]
        s[:len(part)] = s[:len(part)] + part
    lane = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lane ^ o]
    return float(((s[0] + s[64]) + s[128]) + s[192])


@functools.lru_cache(maxsize=None)
def stats(name):
    """what FaceGrid::set_faces keeps of the mesh: F, sum and max of rho_f, the extent of the centroids' box"""
    v, f = mesh(name)
    cen, rho = centroid_ref(v[f])
    rho = rho * (1.0 + SLACK)
    ext = cen.max(0) - cen.min(0)
    return dict(nf=len(f), rho_sum=reduce_rho(rho), rho_max=float(rho.max()), ext=[float(e) for e in ext], emax=float(ext.max()))


def grid(name, rule, d_cap, cell_size=0.0):
    """(cells, cell size) of the grid a unit makes for the band"""
    s = stats(name)
    h0 = cell_size if cell_size > 0.0 else rule(s['rho_sum'], s['nf'], s['rho_max'], d_cap, s['emax'])
    ok, h, dims = size_grid_ref(s['nf'], s['ext'], h0)
    assert ok
    return dims[0] * dims[1] * dims[2], h, h0


@pytest.mark.parametrize('name', MESHES)
def test_the_bands_give_the_starting_cells_intended(name):
    """(no device is asked anything here: the fixtures are checked in the restatement first)"""
    s = stats(name)
    m = s['rho_sum'] / s['nf']
    assert RULE == (16, 1 << 26, 1025, 400)
    if s['emax'] == 0.0:
        assert name == 'one face'
        for d in BANDS:
            assert grid(name, cell_band, d) == (1, 1.0, 1.0) and grid(name, cell_proximity, d) == (1, 1.0, 1.0)
        return
    assert (s['ext'][2] == 0.0) == (name in ('flat sheet',))
    near, _, wide = BANDS
    # the narrow band leaves the cell at twice the mean rho, the wide one takes it to half of d_cap + rho_max
    assert (near + s['rho_max']) / 2.0 < 2.0 * m and grid(name, cell_band, near)[2] == 2.0 * m == grid(name, cell_fixed, near)[2]
    assert (wide + s['rho_max']) / 2.0 > 2.0 * m and grid(name, cell_band, wide)[2] == (wide + s['rho_max']) / 2.0
    assert grid(name, cell_proximity, near)[2] == 2.0 * m and grid(name, cell_proximity, wide)[2] == (wide + s['rho_max']) / 2.0 < 16.0 * m
    assert grid(name, cell_proximity, np.inf)[2] == 16.0 * m
    # ... which shows in the number of cells, but for the mesh of two faces: its two centroids share a cell at either size
    if name == 'two faces':
        assert grid(name, cell_band, near)[0] == grid(name, cell_band, wide)[0] == 1
    else:
        assert grid(name, cell_band, near)[0] > grid(name, cell_band, wide)[0] > 1
        assert grid(name, cell_proximity, near)[0] > grid(name, cell_proximity, wide)[0]


def lattice(v):
    lo = (v.min(0) - F32(1.5)).astype(F32)
    return lo, 1.0, (5, 4, 3)


def cloud(v, n=300):
    rng = np.random.default_rng(5)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    return lo - 2.0 + rng.random((n, 3)) * (hi - lo + 4.0)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', MESHES)
def test_the_band_units_size_one_grid(name):
    v, f = mesh(name)
    pts = cloud(v)
    lo, h, dims = lattice(v)
    other = (v + F32(0.25)).astype(F32)
    with contextlib.ExitStack() as stack:
        vol, mp, prox = (stack.enter_context(contextlib.closing(c())) for c in (volume.VolumeContext, mapping.MappingContext, proximity.ProximityContext))
        vol.set_mesh(v, f, signed=False)
        mp.set_mesh(v, f)
        prox.set_mesh(v, f)
        seen = []
        for d_cap in BANDS:
            cells, cell_size, _ = grid(name, cell_band, d_cap)
            sd = vol.volume(lo, h, dims, d_cap, signed=False)
            field = vol.field()
            print('%s band %g: volume cells %d, restated %d' % (name, d_cap, vol.info['cells'], cells))
            assert vol.info['cells'] == cells
            r = mp.map(pts, band=d_cap)
            print('%s band %g: mapping cells %d size %.17g, restated %d %.17g' % (name, d_cap, r['info']['cells'], r['info']['cell_size'], cells, cell_size))
            assert r['info']['cells'] == cells and np.float64(r['info']['cell_size']).tobytes() == np.float64(cell_size).tobytes()
            pcells, psize, _ = grid(name, cell_proximity, d_cap)
            q = prox.query(other, f, band=d_cap, return_closest=True)
            print('%s band %g: proximity cells %d size %.17g, restated %d %.17g' % (name, d_cap, q['info']['cells'], q['info']['cell_size'], pcells, psize))
            assert q['info']['cells'] == pcells and np.float64(q['info']['cell_size']).tobytes() == np.float64(psize).tobytes()
            seen.append((sd, field, dict(vol.info), r, q))
        # the same band again: the grid at hand, and the same bytes and counters from all three
        a, b = seen[0], seen[1]
        assert same(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2]
        for k in ('face', 'weights', 'distance', 'closest', 'mass', 'count'):
            assert same(a[3][k], b[3][k]), k
        assert a[3]['info'] == b[3]['info']
        for k in ('distance', 'partner', 'kind', 'closest_a', 'closest_b'):
            assert same(a[4][k], b[4][k]), k
        assert a[4]['info'] == b[4]['info']
        # the wide band: binned anew, another number of cells where the restatement has another
        assert (seen[2][2]['cells'] != a[2]['cells']) == (grid(name, cell_band, BANDS[2])[0] != grid(name, cell_band, BANDS[0])[0])
        assert (seen[2][4]['info']['cells'] != a[4]['info']['cells']) == (grid(name, cell_proximity, BANDS[2])[0] != grid(name, cell_proximity, BANDS[0])[0])
        # ... and back: the narrow band's grid once more, with the first call's results
        sd = vol.volume(lo, h, dims, BANDS[0], signed=False)
        assert same(sd, a[0]) and vol.info['cells'] == a[2]['cells']
        # no band, and a cell size of the caller's, which no band changes
        cells, size, _ = grid(name, cell_proximity, np.inf)
        q = prox.query(other, f)
        assert q['info']['cells'] == cells and np.float64(q['info']['cell_size']).tobytes() == np.float64(size).tobytes()
        prox.set_mesh(v, f, cell_size=2.5)
        for d_cap in (BANDS[0], BANDS[2], np.inf):
            cells, size, h0 = grid(name, cell_proximity, d_cap, cell_size=2.5)
            q = prox.query(other, f, band=d_cap)
            assert h0 == 2.5 and q['info']['cells'] == cells and np.float64(q['info']['cell_size']).tobytes() == np.float64(size).tobytes()


@pytest.mark.parametrize('name', MESHES)
def test_the_fixed_units_take_the_same_mesh_in(name):
    """the distance, intersection and ray units bin once, in set_mesh; their answers agree with the band units' on the same mesh"""
    v, f = mesh(name)
    pts = cloud(v)
    with contextlib.ExitStack() as stack:
        dc, xc, rc, mp = (stack.enter_context(contextlib.closing(c()))
                          for c in (distance.DistanceContext, intersections.IntersectionContext, rays.RayContext, mapping.MappingContext))
        dc.set_mesh(v, f)
        dist, closest, face = dc.query(pts, signed=False, return_closest=True, return_face=True)
        mp.set_mesh(v, f)
        r = mp.map(pts, band=BANDS[2])
        near = r['face'] >= 0
        assert near.any() and same(r['distance'][near], dist[near]) and same(r['face'][near], face[near]) and same(r['closest'][near], closest[near])
        assert (dist[~near] > BANDS[2]).all()
        xc.set_mesh(v, f)
        x = xc.find()
        assert x['n_pairs'] == 0 and not x['count'].any()
        rc.set_mesh(v, f)
        c = centroid_ref(v[f])[0]
        n = np.cross(v[f[:, 1]].astype(np.float64) - v[f[:, 0]], v[f[:, 2]].astype(np.float64) - v[f[:, 0]])
        n /= np.linalg.norm(n, axis=1)[:, None]
        hit = rc.cast(c + 3.0 * n, -n)                       # onto every face from 3 above its centroid
        assert np.array_equal(hit['face'], np.arange(len(f))) and np.allclose(hit['t'], 3.0, rtol=0, atol=1e-6 * max(1.0, float(np.abs(v).max())))
        # the same mesh a second time through the same contexts: the same bytes
        dc.set_mesh(v, f)
        assert same(dc.query(pts, signed=False), dist)
        rc.set_mesh(v, f)
        again = rc.cast(c + 3.0 * n, -n)
        assert same(again['t'], hit['t']) and same(again['face'], hit['face'])
