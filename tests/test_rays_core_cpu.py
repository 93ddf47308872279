"""
Ray casting's arithmetic, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_rays_core.h holds the ray-face test and the walk through
the centroid grid as __host__ __device__ functions; this test compiles them for the CPU (g++ -ffp-contract=off) behind a shim of its
own and asks for the bits of the NumPy restatement (tests/mesh_rays_ref.py: t, face, info, hits) -- from the definition's loop over
all faces, and from the walk over a grid that the test lays out in NumPy, in first-hit and in count mode.  The shim is built on
demand in pytest's temporary directory.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_rays_ref as R
from conftest import ROOT

CORE = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_rays_core.h')

SHIM = r'''
#include "nw_rays_core.h"
static void put(const nwc_best &b, long long i, double *t, int *face, int *info, int *hits)
{
    t[i] = b.t; face[i] = b.face; info[i] = b.info; hits[i] = b.hits;
}
extern "C" void shim_cast(const float *pos, const int *faces, int nf, const double *o, const double *d, long long n, const int *sv, const int *sf,
                          double t_max, double *t, int *face, int *info, int *hits)
{
    for (long long i = 0; i < n; ++i)
        put(nwc_cast_all_faces(pos, faces, nf, nwc_make_ray(o + 3 * i, d + 3 * i, sv ? sv[i] : -1, sf ? sf[i] : -1, t_max)), i, t, face, info, hits);
}
extern "C" void shim_walk(const float *pos, const int *faces, int nf, const double *pts, const int *cstart, const double *rho, const double *box,
                          const int *dims, int count, const double *o, const double *d, long long n, const int *sv, const int *sf, double t_max,
                          double *t, int *face, int *info, int *hits, long long *stats)
{
    nwc_mesh m;
    m.pos = pos; m.faces = faces; m.nf = nf; m.pts = (const nwc_point *)pts; m.cstart = cstart; m.rho = rho;
    m.rho_max = box[0]; m.lo0 = box[1]; m.lo1 = box[2]; m.lo2 = box[3]; m.hi0 = box[4]; m.hi1 = box[5]; m.hi2 = box[6]; m.h = box[7];
    m.d0 = dims[0]; m.d1 = dims[1]; m.d2 = dims[2];
    for (long long i = 0; i < n; ++i) {
        const nwc_ray r = nwc_make_ray(o + 3 * i, d + 3 * i, sv ? sv[i] : -1, sf ? sf[i] : -1, t_max);
        nwc_walk_stats st;
        put(count ? nwc_walk<true>(m, r, &st) : nwc_walk<false>(m, r, &st), i, t, face, info, hits);
        stats[3 * i] = st.pieces; stats[3 * i + 1] = st.read; stats[3 * i + 2] = st.tested;
    }
}
extern "C" void shim_pairs(const float *pos, const int *faces, const double *o, const double *d, long long n, unsigned char *hit, double *t,
                           unsigned char *exits)
{
    for (long long i = 0; i < n; ++i) {
        const nwx_tri T = nwx_load(pos, faces, i);
        nwx_v3 c;
        const double rho = nwx_face_centroid(T, &c) * (1.0 + NWC_RHO_SLACK);
        bool e = false;
        t[i] = 0.0;
        hit[i] = nwc_ray_face(nwc_make_ray(o + 3 * i, d + 3 * i, -1, -1, INFINITY), (int)i, T, c, rho, t + i, &e) ? 1 : 0;
        exits[i] = e ? 1 : 0;
    }
}
extern "C" int shim_point_size(void) { return (int)sizeof(nwc_point); }
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwc_shim')
    src, lib = os.path.join(str(d), 'shim.cpp'), os.path.join(str(d), 'libnwc_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', os.path.dirname(CORE),
                           '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    L.shim_cast.argtypes = [vp, vp, i32, vp, vp, i64, vp, vp, f64, vp, vp, vp, vp]
    L.shim_cast.restype = None
    L.shim_walk.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, i64, vp, vp, f64, vp, vp, vp, vp, vp]
    L.shim_walk.restype = None
    assert L.shim_point_size() == 32
    p = lambda a: None if a is None else a.ctypes.data

    def arrays(v, f, o, d, sv, sf):
        v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
        o, d = np.ascontiguousarray(o, np.float64).reshape(-1, 3), np.ascontiguousarray(d, np.float64).reshape(-1, 3)
        sv = None if sv is None else np.ascontiguousarray(sv, np.int32)
        sf = None if sf is None else np.ascontiguousarray(sf, np.int32)
        n = o.shape[0]
        out = dict(t=np.empty(n), face=np.empty(n, np.int32), info=np.empty(n, np.int32), hits=np.empty(n, np.int32))
        return v, f, o, d, sv, sf, n, out

    def cast(v, f, o, d, sv=None, sf=None, t_max=np.inf):
        v, f, o, d, sv, sf, n, out = arrays(v, f, o, d, sv, sf)
        L.shim_cast(p(v), p(f), len(f), p(o), p(d), n, p(sv), p(sf), t_max, p(out['t']), p(out['face']), p(out['info']), p(out['hits']))
        return out

    def walk(v, f, o, d, sv=None, sf=None, t_max=np.inf, count=False, h=None):
        v, f, o, d, sv, sf, n, out = arrays(v, f, o, d, sv, sf)
        g = R.centroid_grid(v, f, h)
        pts = np.zeros(len(f), np.dtype([('c', np.float64, 3), ('i', np.int64)]))
        pts['c'], pts['i'] = g['cen'][g['order']], g['order']
        box = np.array([g['rho_max']] + list(g['lo']) + list(g['hi']) + [g['h']], np.float64)
        dims = np.ascontiguousarray(g['dims'], np.int32)
        rho = np.ascontiguousarray(g['rho'])
        out['stats'] = np.zeros((n, 3), np.int64)
        L.shim_walk(p(v), p(f), len(f), p(pts), p(g['cstart']), p(rho), p(box), p(dims), int(count), p(o), p(d), n, p(sv), p(sf), t_max,
                    p(out['t']), p(out['face']), p(out['info']), p(out['hits']), p(out['stats']))
        return out
    L.shim_pairs.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
    L.shim_pairs.restype = None

    def pairs(v, f, o, d):
        v, f, o, d, _, _, n, _ = arrays(v, f, o, d, None, None)
        hit, t, ex = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.uint8)
        L.shim_pairs(p(v), p(f), p(o), p(d), n, p(hit), p(t), p(ex))
        return dict(hit=hit.astype(bool), t=t, exits=ex.astype(bool))
    cast.walk, cast.pairs = walk, pairs
    return cast


def everything_agrees(shim, v, f, o, d, sv=None, sf=None, t_max=np.inf, h=None):
    """the definition's loop, the walk in count mode and the walk in first-hit mode, against the restatement"""
    ref = R.cast(v, f, o, d, sv, sf, t_max)
    R.same(shim(v, f, o, d, sv, sf, t_max), ref)
    counted = shim.walk(v, f, o, d, sv, sf, t_max, count=True, h=h)
    R.same(counted, ref)
    first = shim.walk(v, f, o, d, sv, sf, t_max, count=False, h=h)
    R.same(first, ref, count=False)
    assert (first['stats'] <= counted['stats']).all()
    return ref, counted['stats']


def test_the_lattice_cube(shim):
    v, f, ids = R.lattice_box()
    bottom = np.array([[x, y, 0] for x in (1, 2, 3) for y in (1, 2, 3)], np.float64)
    up = np.tile([0.0, 0.0, 1.0], (9, 1))
    ref, _ = everything_agrees(shim, v, f, bottom, up)
    assert (ref['t'] == 4.0).all() and (ref['hits'] == 6).all() and (ref['info'] == 1).all()
    ref, _ = everything_agrees(shim, v, f, bottom, up, sv=[ids[tuple(int(c) for c in b)] for b in bottom])
    assert (ref['t'] == 4.0).all() and (ref['hits'] == 6).all()
    # through vertices and edge midpoints of the lattice, from inside and from outside, along every axis and the diagonals
    o, d = [], []
    for start in ([1, 1, 1], [2, 1, 3], [1.5, 2, 2], [2, 2.5, 1], [-3, 2, 2], [1, 1, -2], [7, 7, 7], [0, 0, 0], [4, 2, 2]):
        for step in ([1, 0, 0], [0, -1, 0], [0, 0, 1], [1, 1, 0], [0, 1, -1], [1, 1, 1], [-1, -1, -1], [1, -1, 1], [2, 1, 0], [0, 0, 0]):
            o.append(start)
            d.append(step)
    ref, _ = everything_agrees(shim, v, f, o, d)
    assert (ref['hits'] > 2).sum() > 20                                                   # fans
    for t_max, hit in ((4.0, True), (np.nextafter(4.0, 0.0), False), (np.inf, True)):
        ref, _ = everything_agrees(shim, v, f, bottom, up, t_max=t_max)
        assert (ref['face'] >= 0).all() == hit and (ref['face'] < 0).all() == (not hit)
    sf = R.cast(v, f, bottom, up)['face']
    ref, _ = everything_agrees(shim, v, f, bottom, up, sf=sf)
    assert (ref['t'] == 4.0).all() and (ref['hits'] == 5).all() and (ref['face'] != sf).all()


@pytest.mark.parametrize('h', [None, 0.05, 0.31, 3.0])
def test_the_noisy_sphere_on_several_grids(shim, h):
    v, f = R.noisy_sphere()
    o, d = R.mixed_rays(v, 400, 5)
    ref, stats = everything_agrees(shim, v, f, o, d, h=h)
    assert 100 < (ref['face'] >= 0).sum() < 350 and (ref['hits'] >= 2).sum() > 50
    n = R.vertex_normals(v, f)
    ref, _ = everything_agrees(shim, v, f, np.asarray(v, np.float64), -n, sv=np.arange(len(v)), h=h)
    assert (ref['face'] >= 0).all() and (ref['info'] == 1).all()
    ref, _ = everything_agrees(shim, v, f, o, d, t_max=0.7, h=h)
    assert 20 < (ref['face'] >= 0).sum() < 300


def test_one_oversize_face_is_slow_and_exact(shim):
    v, f = R.noisy_sphere(oversize=True)
    o, d = R.mixed_rays(v[:-3], 200, 6)
    ref, stats = everything_agrees(shim, v, f, o, d)
    walked = stats[:, 0] > 0
    assert walked.sum() > 100 and (stats[walked, 1] >= len(f)).all()                       # every ray that reaches the box reads every centroid
    assert (ref['face'] == len(f) - 1).sum() > 5
    plain = shim.walk(*R.noisy_sphere(), o, d, count=True)['stats']
    assert stats[:, 1].sum() > 20 * plain[:, 1].sum()


def test_a_mesh_a_million_from_the_origin(shim):
    v, f = R.sphere(2, 100.0, 1e6)
    assert np.spacing(np.abs(v).min()) == np.float32(0.0625)
    o, d = R.mixed_rays(v, 300, 7)
    ref, _ = everything_agrees(shim, v, f, o, d)
    assert 80 < (ref['face'] >= 0).sum() < 280
    ref, _ = everything_agrees(shim, v, f, np.asarray(v, np.float64), -R.vertex_normals(v, f), sv=np.arange(len(v)))
    assert (ref['face'] >= 0).all() and (np.abs(ref['t'] - 200.0) < 2.0).all()


def test_rays_from_five_thousand_radii_away(shim):
    v, f = R.noisy_sphere()
    rng = np.random.default_rng(8)
    u = rng.normal(size=(200, 3))
    o = 5000.0 * u / np.linalg.norm(u, axis=1)[:, None]
    d = rng.uniform(-0.8, 0.8, (200, 3)) - o
    ref, _ = everything_agrees(shim, v, f, o, d)
    assert (ref['face'] >= 0).sum() > 150 and (ref['hits'][ref['face'] >= 0] >= 2).all()


@pytest.mark.parametrize('length', [1e300, 1e155, 1e100, 1e-100, 1e-150, 3e-162, 1e-170, 1e-300])
def test_directions_of_every_finite_length(shim, length):
    """d.d leaves double's normal range beyond |d| = 1e154 (L = inf) and below 1e-154 (L with few digits or none): the walk follows
    the direction scaled by its largest component, so it gives the definition's answer at every length, and walks no farther than
    at length one.  Where d.d is zero (below about 1e-162) the definition says that nothing is hit."""
    v, f = R.sphere(3)
    o, d = R.mixed_rays(v, 400, 5)
    unit = d / np.linalg.norm(d, axis=1)[:, None]
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        ref, stats = everything_agrees(shim, v, f, o, unit * length)
        _, stats_one = everything_agrees(shim, v, f, o, unit)
        _, _ = everything_agrees(shim, v, f, o, unit * length, t_max=100.0 / length)
    if length < 1e-162:
        assert (ref['face'] == -1).all() and (stats == 0).all()
    else:
        assert 100 < (ref['face'] >= 0).sum() < 350
        assert (stats[:, 0] <= stats_one[:, 0] + 1).all()                                          # pieces: bounded by the grid, not by |d|


def test_needles_of_aspect_ten_thousand(shim):
    rng = np.random.default_rng(23)
    tris = []
    for i in range(600):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3))
        w /= np.linalg.norm(w)
        c = rng.normal(scale=0.02, size=3)
        tris.append(np.array([c - 50.0 * u, c + 50.0 * u, c + rng.uniform(-0.4, 0.4) * 50.0 * u + 0.01 * w]))
    from mesh_intersections_ref import soup
    v, f = soup(*tris)
    o = rng.normal(scale=20.0, size=(500, 3))
    d = rng.normal(scale=0.5, size=(500, 3)) - o                                          # aimed at the knot in the middle
    ref, _ = everything_agrees(shim, v, f, o, d)
    assert 50 < (ref['hits'] > 0).sum() and ref['hits'].max() >= 3


def test_flat_faces_open_patches_and_small_meshes(shim):
    from mesh_intersections_ref import A_TRI, soup
    # one face, two faces, a grid one cell thick (a flat patch)
    o, d = R.mixed_rays(np.array([[0, 0, -1], [4, 4, 1]], np.float32), 200, 9)
    ref, _ = everything_agrees(shim, A_TRI, [[0, 1, 2]], o, d)
    assert 5 < (ref['face'] == 0).sum() < 150
    v, f = soup(A_TRI, A_TRI + np.float32([0, 0, 0.5]))
    ref, _ = everything_agrees(shim, v, f, o, d)
    assert (ref['hits'] == 2).sum() > 5
    n = 9
    gx, gy = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    pv = np.stack([gx.ravel(), gy.ravel(), np.zeros(n * n)], axis=1).astype(np.float32)
    pf = np.array([t for i in range(n - 1) for j in range(n - 1) for t in ([i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1],
                                                                               [i * n + j, (i + 1) * n + j + 1, i * n + j + 1])], np.int32)
    assert R.centroid_grid(pv, pf)['dims'][2] == 1
    o, d = R.mixed_rays(np.array([[0, 0, -2], [8, 8, 2]], np.float32), 300, 10)
    ref, _ = everything_agrees(shim, pv, pf, o, d)
    assert 30 < (ref['face'] >= 0).sum() < 290
    # a ray in the patch's plane (den == 0) hits nothing; one leaving through the border neither
    ref, _ = everything_agrees(shim, pv, pf, [[-1, 3.3, 0], [4.2, 4.1, 0]], [[1, 0, 0], [1, 0.3, 0]])
    assert (ref['face'] == -1).all() and (ref['hits'] == 0).all() and np.isinf(ref['t']).all()
    # flat faces among real ones: a repeated id, three collinear vertices
    fv = np.concatenate([pv, [[1, 1, 1], [2, 2, 2], [3, 3, 3]]]).astype(np.float32)
    ff = np.concatenate([pf[:20], [[0, 0, 5], [81, 82, 83]], pf[20:]]).astype(np.int32)
    ref, _ = everything_agrees(shim, fv, ff, o, d)
    assert not np.isin(ref['face'], [20, 21]).any() and (ref['face'] >= 0).sum() > 30


def test_ten_thousand_random_ray_face_pairs(shim):
    """ray i against face i alone: hit, t and the sign of den"""
    rng = np.random.default_rng(31)
    n, blk = 10000, 100
    v = rng.normal(size=(3 * n, 3)).astype(np.float32)
    f = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    o = rng.normal(scale=2.0, size=(n, 3))
    d = (v.astype(np.float64).reshape(n, 3, 3) * rng.dirichlet([1, 1, 1], n)[:, :, None]).sum(1) + rng.normal(scale=0.4, size=(n, 3)) - o
    hit, t, exits = np.zeros(n, bool), np.zeros(n), np.zeros(n, bool)
    for s in range(0, n, blk):
        k = np.arange(blk)
        H, T, D = R.hit_matrix(v, f[s:s + blk], o[s:s + blk], d[s:s + blk])
        hit[s:s + blk], t[s:s + blk], exits[s:s + blk] = H[k, k], T[k, k], D[k, k] > 0
    got = shim.pairs(v, f, o, d)
    assert np.array_equal(got['hit'], hit) and np.array_equal(got['t'][hit], t[hit]) and np.array_equal(got['exits'][hit], exits[hit])
    assert 2000 < hit.sum() < 8000 and 0 < exits[hit].sum() < hit.sum()
