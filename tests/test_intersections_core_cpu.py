"""
The self-intersection check's arithmetic, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_intersections_core.h holds the pair
predicate as __host__ __device__ functions; this test compiles them for the CPU (g++ -ffp-contract=off) behind a shim of its own -- a
loop over a list of face pairs -- and asks for the booleans of the NumPy restatement (tests/mesh_intersections_ref.py) on a corpus of
pairs.  The shim is built on demand in pytest's temporary directory.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_intersections_ref as R
from conftest import ROOT

CORE = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_intersections_core.h')

SHIM = r'''
#include "nw_intersections_core.h"
extern "C" void shim_pairs(const float *pos, const int *faces, const long long *fa, const long long *fb, long long n, unsigned char *out)
{
    for (long long i = 0; i < n; ++i) {
        const long long lo = fa[i] < fb[i] ? fa[i] : fb[i], hi = fa[i] < fb[i] ? fb[i] : fa[i];
        out[i] = nwx_pair(nwx_load(pos, faces, lo), nwx_load(pos, faces, hi)) ? 1 : 0;
    }
}
extern "C" double shim_centroid(const float *pos, const int *faces, long long f, double *cen)
{
    nwx_v3 m;
    const double rho = nwx_face_centroid(nwx_load(pos, faces, f), &m);
    cen[0] = m.x; cen[1] = m.y; cen[2] = m.z;
    return rho;
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwx_shim')
    src, lib = os.path.join(str(d), 'shim.cpp'), os.path.join(str(d), 'libnwx_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', os.path.dirname(CORE),
                           '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    L.shim_pairs.argtypes = [vp, vp, vp, vp, ctypes.c_longlong, vp]
    L.shim_pairs.restype = None
    L.shim_centroid.argtypes = [vp, vp, ctypes.c_longlong, vp]
    L.shim_centroid.restype = ctypes.c_double

    def run(vertices, faces, fa, fb):
        v = np.ascontiguousarray(vertices, np.float32)
        f = np.ascontiguousarray(faces, np.int32)
        fa, fb = np.ascontiguousarray(fa, np.int64), np.ascontiguousarray(fb, np.int64)
        out = np.zeros(fa.size, np.uint8)
        L.shim_pairs(v.ctypes.data, f.ctypes.data, fa.ctypes.data, fb.ctypes.data, fa.size, out.ctypes.data)
        return out.astype(bool)

    def centroid(vertices, faces, k):
        v = np.ascontiguousarray(vertices, np.float32)
        f = np.ascontiguousarray(faces, np.int32)
        cen = np.empty(3)
        return L.shim_centroid(v.ctypes.data, f.ctypes.data, k, cen.ctypes.data), cen
    run.centroid = centroid
    return run


def same_on_all_pairs(shim, v, f, both_orders=True):
    fa, fb = np.triu_indices(len(f), 1)
    ref = R.pair_bits(v, f, fa, fb)
    assert np.array_equal(shim(v, f, fa, fb), ref)
    if both_orders:
        assert np.array_equal(shim(v, f, fb, fa), ref)                                    # the smaller id is A, whoever asks
    return int(ref.sum())


def test_the_hand_made_cases(shim):
    assert same_on_all_pairs(shim, *R.cube_and_plane()) == 8
    for name, (B, expected) in R.TWO_TRIANGLES.items():
        for tris in ((R.A_TRI, B), (B, R.A_TRI)):
            assert same_on_all_pairs(shim, *R.soup(*tris)) == expected, name
    for crossing in (True, False):
        for ra in range(3):
            for rb in range(3):
                assert same_on_all_pairs(shim, *R.shared_corner(crossing, ra, rb)) == int(crossing)
    from test_mesh_intersections_ref import TOUCHING_AT_AN_EDGE_MIDPOINT
    assert same_on_all_pairs(shim, TOUCHING_AT_AN_EDGE_MIDPOINT, [[0, 1, 2], [3, 4, 5]]) == 0


def test_the_meshes(shim):
    assert same_on_all_pairs(shim, *R.noisy_sphere(0.3)) == 700
    assert same_on_all_pairs(shim, *R.noisy_sphere(0.05)) == 0
    for radius, centre in ((1.0, 0.0), (100.0, 1e6)):
        v, f, _ = R.two_spheres(radius, centre)
        assert same_on_all_pairs(shim, v, f, False) == 78
    assert same_on_all_pairs(shim, *R.cushion()) == 190
    v, f, _ = R.with_flat_faces()
    assert same_on_all_pairs(shim, v, f, False) == 78
    assert same_on_all_pairs(shim, *R.sphere_and_oversize_face()) == R.self_intersections(*R.sphere_and_oversize_face())['n_pairs'] > 0


def random_pairs(n, seed, centre=0.0, scale=1.0, share=True):
    """n pairs of random triangles (faces 2i, 2i + 1) close enough to cross about half the time; with `share`, a third of them share
    one vertex id and a tenth two"""
    rng = np.random.default_rng(seed)
    v = (centre + scale * rng.normal(size=(6 * n, 3))).astype(np.float32)
    f = np.arange(6 * n, dtype=np.int32).reshape(-1, 3)
    if share:
        for i in range(n):
            u = rng.random()
            if u < 0.33:
                f[2 * i + 1, rng.integers(3)] = f[2 * i, rng.integers(3)]
            elif u < 0.43:
                ka, kb = rng.permutation(3)[:2], rng.permutation(3)[:2]
                f[2 * i + 1, kb] = f[2 * i, ka]
    return v, f, 2 * np.arange(n), 2 * np.arange(n) + 1


def test_ten_thousand_random_pairs(shim):
    v, f, fa, fb = random_pairs(10000, 21)
    ref = R.pair_bits(v, f, fa, fb)
    s = R.shared_corners(f, np.stack([fa, fb], axis=1))
    for k in (0, 1):
        assert 200 < ref[s == k].sum() < (s == k).sum() - 200                              # both answers, with and without a shared corner
    assert (s == 2).sum() > 500 and not ref[s >= 2].any()
    assert np.array_equal(shim(v, f, fa, fb), ref) and np.array_equal(shim(v, f, fb, fa), ref)


def test_pairs_a_million_from_the_origin(shim):
    v, f, fa, fb = random_pairs(4000, 22, centre=1e6, scale=2.0)
    assert np.spacing(np.abs(v).min()) == np.float32(0.0625)
    ref = R.pair_bits(v, f, fa, fb)
    assert 500 < ref.sum() < 3500
    assert np.array_equal(shim(v, f, fa, fb), ref)


def test_needles_of_aspect_ten_thousand(shim):
    rng = np.random.default_rng(23)
    n = 3000
    tris = []
    for i in range(2 * n):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        w = np.cross(u, rng.normal(size=3))
        w /= np.linalg.norm(w)
        c = rng.normal(scale=0.02, size=3)
        t = rng.uniform(-0.4, 0.4)
        tris.append(np.array([c - 50.0 * u, c + 50.0 * u, c + t * 50.0 * u + 0.01 * w]))
    v, f = R.soup(*tris)
    d = v.astype(np.float64)
    e = np.linalg.norm(d[f[:, 1]] - d[f[:, 0]], axis=1)
    area2 = np.linalg.norm(np.cross(d[f[:, 1]] - d[f[:, 0]], d[f[:, 2]] - d[f[:, 0]]), axis=1)
    assert (e / (area2 / e) > 5e3).all()                                                  # base over height
    fa, fb = 2 * np.arange(n), 2 * np.arange(n) + 1
    ref = R.pair_bits(v, f, fa, fb)
    assert 30 < ref.sum() < n - 30
    assert np.array_equal(shim(v, f, fa, fb), ref)


def test_piercing_point_approaching_an_edge(shim):
    """A's edge 0 -> 1 runs along the y axis through the origin, A lies at x < 0; a vertical segment pierces A's plane at
    (-+2^-k, 0, 0): a crossing on the inner side, none on the outer, for every k up to 50, in closed form"""
    A = np.array([[0, -1, 0], [0, 1, 0], [-2, 0, 0]], np.float64)
    tris, expected = [], []
    for k in range(1, 51):
        for sign in (-1.0, 1.0):
            x = sign * 2.0 ** -k
            tris += [A, np.array([[x, 0, -1], [x, 0, 1], [x + 3, 0.5, 1]])]
            expected.append(sign < 0)
    v, f = R.soup(*tris)
    assert np.array_equal(v.astype(np.float64)[3::6, 0], [s * 2.0 ** -k for k in range(1, 51) for s in (-1, 1)])
    fa, fb = 2 * np.arange(100), 2 * np.arange(100) + 1
    ref = R.pair_bits(v, f, fa, fb)
    assert np.array_equal(ref, expected)
    assert np.array_equal(shim(v, f, fa, fb), ref) and np.array_equal(shim(v, f, fb, fa), ref)


def test_centroid_radius_covers_the_face(shim):
    """rho_f, the bound the device's walk rests on: the same numbers as the distance unit's, and no point of a face farther out"""
    rng = np.random.default_rng(9)
    v, f, _, _ = random_pairs(50, 24, centre=10.0, scale=3.0, share=False)
    d = v.astype(np.float64)
    for k, face in enumerate(f):
        rho, cen = shim.centroid(v, f, k)
        assert np.array_equal(cen, ((d[face[0]] + d[face[1]]) + d[face[2]]) / 3.0)
        e = d[face] - cen
        assert rho == np.sqrt(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).max())
        pts = (rng.dirichlet([1, 1, 1], 50)[:, :, None] * d[face]).sum(1)
        assert np.linalg.norm(pts - cen, axis=1).max() <= rho * (1 + 1e-12)
