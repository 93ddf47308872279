"""
The point-to-mesh distance's arithmetic, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_distance_core.h holds the point-triangle
distance, the pseudonormals and the sign as __host__ __device__ functions; this test compiles them for the CPU (g++ -ffp-contract=off)
behind a shim of its own -- the brute-force loop over all faces, the smallest (d2, face id) -- and asks for the arrays of the NumPy
restatement (tests/mesh_distance_ref.py): d2, closest point, face and feature bit for bit, the sign wherever it is not a matter of
rounding.  The shim is built on demand in pytest's temporary directory.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_distance_ref as R
from conftest import ROOT
from ch_shrinkwrap_amd.trimesh import icosphere

CORE = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_distance_core.h')

SHIM = r'''
#include "nw_distance_core.h"
extern "C" void shim_distance(const float *pos, const int *faces, const int *twin, long long nf, const double *q, long long nq,
                              double *d2_out, double *dist_out, double *closest_out, int *face_out, int *feature_out, double *normal_out)
{
    for (long long i = 0; i < nq; ++i) {
        double best = INFINITY, bc[3] = {0, 0, 0};
        int bf = -1, bfeat = 0;
        for (long long f = 0; f < nf; ++f) {
            double c[3];
            int feat;
            const double d2 = nwd_point_triangle(q + 3 * i, pos + 3 * (long long)faces[3 * f], pos + 3 * (long long)faces[3 * f + 1],
                                                 pos + 3 * (long long)faces[3 * f + 2], c, &feat);
            if (d2 < best) { best = d2; bf = (int)f; bfeat = feat; bc[0] = c[0]; bc[1] = c[1]; bc[2] = c[2]; }
        }
        double d = sqrt(best), N[3] = {0, 0, 0};
        if (twin) {
            bfeat |= nwd_pseudonormal(pos, faces, twin, bf, bfeat, N);
            if (best > 0.0 && nwd_sign(q + 3 * i, bc, N) < 0.0) d = -d;
        }
        d2_out[i] = best; dist_out[i] = d; face_out[i] = bf; feature_out[i] = bfeat;
        for (int k = 0; k < 3; ++k) { closest_out[3 * i + k] = bc[k]; normal_out[3 * i + k] = N[k]; }
    }
}
extern "C" double shim_centroid(const float *a, const float *b, const float *c, double *cen) { return nwd_face_centroid(a, b, c, cen); }
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwd_shim')
    src, lib = os.path.join(str(d), 'shim.cpp'), os.path.join(str(d), 'libnwd_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', os.path.dirname(CORE),
                           '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    L.shim_distance.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, ctypes.c_longlong, vp, vp, vp, vp, vp, vp]
    L.shim_distance.restype = None
    L.shim_centroid.argtypes = [vp, vp, vp, vp]
    L.shim_centroid.restype = ctypes.c_double

    def run(vertices, faces, twin, queries):
        v = np.ascontiguousarray(vertices, np.float32)
        f = np.ascontiguousarray(faces, np.int32)
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, 3)
        t = None if twin is None else np.ascontiguousarray(twin, np.int32)
        n = q.shape[0]
        out = dict(d2=np.empty(n), dist=np.empty(n), closest=np.empty((n, 3)), face=np.empty(n, np.int32), feature=np.empty(n, np.int32),
                   normal=np.empty((n, 3)))
        L.shim_distance(v.ctypes.data, f.ctypes.data, None if t is None else t.ctypes.data, f.shape[0], q.ctypes.data, n,
                        *(out[k].ctypes.data for k in ('d2', 'dist', 'closest', 'face', 'feature', 'normal')))
        return out
    run.centroid = L.shim_centroid
    return run


def test_one_triangle_in_all_seven_regions(shim):
    v, f, q, code = R.triangle_region_queries()
    tw = R.twins(f)
    ref = R.distance(q, v, f, tw)
    mine = shim(v, f, tw, q)
    R.same_as_restatement(mine, ref, True)
    assert (mine['feature'] == code).all() and sorted(set(mine['feature'].tolist())) == list(range(7))
    # in the plane and beside the triangle the sign is a matter of rounding, and it is + by the rule (not below zero)
    assert (mine['dist'][np.asarray(q)[:, 2] == 0] >= 0).all()
    more = R.around(v, 500, 4, spread=3.0)
    assert R.same_as_restatement(shim(v, f, tw, more), R.distance(more, v, f, tw), True) > 400


def test_zero_length_edges_and_collinear_corners(shim):
    v, f = R.degenerate_faces()
    q = np.concatenate([R.around(v, 400, 5), [[2.5, 0.5, 0.0], [4.0, -1.0, 0.0], [2.0, 2.0, 2.5], [3.0, 0.0, 0.0], [2.0, 2.0, 2.0]]])
    ref = R.distance(q, v, f)
    mine = shim(v, f, None, q)
    R.same_as_restatement(mine, ref, False)
    zero_area = np.isin(mine['face'], [1, 2, 3, 4])
    assert zero_area.sum() > 100 and (mine['feature'][zero_area] != 0).all()              # never 'interior'
    assert np.isfinite(mine['d2']).all() and np.isfinite(mine['closest']).all()
    # with twins: zero-area faces add nothing to a pseudonormal, and nothing is nan
    tw = R.twins(f)
    ref, mine = R.distance(q, v, f, tw), shim(v, f, tw, q)
    R.same_as_restatement(mine, ref, True)
    assert np.isfinite(mine['normal']).all() and np.isfinite(mine['dist']).all()


def test_needles_of_aspect_ten_thousand(shim):
    v, f = R.needles()
    vd = v.astype(np.float64)
    e = np.linalg.norm(vd[f[:, 1]] - vd[f[:, 0]], axis=1)
    area2 = np.linalg.norm(np.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]]), axis=1)
    assert (e / (area2 / e) > 5e3).all()                                                  # base over height
    rng = np.random.default_rng(6)
    w = rng.dirichlet([1, 1, 1], 600)
    k = rng.integers(0, len(f), 600)
    on = (w[:, :, None] * vd[f[k]]).sum(1)                                                 # points of the needles, then lifted off them
    q = np.concatenate([on + rng.normal(scale=0.05, size=on.shape), on + rng.normal(scale=30.0, size=on.shape),
                        vd + rng.normal(scale=5.0, size=vd.shape)])                         # ... and around the needles' ends
    a, b, c = vd[f[:, 0]], vd[f[:, 1]], vd[f[:, 2]]
    u = (b - a) / np.linalg.norm(b - a, axis=1)[:, None]
    perp = (c - a) - ((c - a) * u).sum(1)[:, None] * u
    q = np.concatenate([q, c + 200.0 * perp])                                              # straight off the blunt corner of each
    tw = R.twins(f)
    ref, mine = R.distance(q, v, f, tw), shim(v, f, tw, q)
    assert R.same_as_restatement(mine, ref, True) > 1000
    assert len(set(mine['feature'].tolist())) == 7


def test_a_mesh_a_million_from_the_origin(shim):
    v, f = icosphere(2, 50.0)
    v = (v + np.float32(1e6)).astype(np.float32)
    assert np.spacing(v.min()) == np.float32(0.0625)
    q = R.around(v, 1200, 7)
    tw = R.twins(f)
    ref, mine = R.distance(q, v, f, tw), shim(v, f, tw, q)
    assert R.same_as_restatement(mine, ref, True) > 1000
    assert (mine['d2'][:8] == 0).all() and (mine['dist'] < 0).sum() > 100


@pytest.mark.parametrize('name', ['cube', 'spike', 'l_prism', 'disk'])
def test_core_equals_the_restatement_on_the_named_meshes(shim, name):
    v, f = getattr(R, name)()
    tw = R.twins(f)
    q = np.concatenate([R.around(v, 1000, 8), R.spike_queries(100) if name == 'spike' else np.zeros((1, 3))])
    taken = {}
    ref, mine = R.distance(q, v, f, tw, taken=taken), shim(v, f, tw, q)
    assert R.same_as_restatement(mine, ref, True) > 900
    if name == 'disk':
        assert taken.get('border', 0) > 50 and taken.get('border_edge', 0) > 50
    if name == 'cube':
        assert mine['face'][-1] == 0 and mine['d2'][-1] == 1.0                            # the centre: twelve faces tie, the smallest id wins
    if name == 'spike':
        assert (mine['dist'][-100:] > 0).all()


def test_capped_fan(shim):
    n = R.FAN_CAP + 40
    a = 2.0 * np.pi * np.arange(n) / n
    v = np.array([[0.0, 0.0, 1.0]] + [[np.cos(t), np.sin(t), 0.0] for t in a], np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    q = np.array([[0.0, 0.0, 3.0], [2.0, 0.0, 0.0], [0.1, 0.0, 2.0]])
    tw = R.twins(f)
    ref, mine = R.distance(q, v, f, tw), shim(v, f, tw, q)
    R.same_as_restatement(mine, ref, True)
    assert mine['feature'][0] == (4 | R.CAPPED)


def test_centroid_radius_covers_the_face(shim):
    """rho_f, the bound the device's walk rests on: no point of a face is farther from the centroid than its farthest corner"""
    rng = np.random.default_rng(9)
    for v, f in (R.needles(), R.degenerate_faces(), R.cube()):
        vd = v.astype(np.float64)
        for face in f:
            a, b, c = (np.ascontiguousarray(v[i]) for i in face)
            cen = np.empty(3)
            rho = shim.centroid(a.ctypes.data, b.ctypes.data, c.ctypes.data, cen.ctypes.data)
            assert np.array_equal(cen, ((vd[face[0]] + vd[face[1]]) + vd[face[2]]) / 3.0)
            assert rho == np.sqrt(((vd[face] - cen) ** 2).sum(1).max()) or np.isclose(rho, np.linalg.norm(vd[face] - cen, axis=1).max(), rtol=1e-15)
            pts = (rng.dirichlet([1, 1, 1], 50)[:, :, None] * vd[face]).sum(1)
            assert np.linalg.norm(pts - cen, axis=1).max() <= rho * (1 + 1e-12) + 1e-14 * np.abs(vd[face]).max()
