"""
The mesh sampler's arithmetic, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_evaluation_core.h holds the per-face set-up and the
node test of nwe_sample_mesh as __host__ __device__ functions; this test compiles them for the CPU (g++ -ffp-contract=off) into a shim
of its own -- count per face, test every node, emit: the kernels' passes as two loops -- and asks for the arrays of
evaluation.points_from_mesh(p=1), bit for bit and in the same order.  The shim is built on demand in pytest's temporary directory.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden, ROOT
from ch_shrinkwrap_amd import evaluation as E
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere

CORE = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_evaluation_core.h')

SHIM = r'''
#include "nw_evaluation_core.h"
extern "C" long long shim_sample(const float *pos, const int *faces, long long nf, double dx, double *out, int *face_out, long long cap)
{
    long long n = 0;
    for (long long f = 0; f < nf; ++f) {
        nwe_face_setup s;
        if (!nwe_setup_face(pos + 3 * (long long)faces[3 * f], pos + 3 * (long long)faces[3 * f + 1], pos + 3 * (long long)faces[3 * f + 2], dx, &s)) continue;
        const long long nodes = (long long)s.nx * s.ny;
        for (long long k = 0; k < nodes; ++k) {
            double X, Y;
            if (!nwe_node_inside(&s, k, dx, &X, &Y)) continue;
            if (out && n < cap) { nwe_node_position(&s, X, Y, out + 3 * n); face_out[n] = (int)f; }
            ++n;
        }
    }
    return n;
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwe_shim')
    src, lib = os.path.join(str(d), 'shim.cpp'), os.path.join(str(d), 'libnwe_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-I', os.path.dirname(CORE),
                           '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp = ctypes.c_void_p
    L.shim_sample.argtypes = [vp, vp, ctypes.c_longlong, ctypes.c_double, vp, vp, ctypes.c_longlong]
    L.shim_sample.restype = ctypes.c_longlong

    def sample(vertices, faces, dx):
        v = np.ascontiguousarray(vertices, np.float32)
        f = np.ascontiguousarray(faces, np.int32)
        n = L.shim_sample(v.ctypes.data, f.ctypes.data, f.shape[0], float(dx), None, None, 0)
        out, fid = np.empty((n, 3), np.float64), np.empty(n, np.int32)
        assert L.shim_sample(v.ctypes.data, f.ctypes.data, f.shape[0], float(dx), out.ctypes.data, fid.ctypes.data, n) == n
        return out, fid
    return sample


def _triangles(rng, n, length, width, centre_range):
    """n separate triangles (3 n vertices) in random orientations: a base of `length`, an apex `width` above a random point of it;
    the corner each face starts from is random too."""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1)[:, None]
    p0 = rng.uniform(-centre_range, centre_range, (n, 3))
    tri = np.stack([p0, p0 + length * u, p0 + rng.uniform(0.2, 0.8, (n, 1)) * length * u + width * w], 1)       # (n, 3, 3)
    roll = rng.integers(0, 3, n)
    tri = tri[np.arange(n)[:, None], (np.arange(3)[None, :] + roll[:, None]) % 3]
    return tri.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def edge_mesh(name):
    """Meshes at the sampler's edges -> [(vertices, faces, dx), ...]; tests/test_hip_evaluation_edges.py runs the same ones on the device.
    The grid of a face starts dx / 2 before its lower corner, so every face of non-zero area has a node, however small it is: the
    faces without nodes of `mostly_empty` are faces of zero area."""
    rng = np.random.default_rng(29)
    if name == 'mostly_empty':
        # icosphere(5, 10.0): 20 480 faces with edges below 1, so at dx = 4 one node each and hardly a sample; all but three windows of
        # them are collapsed onto an edge (no node).  Three large triangles: the first face, one in the middle, one before the last run.
        v, f = icosphere(5, 10.0)
        f = f.copy()
        keep = np.zeros(len(f), bool)
        for a, b in ((3000, 3400), (11000, 11500), (15000, 15600)):
            keep[a:b] = True
        f[~keep, 2] = f[~keep, 1]
        bv, bf = _triangles(rng, 3, 60.0, 50.0, 20.0)
        bf = bf + len(v)
        return [(np.concatenate([v, bv]), np.concatenate([bf[:1], f[:10240], bf[1:2], f[10240:18000], bf[2:], f[18000:]]), 4.0)]
    if name == 'needles':
        # aspect ratio 10^4.  At dx = 0.5 a face 0.1 wide has one or two rows of 2 000 nodes, the first 0.25 below it, and seldom a
        # sample; the first 100 again at dx = 0.15, where a row of nodes lies inside
        v, f = _triangles(rng, 500, 1000.0, 0.1, 2000.0)
        return [(v, f, 0.5), (v, f[:100], 0.15)]
    if name == 'skew':
        v, f = _triangles(rng, 3001, 2.0, np.sqrt(3.0), 1000.0)
        k = 1500
        c = v[3 * k]
        v[3 * k:3 * k + 3] = c + 1000.0 * (v[3 * k:3 * k + 3] - c)                  # side 2000
        return [(v, f, 1.0)]
    if name == 'far_off_origin':
        v, f = icosphere(4, 50.0)
        return [((v + np.float32(1e6)).astype(np.float32), f, 2.0)]
    raise KeyError(name)


EDGE_MESHES = ['mostly_empty', 'needles', 'skew', 'far_off_origin']


def edge_mesh_premise(name, runs):
    """what each edge mesh is there for, from the host's per-face node counts; -> those counts, one array per run"""
    counts = [E.node_counts(TriMesh(v, f), dx) for v, f, dx in runs]
    c = counts[0]
    if name == 'mostly_empty':
        assert (c == 0).mean() > 0.9 and c[0] > 100 and c[-1] == 0
        empty_run = np.diff(np.flatnonzero(np.concatenate([[1], c, [1]]))) - 1      # lengths of the runs of faces without nodes
        assert empty_run.max() > 2048 and len(c) - 1 - np.flatnonzero(c)[-1] > 2048    # ... longer than a tile of the scan, the last one too
    if name == 'needles':
        assert ((c >= 1900) & (c <= 4100)).all()                                    # one or two rows (or columns) of 2 000
    if name == 'skew':
        assert c.max() > 0.99 * c.sum() and np.argmax(c) == 1500
    if name == 'far_off_origin':
        v = runs[0][0]
        assert np.spacing(v.min()) == np.float32(0.0625) and np.spacing(v.max()) == np.float32(0.0625)
    return counts


def _same(shim, v, f, dx):
    host = E.points_from_mesh(TriMesh(v, f), dx_min=dx, p=1.0)
    mine, fid = shim(v, f, dx)
    assert host.dtype == np.float64 and mine.shape == host.shape
    assert np.array_equal(mine.view(np.uint64), host.view(np.uint64))            # bit for bit, in the host function's order
    assert (np.diff(fid) >= 0).all() and (fid >= 0).all() and (fid < len(f)).all()
    return host, fid


@pytest.mark.parametrize('name,spacings', [('fit_quality', (5.0, 11.0)), ('evaluation_case', (3.0, 7.5))])
def test_core_equals_the_host_function_on_the_golden_meshes(shim, name, spacings):
    g = load_golden(name)
    for dx in spacings:
        host, _ = _same(shim, g['vertices'], g['faces'], dx)
        assert host.shape[0] > 100


def test_core_equals_the_host_function_off_the_origin(shim):
    v, f = icosphere(6, 300.0)
    v = (v + np.array([5000.0, -3000.0, 800.0], 'f4')).astype('f4')
    host, fid = _same(shim, v, f, 5.0)
    assert host.shape[0] > 40000 and np.unique(fid).size > 0.5 * len(f)


def test_zero_area_faces_are_left_out(shim):
    v, f = icosphere(3, 100.0)
    f = f.copy()
    f[7] = [f[7, 0], f[7, 1], f[7, 1]]                         # an edge
    f[100] = [f[100, 2], f[100, 2], f[100, 2]]                 # a point
    host, fid = _same(shim, v, f, 3.0)
    assert 7 not in fid and 100 not in fid and host.shape[0] > 1000


@pytest.mark.parametrize('name', EDGE_MESHES)
def test_core_equals_the_host_function_on_the_edge_meshes(shim, name):
    runs = edge_mesh(name)
    counts = edge_mesh_premise(name, runs)
    total = 0
    for (v, f, dx), c in zip(runs, counts):
        host, fid = _same(shim, v, f, dx)
        assert (c[fid] > 0).all()                              # (no sample names a face without nodes)
        total += host.shape[0]
    print('%s: %s nodes, %d samples' % (name, [int(c.sum()) for c in counts], total))
    assert total > 100
