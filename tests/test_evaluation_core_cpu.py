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
