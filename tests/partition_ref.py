"""
The host restatement of the query's k-d work list (ch_shrinkwrap_amd/csrc/nw_partition_core.h: partition_host) as a stand-alone program:
built with g++ (no HIP header on the include path), run as a child process on one input file, read back with numpy.  Shared by
tests/test_partition_core_cpu.py (the rules, plain and under sanitizers) and tests/test_hip_partition.py (the device partition against it).
"""
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')
HEADER = os.path.join(CSRC, 'nw_partition_core.h')
CXX = os.environ.get('CXX', 'g++')

PROGRAM = r'''
#include "nw_partition_core.h"
#include <cstdio>
#include <cstdlib>

template <class T> static void rd(FILE *fh, T *p, size_t n) { if (n && fread(p, sizeof(T), n, fh) != n) { fprintf(stderr, "short input\n"); exit(2); } }
template <class T> static void wr(FILE *fh, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, fh) != n) { fprintf(stderr, "short output\n"); exit(2); } }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    int hdr[4];
    float w;
    rd(in, hdr, 4); rd(in, &w, 1);
    const int n = hdr[0], leaf = hdr[1], cap = hdr[2], sort_max = hdr[3];
    std::vector<uint32_t> key((size_t)n);
    std::vector<float> foot(4 * (size_t)n);
    std::vector<int> face((size_t)n);
    rd(in, key.data(), key.size()); rd(in, foot.data(), foot.size()); rd(in, face.data(), face.size());
    fclose(in);
    const nwp::HostResult a = nwp::partition_host(n, key.data(), foot.data(), face.data(), leaf, cap, w, sort_max);
    const nwp::HostResult b = nwp::partition_host(n, key.data(), foot.data(), face.data(), leaf, cap, w, sort_max);
    if (a.order != b.order || a.seg_start != b.seg_start || a.leaf_start != b.leaf_start || a.level != b.level) { fprintf(stderr, "two runs differ\n"); return 3; }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    const int res[3] = {a.level, (int)a.seg_start.size() - 1, (int)a.leaf_start.size() - 1};
    wr(out, res, 3); wr(out, a.order.data(), a.order.size()); wr(out, a.seg_start.data(), a.seg_start.size()); wr(out, a.leaf_start.data(), a.leaf_start.size());
    fclose(out);
    return 0;
}
'''


def build(d, flags=()):
    """-> path of the program, built in directory d with the extra flags"""
    src, exe = os.path.join(d, 'partition.cpp'), os.path.join(d, 'partition')
    with open(src, 'w') as fh:
        fh.write(PROGRAM)
    subprocess.check_call([CXX, '-O1', '-g', '-std=c++14', '-Wall', '-Werror'] + list(flags) + ['-I', CSRC, '-o', exe, src])
    return exe


def run(exe, d, key, foot, face, leaf, cap, w, sort_max=1024):
    """-> (level, order, seg_start, leaf_start) of the restatement; stderr must be clean of sanitizer reports"""
    key, foot, face = np.ascontiguousarray(key, np.uint32), np.ascontiguousarray(foot, np.float32), np.ascontiguousarray(face, np.int32)
    n = len(key)
    assert foot.shape == (n, 4) and face.shape == (n,)
    fin, fout = os.path.join(d, 'in.bin'), os.path.join(d, 'out.bin')
    with open(fin, 'wb') as fh:
        fh.write(np.array([n, leaf, cap, sort_max], np.int32).tobytes() + np.float32(w).tobytes() + key.tobytes() + foot.tobytes() + face.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    for report in ('AddressSanitizer', 'LeakSanitizer', 'runtime error'):
        assert report not in r.stderr, r.stderr[-4000:]
    out = np.fromfile(fout, np.int32)
    level, nsegs, nleaves = (int(x) for x in out[:3])
    assert len(out) == 3 + n + nsegs + 1 + nleaves + 1
    order = out[3:3 + n]
    seg_start = out[3 + n:3 + n + nsegs + 1]
    leaf_start = out[3 + n + nsegs + 1:]
    return level, order, seg_start, leaf_start


def morton_keys(xyz, lo, unit):
    """30-bit Morton keys of points, 10 bits an axis (x lowest), as the library's second sort builds them"""
    q = np.clip(((np.asarray(xyz, np.float32) - np.float32(lo)) * np.float32(1.0 / unit)).astype(np.int64), 0, 1023)
    key = np.zeros(len(q), np.uint32)
    for b in range(10):
        for a in range(3):
            key |= (((q[:, a] >> b) & 1) << (3 * b + a)).astype(np.uint32)
    return key


# ---- reading the layout of a solver (developer aids of nw_debug) ------------------------------------------------------------------------
def layout(cg):
    """-> (perm: sorted slot -> the caller's index, {leaves, segments, level, leaf, w} of the k-d list, items (p0, n) of the query's list)"""
    import ctypes
    vp = ctypes.c_void_p
    n = ctypes.c_int(0)
    N = cg._points_f32.shape[0]
    perm, kd = np.empty(N, np.int32), np.zeros(5, np.int32)
    cg._native.check(cg._L.nw_debug(cg._h, 4, perm.ctypes.data_as(vp), kd.ctypes.data_as(vp), N, ctypes.byref(n)))
    assert n.value == N
    cap = N + 1024
    items = np.zeros((cap, 2), np.int32)
    cg._native.check(cg._L.nw_debug(cg._h, 1, items.ctypes.data_as(vp), None, cap, ctypes.byref(n)))
    info = dict(leaves=int(kd[0]), segments=int(kd[1]), level=int(kd[2]), leaf=int(kd[3]), w=float(kd[4:5].view(np.float32)[0]))
    return perm, info, items[:n.value].copy()


def partition_inputs(cg):
    """with NW_KD_KEEP set: what the second sort's k-d partition was given, in key order -> (key, foot (n, 4), face, the caller's index)"""
    import ctypes
    vp = ctypes.c_void_p
    n = ctypes.c_int(0)
    N = cg._points_f32.shape[0]
    key, foot, face, perm = np.empty(N, np.uint32), np.empty((N, 4), np.float32), np.empty(N, np.int32), np.empty(N, np.int32)
    cg._native.check(cg._L.nw_debug(cg._h, 5, key.ctypes.data_as(vp), foot.ctypes.data_as(vp), N, ctypes.byref(n)))
    assert n.value == N, 'the partition did not run, or NW_KD_KEEP was not set'
    cg._native.check(cg._L.nw_debug(cg._h, 6, face.ctypes.data_as(vp), perm.ctypes.data_as(vp), N, ctypes.byref(n)))
    return key, foot, face, perm


# ---- C1's shape with what the exactness test needs ---------------------------------------------------------------------------------------
DUPLICATED = [100, 2000, 4000]      # faces handed over twice: both copies have the same centroid wherever the mesh goes, every time


def c1_scene():
    """10 000 localizations around the subdivision-4 icosphere; one of them masked (zero weights: the library refuses a
    non-finite localization or residual target outright, status -5 / NaN); three faces listed twice (so whoever is nearest to
    one of them is exactly equidistant from two centroids), and two localizations put right over two of those faces"""
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    from ch_shrinkwrap_amd.synth import sphere_cloud
    v, f = icosphere(4, 120.0)
    base = TriMesh(v.copy(), f)
    nrm, nbr = np.ascontiguousarray(base.vertex_normals, 'f4'), base.neighbor_vertex_table()
    faces = np.ascontiguousarray(np.concatenate([f, f[DUPLICATED]]), 'i4')
    pts = sphere_cloud(10000, 100.0, 10.0, seed=7)
    for i, k in ((10, DUPLICATED[0]), (11, DUPLICATED[1])):
        c = v[f[k]].mean(0)
        pts[i] = c * (100.0 / np.linalg.norm(c))
    pts = np.ascontiguousarray(pts, 'f4')
    weights = np.ones(pts.size, 'f4')
    weights[3 * 1234:3 * 1235] = 0.0
    return v, nrm, nbr, faces, pts, weights


def run_c1():
    """block, optimize_layout, block -> what the exactness test looks at"""
    from ch_shrinkwrap_amd.parallel import ArrayMesh
    from ch_shrinkwrap_amd.mesh_conj_grad import ShrinkwrapMeshConjGrad
    v, nrm, nbr, faces, pts, weights = c1_scene()
    mesh = ArrayMesh(v.copy(), nrm, nbr, faces, np.ones(v.shape[0], np.uint8))
    cg = ShrinkwrapMeshConjGrad(mesh, pts)
    out1 = cg.search(pts, lams=[10.0], num_iters=3, sigma_inv=0.1, weights=weights).copy()
    cg.optimize_layout()
    face = cg.nearest_face.copy()
    perm, info, items = layout(cg)
    out2 = cg.search(pts, lams=[10.0], num_iters=3, sigma_inv=0.1, weights=weights).copy()
    return dict(out1=out1, face=face, out2=out2, perm=perm, items=items, kd=np.array([info['leaves'], info['segments'], info['level'], info['leaf']]))


if __name__ == '__main__':
    import sys
    np.savez(sys.argv[1], **run_c1())
