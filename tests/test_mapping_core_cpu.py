"""
The localization mapping, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_mapping_core.h holds the weights, the quantisation, the
limbs and the vertex areas as __host__ __device__ functions, over nw_volume_core.h's capped walk of a centroid grid handed in as arrays.
This test compiles them for the CPU (g++ -ffp-contract=off) behind a shim of its own -- the loop over the localizations with plain
integer adds where the device has atomics -- and asks for the restatement's (tests/surface_mapping_ref.py) face, weights, distance bits
and closest-point bits and its accumulators.  The grid is binned here in NumPy, at four cell sizes.  The same source with a main of its
own runs once under -fsanitize=address,undefined.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_distance_ref as D
import surface_mapping_ref as M
from ch_shrinkwrap_amd.trimesh import icosphere
from conftest import ROOT
from test_volume_core_cpu import centroid_grid, spanning_face

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nw_mapping_core.h"
// the cloud onto the accumulators as they are (the caller zeroes them, or hands in a previous call's) -> bit NWL_Q_NONFINITE or
// NWL_Q_RANGE for a value the definition refuses
extern "C" int shim_map(const float *pos, const int *faces, long long nf, const nwv_pt *pts, const int *cstart, const double *rho, double rho_max,
                        const double *glo, const double *ghi, double gh, const int *gdims, double d_cap, const double *xyz, long long n,
                        const double *values, int n_col, const double *scales, int *face, int *w, double *dist, double *closest,
                        unsigned long long *mass, int *count, long long *sum_hi, unsigned long long *sum_lo, long long *rings, long long *centroids)
{
    nwv_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = glo[d]; g.hi[d] = ghi[d]; g.dims[d] = gdims[d]; }
    g.h = gh;
    int flags = 0;
    for (long long i = 0; i < n; ++i) {
        nwl_hit h;
        int n_cen = 0;
        rings[i] = nwl_locate(xyz + 3 * i, pos, faces, (int)nf, pts, cstart, rho, rho_max, g, d_cap, h, n_cen);
        centroids[i] = n_cen;
        face[i] = h.face;
        dist[i] = h.d;
        for (int k = 0; k < 3; ++k) { w[3 * i + k] = h.w[k]; closest[3 * i + k] = h.c[k]; }
        if (h.face < 0) continue;
        count[h.face] += 1;
        for (int k = 0; k < 3; ++k) mass[faces[3 * (long long)h.face + k]] += (unsigned long long)h.w[k];
        for (int c = 0; c < n_col; ++c) {
            int64_t q;
            const int bad = nwl_quantise(values[i * n_col + c], scales[c], &q);
            if (bad) { flags |= 1 << bad; continue; }
            for (int k = 0; k < 3; ++k) {
                uint64_t lo;
                int64_t hi;
                nwl_limbs((int64_t)h.w[k] * q, &lo, &hi);
                const long long v = faces[3 * (long long)h.face + k];
                sum_lo[v * n_col + c] += lo;
                sum_hi[v * n_col + c] += hi;
            }
        }
    }
    return flags;
}

// -> the number of faces beyond the area limit
extern "C" long long shim_areas(const float *pos, const int *faces, long long nf, unsigned long long *area3)
{
    long long refused = 0;
    for (long long f = 0; f < nf; ++f) {
        uint64_t aq;
        if (!nwl_face_area(pos + 3 * (long long)faces[3 * f], pos + 3 * (long long)faces[3 * f + 1], pos + 3 * (long long)faces[3 * f + 2], &aq)) { ++refused; continue; }
        for (int k = 0; k < 3; ++k) area3[faces[3 * f + k]] += aq;
    }
    return refused;
}

extern "C" void shim_weights(const double *q, const float *tri, const int *feature, long long n, int *w)
{
    for (long long i = 0; i < n; ++i) nwl_weights(q + 3 * i, tri + 9 * i, tri + 9 * i + 3, tri + 9 * i + 6, feature[i], w + 3 * i);
}

#ifdef NWL_MAIN
// the same calls on arrays read from a file: <in> holds 6 int64 counts (nv, nf, npts, ncells, n, n_col), then the arrays
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 6);
    const auto pos = rd<float>(fh, 3 * c[0]);
    const auto faces = rd<int>(fh, 3 * c[1]);
    const auto pts = rd<nwv_pt>(fh, c[2]);
    const auto cstart = rd<int>(fh, c[3] + 1);
    const auto rho = rd<double>(fh, c[1]);
    const auto dbl = rd<double>(fh, 9);                       // rho_max, glo[3], ghi[3], gh, d_cap
    const auto gdims = rd<int>(fh, 3);
    const auto xyz = rd<double>(fh, 3 * c[4]);
    const auto values = rd<double>(fh, c[4] * c[5]);
    const auto scales = rd<double>(fh, c[5]);
    fclose(fh);
    const size_t nv = (size_t)c[0], nf = (size_t)c[1], n = (size_t)c[4], nc = (size_t)c[5];
    std::vector<int> face(n), w(3 * n), count(nf);
    std::vector<double> dist(n), closest(3 * n);
    std::vector<unsigned long long> mass(nv), sum_lo(nv * nc), area3(nv);
    std::vector<long long> sum_hi(nv * nc), rings(n), cen(n);
    const int flags = shim_map(pos.data(), faces.data(), c[1], pts.data(), cstart.data(), rho.data(), dbl[0], &dbl[1], &dbl[4], dbl[7], gdims.data(), dbl[8],
                               xyz.data(), c[4], values.data(), (int)c[5], scales.data(), face.data(), w.data(), dist.data(), closest.data(), mass.data(),
                               count.data(), sum_hi.data(), sum_lo.data(), rings.data(), cen.data());
    const long long refused = shim_areas(pos.data(), faces.data(), c[1], area3.data());
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(dist.data(), sizeof(double), n, fh);
    fwrite(mass.data(), sizeof(unsigned long long), nv, fh);
    fwrite(sum_hi.data(), sizeof(long long), nv * nc, fh);
    fwrite(sum_lo.data(), sizeof(unsigned long long), nv * nc, fh);
    fwrite(area3.data(), sizeof(unsigned long long), nv, fh);
    fwrite(w.data(), sizeof(int), 3 * n, fh);
    fclose(fh);
    return (flags || refused) ? 1 : 0;
}
#endif
'''


def _source(tmp):
    src = os.path.join(str(tmp), 'shim.cpp')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    return src


p = lambda a: a.ctypes.data


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwl_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwl_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f64, ll, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_longlong, ctypes.c_int
    L.shim_map.argtypes = [vp, vp, ll, vp, vp, vp, f64, vp, vp, f64, vp, f64, vp, ll, vp, i32, vp] + [vp] * 10
    L.shim_map.restype = i32
    L.shim_areas.argtypes = [vp, vp, ll, vp]
    L.shim_areas.restype = ll
    L.shim_weights.argtypes = [vp, vp, vp, ll, vp]
    L.shim_weights.restype = None
    return L


def shim_map(lib, v, f, pts_xyz, band, h_cell, values=None, scales=None, onto=None):
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    xyz = np.ascontiguousarray(pts_xyz, np.float64).reshape(-1, 3)
    n, V, F = len(xyz), len(v), len(f)
    vals = np.zeros((n, 0)) if values is None else np.ascontiguousarray(values, np.float64).reshape(n, -1)
    C = vals.shape[1]
    sc = np.ascontiguousarray(scales if C else [], np.float64)
    pts, cstart, rho, rho_max, glo, ghi, gdims = centroid_grid(v, f, h_cell)
    out = dict(face=np.empty(n, np.int32), weights=np.empty((n, 3), np.int32), distance=np.empty(n), closest=np.empty((n, 3)),
               rings=np.empty(n, np.int64), centroids=np.empty(n, np.int64))
    if onto is None:
        out.update(mass=np.zeros(V, np.uint64), count=np.zeros(F, np.int32), sum_hi=np.zeros((V, C), np.int64), sum_lo=np.zeros((V, C), np.uint64))
    else:
        out.update({k: onto[k].copy() for k in ('mass', 'count', 'sum_hi', 'sum_lo')})
    out['flags'] = lib.shim_map(p(v), p(f), F, p(pts), p(cstart), p(rho), rho_max, p(glo), p(ghi), float(h_cell), p(gdims), float(band), p(xyz), n,
                                p(vals), C, p(sc), *(p(out[k]) for k in ('face', 'weights', 'distance', 'closest', 'mass', 'count', 'sum_hi', 'sum_lo',
                                                                         'rings', 'centroids')))
    out['blob'] = (v, f, pts, cstart, rho, rho_max, glo, ghi, gdims, xyz, vals, sc)
    return out


def shim_areas(lib, v, f):
    v, f = np.ascontiguousarray(v, np.float32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    a3 = np.zeros(len(v), np.uint64)
    return a3, lib.shim_areas(p(v), p(f), len(f), p(a3))


def columns(n, seed):
    """three value columns and their scales: a wide signed one, a 0 / 1 flag, zeros"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-900.0, 5000.0, n), rng.integers(0, 2, n).astype(np.float64), np.zeros(n)], 1), np.array([8192.0, 1.0, 1.0])


def check(lib, v, f, pts, band, cells, with_values=True):
    vals, scales = columns(len(pts), 4) if with_values else (None, None)
    ref = M.map_cloud(pts, v, f, band, vals, scales)
    for h_cell in cells:
        mine = shim_map(lib, v, f, pts, band, h_cell, vals, scales)
        assert mine['flags'] == 0
        M.same_as_restatement(mine, ref)
    a3, refused = shim_areas(lib, v, f)
    assert refused == 0 and np.array_equal(a3, M.vertex_areas(v, f))
    return ref, mine


def test_the_cube_at_four_cell_sizes_and_in_chunks(lib):
    v, f = D.cube()
    pts = M.cloud_around(v, 700, 5, spread=1.6)
    ref, mine = check(lib, v, f, pts, 0.6, (0.3, 0.7, 1.1, 9.0))
    assert 100 < ref['n_in_band'] < len(pts) and int(ref['mass'].sum()) == ref['n_in_band'] * M.W_ONE
    vals, scales = columns(len(pts), 4)
    acc = None
    for s, e in ((0, 1), (1, 300), (300, len(pts))):
        acc = shim_map(lib, v, f, pts[s:e], 0.6, 0.7, vals[s:e], scales, onto=acc)
    M.same_accumulators(acc, ref)


def test_the_closed_forms_of_the_weights(lib):
    v, f = M.right_triangle()
    pts = np.array([[-1, -1, 1], [5, -1, -2], [-0.5, 4, 0], [1.5, -1, 0.5], [2, 2, 1], [-2, 1.5, 0], [0.75, -1, 0], [1, 1, 5], [0.75, 1.5, 2]], np.float64)
    mine = shim_map(lib, v, f, pts, 10.0, 1.0)
    W = M.W_ONE
    assert mine['weights'].tolist() == [[W, 0, 0], [0, W, 0], [0, 0, W], [W // 2, W // 2, 0], [0, W // 2, W // 2], [W // 2, 0, W // 2],
                                        [3 * W // 4, W // 4, 0], [349525, 349525, 349526], [W // 4, W // 4, W // 2]]
    # a closest point a hair outside its face (negative edge functions are raised to 0) and a face without area asked as an interior
    tri = np.array([[[0, 0, 0], [3, 0, 0], [0, 3, 0]], [[1, 1, 1], [1, 1, 1], [1, 1, 1]]], np.float32)
    q = np.array([[-1e-9, 1.0, 0.0], [1.0, 1.0, 1.0]])
    w = np.empty((2, 3), np.int32)
    lib.shim_weights(p(q), p(tri), p(np.zeros(2, np.int32)), 2, p(w))
    ref = M.weights(q, *(tri[:, k].astype(np.float64) for k in range(3)), np.zeros(2, np.int32))
    assert np.array_equal(w, ref) and w[1].tolist() == [W, 0, 0] and w[0].sum() == W and w[0, 1] == 0


def test_the_seven_regions_of_a_triangle_and_the_band_edge(lib):
    v, f, q, code = D.triangle_region_queries()
    ref, _ = check(lib, v, f, q, 10.0, (0.5, 1.0, 3.0, 20.0))
    assert ref['n_in_band'] == len(q)
    for i in (0, 3, 12):                                                              # interior, edge and vertex regions, off the plane
        d = float(ref['distance'][i])
        assert d > 0
        for h_cell in (0.5, 20.0):
            assert shim_map(lib, v, f, q[i:i + 1], d, h_cell)['face'][0] == 0
            out = shim_map(lib, v, f, q[i:i + 1], np.nextafter(d, 0.0), h_cell)
            assert out['face'][0] == -1 and np.isinf(out['distance'][0]) and np.isnan(out['closest']).all() and not out['mass'].any()


def test_faces_without_area_and_needles(lib):
    v, f = D.degenerate_faces()
    ref, _ = check(lib, v, f, M.cloud_around(v, 300, 8), 0.8, (0.4, 1.0, 2.5, 30.0))
    assert 30 < ref['n_in_band'] < 300 and len(set(ref['face'][ref['in_band']].tolist())) >= 4
    v, f = D.needles()
    pts = np.concatenate([M.cloud_around(v, 150, 6, spread=1.1), v[f[:, 0]].astype(np.float64) + 0.3, (v[f[:, 0]].astype(np.float64) + v[f[:, 1]]) / 2 + 0.2])
    ref, _ = check(lib, v, f, pts, 40.0, (30.0, 90.0, 400.0, 5000.0))
    assert 60 < ref['n_in_band'] < len(pts)


def test_a_mesh_a_million_from_the_origin_and_a_face_spanning_three_times_the_mesh(lib):
    v, f = icosphere(1, 50.0)
    v = (v + np.float32(1e6)).astype(np.float32)
    pts = M.sphere_points(300, 55.0, 3, jitter=12.0) + 1e6
    ref, _ = check(lib, v, f, pts, 10.0, (8.0, 20.0, 45.0, 500.0))
    assert 50 < ref['n_in_band'] < 300
    v, f = spanning_face()
    pts = np.concatenate([M.sphere_points(150, 10.0, 4, jitter=1.5), np.random.default_rng(1).uniform([-28, -28, 12.5], [28, 28, 15.5], (150, 3))])
    ref, _ = check(lib, v, f, pts, 1.0, (1.5, 4.0, 11.0, 120.0))
    big = ref['face'] == len(f) - 1
    assert big.sum() > 15 and (ref['face'] >= 0).sum() > big.sum() + 40 and (ref['face'] == -1).sum() > 20


def test_values_beyond_the_scale_and_the_plus_and_minus_scale_columns(lib):
    v, f = D.cube()
    pts = M.cloud_around(v, 400, 5, spread=1.6)
    vals = np.stack([np.full(len(pts), 64.0), np.full(len(pts), -64.0)], 1)
    ref = M.map_cloud(pts, v, f, 0.6, vals, [64.0, 64.0])
    mine = shim_map(lib, v, f, pts, 0.6, 0.7, vals, [64.0, 64.0])
    M.same_as_restatement(mine, ref)
    total = M.column_sums(mine['sum_hi'], mine['sum_lo'])
    assert (total[:, 0] == mine['mass'].astype(object) * M.Q_ONE).all() and (total[:, 1] == -total[:, 0]).all()
    far, near = int(np.flatnonzero(~ref['in_band'])[0]), int(np.flatnonzero(ref['in_band'])[0])
    vals[far] = [96.0, np.nan]
    out = shim_map(lib, v, f, pts, 0.6, 0.7, vals, [64.0, 64.0])
    assert out['flags'] == 0
    M.same_accumulators(out, ref)
    vals[near, 0] = 96.0
    assert shim_map(lib, v, f, pts, 0.6, 0.7, vals, [64.0, 64.0])['flags'] == 1 << 2
    vals[near] = [64.0, np.inf]
    assert shim_map(lib, v, f, pts, 0.6, 0.7, vals, [64.0, 64.0])['flags'] == 1 << 1


def test_a_face_of_area_two_to_the_forty_is_refused(lib):
    a3, refused = shim_areas(lib, np.array([[0, 0, 0], [2.0 ** 21, 0, 0], [0, 2.0 ** 20, 0]], np.float32), [[0, 1, 2]])
    assert refused == 1 and not a3.any()                                              # exactly 2^40
    a3, refused = shim_areas(lib, np.array([[0, 0, 0], [2.0 ** 21, 0, 0], [0, 2.0 ** 20 - 0.0625, 0]], np.float32), [[0, 1, 2]])
    assert refused == 0 and int(a3[0]) == (2 ** 40 - 2 ** 16) * 2 ** 20               # (2^21 (2^20 - 2^-4) / 2) 2^20, exact


def test_a_main_of_its_own_under_the_sanitizers(lib, tmp_path):
    cxx = os.environ.get('CXX', 'g++')
    exe = os.path.join(str(tmp_path), 'nwl_main')
    flags = ['-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    # whether the compiler has the sanitizers' runtimes is asked of a program of one line; the shim's own compile errors fail the test
    probe = os.path.join(str(tmp_path), 'probe.cpp')
    with open(probe, 'w') as fh:
        fh.write('int main() { return 0; }\n')
    if subprocess.run([cxx] + flags + ['-o', os.path.join(str(tmp_path), 'probe'), probe], capture_output=True, text=True).returncode != 0:
        pytest.skip('the compiler has no sanitizer runtime')
    r = subprocess.run([cxx] + flags + ['-DNWL_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    v, f = D.degenerate_faces()
    pts = M.cloud_around(v, 300, 8)
    vals, scales = columns(len(pts), 4)
    mine = shim_map(lib, v, f, pts, 0.8, 1.0, vals, scales)
    v, f, gpts, cstart, rho, rho_max, glo, ghi, gdims, xyz, vals, sc = mine['blob']
    src, dst = os.path.join(str(tmp_path), 'in.bin'), os.path.join(str(tmp_path), 'out.bin')
    with open(src, 'wb') as fh:
        fh.write(np.array([len(v), len(f), len(gpts), len(cstart) - 1, len(xyz), vals.shape[1]], np.int64).tobytes())
        for a in (v, f, gpts, cstart, rho, np.array([rho_max] + glo.tolist() + ghi.tolist() + [1.0, 0.8]), gdims, xyz, vals, sc):
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(dst, 'rb').read()
    n, V, C = len(xyz), len(v), vals.shape[1]
    o = 0
    for a in (mine['distance'], mine['mass'], mine['sum_hi'], mine['sum_lo'], shim_areas(lib, v, f)[0], mine['weights']):
        assert raw[o:o + a.nbytes] == np.ascontiguousarray(a).tobytes()
        o += a.nbytes
    assert o == len(raw) and (n, V, C) == (300, 7, 3)
