"""
The DBSCAN query, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_clustering_core.h holds near, the ring walk, the guard of the two
shortcuts and the three visitors as __host__ __device__ functions over a cell grid handed in as arrays.  This test compiles them for the
CPU (g++ -ffp-contract=off) behind a shim of its own -- the device's passes in the device's order, with a sequential union where the
device has its lock-free one -- and asks for the restatement's (tests/dbscan_ref.py) labels, anchors, counts and core flags bit for bit.
The grid is binned here in NumPy with float32 cell indices, at four cell sizes: two small enough for the shortcuts, two that forbid
them; the counters say that each shortcut fired in the first and neither in the others.  The same source with a main of its own runs
once under -fsanitize=address,undefined.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dbscan_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <vector>
#include "nw_clustering_core.h"

struct seq_union {
    int *parent;
    int find(int v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; }
    void unite(int f, int g) { const int a = find(f), b = find(g); if (a != b) parent[a > b ? a : b] = a > b ? b : a; }
};

// pts in cell order, cells[3 q ..] = the cell of pts[q], cstart the cells' starts; counters: tests of the count, shortcut (a), tests of the
// unions, shortcut (b), tests of the border rule, the guard -> the number of clusters
extern "C" int shim_dbscan(const nwp_pt *pts, const int *cells, const int *cstart, const int *dims, double h, long long n, double eps, long long min_points,
                           long long count_cap, int shortcuts_on, int *label, int *anchor, int *count, unsigned char *core, long long *counters)
{
    if (!nwp_args_ok(eps, min_points, count_cap)) return -1;
    const double eps2 = eps * eps;
    const int cap = (int)count_cap;
    const int sc = (shortcuts_on && nwp_shortcuts_ok(h, eps)) ? 1 : 0;
    const long long ncell = (long long)dims[0] * dims[1] * dims[2];
    std::vector<unsigned char> core_sorted(n);
    std::vector<int> parent(n), cell_min(ncell, INT_MAX), root(n), rank(n + 1, -1);
    for (int c = 0; c < 6; ++c) counters[c] = 0;
    counters[5] = sc;
    auto cell_id = [&](long long q) { return ((long long)cells[3 * q + 2] * dims[1] + cells[3 * q + 1]) * dims[0] + cells[3 * q]; };
    for (long long q = 0; q < n; ++q) {                          // k_pc_count
        const nwp_pt pt = pts[q];
        const long long c = cell_id(q);
        int cnt;
        if (sc && cstart[c + 1] - cstart[c] >= cap) { cnt = cap; counters[1] += 1; }
        else {
            nwp_count_visit v = {(double)pt.x, (double)pt.y, (double)pt.z, eps2, 0, cap, 0};
            nwp_walk(pts, cstart, dims, h, cells[3 * q], cells[3 * q + 1], cells[3 * q + 2], eps2, 0, v);
            cnt = v.cnt;
            counters[0] += v.tests;
        }
        const bool is_core = cnt >= min_points;
        count[pt.i] = cnt;
        core[pt.i] = core_sorted[q] = is_core ? 1 : 0;
        parent[pt.i] = pt.i;
        if (sc && is_core && pt.i < cell_min[c]) cell_min[c] = pt.i;
    }
    seq_union u = {parent.data()};
    for (long long q = 0; q < n; ++q) {                          // k_pc_hook
        if (!core_sorted[q]) continue;
        const nwp_pt pt = pts[q];
        if (sc) {
            const int m = cell_min[cell_id(q)];
            if (m < pt.i) { u.unite(pt.i, m); counters[3] += 1; }
        }
        nwp_hook_visit<seq_union> v = {(double)pt.x, (double)pt.y, (double)pt.z, eps2, pt.i, sc != 0, core_sorted.data(), &u, 0};
        nwp_walk(pts, cstart, dims, h, cells[3 * q], cells[3 * q + 1], cells[3 * q + 2], eps2, sc ? 1 : 0, v);
        counters[2] += v.tests;
    }
    int C = 0;                                                   // k_pc_compress, the scan, k_pc_number
    for (long long i = 0; i < n; ++i) root[i] = core[i] ? u.find((int)i) : -1;
    for (long long i = 0; i < n; ++i) if (root[i] == i) rank[i] = C++;
    for (long long i = 0; i < n; ++i) { label[i] = root[i] < 0 ? -1 : rank[root[i]]; anchor[i] = root[i] < 0 ? -1 : (int)i; }
    for (long long q = 0; q < n; ++q) {                          // k_pc_border
        if (core_sorted[q]) continue;
        const nwp_pt pt = pts[q];
        nwp_border_visit v = {(double)pt.x, (double)pt.y, (double)pt.z, eps2, core_sorted.data(), 0.0, -1, 0};
        nwp_walk(pts, cstart, dims, h, cells[3 * q], cells[3 * q + 1], cells[3 * q + 2], eps2, 0, v);
        counters[4] += v.tests;
        if (v.best_i >= 0) { anchor[pt.i] = v.best_i; label[pt.i] = rank[root[v.best_i]]; }
    }
    return C;
}

extern "C" int shim_guard(double h, double eps) { return nwp_shortcuts_ok(h, eps) ? 1 : 0; }
extern "C" int shim_args_ok(double eps, long long min_points, long long count_cap) { return nwp_args_ok(eps, min_points, count_cap) ? 1 : 0; }

#ifdef NWP_MAIN
// the same call on arrays read from a file: <in> holds 5 int64 (n, ncell, min_points, count_cap, shortcuts_on), 2 doubles (h, eps), 3 int dims,
// then pts, cells, cstart
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 5);
    const auto dbl = rd<double>(fh, 2);
    const auto dims = rd<int>(fh, 3);
    const auto pts = rd<nwp_pt>(fh, c[0]);
    const auto cells = rd<int>(fh, 3 * c[0]);
    const auto cstart = rd<int>(fh, c[1] + 1);
    fclose(fh);
    const size_t n = (size_t)c[0];
    std::vector<int> label(n), anchor(n), count(n);
    std::vector<unsigned char> core(n);
    long long counters[6];
    const int C = shim_dbscan(pts.data(), cells.data(), cstart.data(), dims.data(), dbl[0], c[0], dbl[1], c[2], c[3], (int)c[4], label.data(), anchor.data(),
                              count.data(), core.data(), counters);
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(&C, sizeof(int), 1, fh);
    fwrite(label.data(), sizeof(int), n, fh);
    fwrite(anchor.data(), sizeof(int), n, fh);
    fwrite(count.data(), sizeof(int), n, fh);
    fwrite(core.data(), 1, n, fh);
    fwrite(counters, sizeof(long long), 6, fh);
    fclose(fh);
    return 0;
}
#endif
'''

PT = np.dtype([('x', np.float32), ('y', np.float32), ('z', np.float32), ('i', np.int32)])
p = lambda a: a.ctypes.data


def _source(tmp):
    src = os.path.join(str(tmp), 'shim.cpp')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    return src


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwp_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwp_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f64, ll, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_longlong, ctypes.c_int
    L.shim_dbscan.argtypes = [vp, vp, vp, vp, f64, ll, f64, ll, ll, i32] + [vp] * 5
    L.shim_guard.argtypes = [f64, f64]
    L.shim_args_ok.argtypes = [f64, ll, ll]
    return L


def point_grid(P32, h, seed=0):
    """the cloud binned as bq::build_grid<float> bins it: float32 cell indices floorf((x - lo) / h) clamped to dims = floor(ext / h) + 1, a
    counting sort by cell id, the order inside a cell shuffled -> (pts, cells of the sorted points, cstart, dims, (double)(float)h)"""
    P32 = R.cloud32(P32)
    lo, hi = P32.min(0), P32.max(0)
    h32 = np.float32(h)
    dims = (np.floor((hi.astype(np.float64) - lo.astype(np.float64)) / float(h)) + 1.0).astype(np.int32)
    t = np.floor((P32 - lo) / h32)                                # float32 throughout
    cells = np.minimum(np.maximum(t, np.float32(0)), (dims - 1).astype(np.float32)).astype(np.int32)
    cid = (cells[:, 2].astype(np.int64) * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
    order = np.lexsort((np.random.default_rng(seed).random(len(P32)), cid))
    ncell = int(dims[0]) * int(dims[1]) * int(dims[2])
    cstart = np.zeros(ncell + 1, np.int32)
    np.cumsum(np.bincount(cid, minlength=ncell), out=cstart[1:])
    pts = np.empty(len(P32), PT)
    pts['x'], pts['y'], pts['z'], pts['i'] = P32[order, 0], P32[order, 1], P32[order, 2], order
    return pts, np.ascontiguousarray(cells[order]), cstart, np.ascontiguousarray(dims), float(h32)


def shim_dbscan(lib, P32, eps, min_points, count_cap=None, h=None, shortcuts=True, seed=0):
    P32 = R.cloud32(P32)
    n = len(P32)
    cap = int(min_points) if count_cap is None else int(count_cap)
    pts, cells, cstart, dims, hd = point_grid(P32, 0.57 * eps if h is None else h, seed)
    out = dict(labels=np.empty(n, np.int32), anchor=np.empty(n, np.int32), count=np.empty(n, np.int32), core=np.empty(n, np.uint8))
    counters = np.zeros(6, np.int64)
    out['n_clusters'] = lib.shim_dbscan(p(pts), p(cells), p(cstart), p(dims), hd, n, float(eps), int(min_points), cap, int(shortcuts),
                                        p(out['labels']), p(out['anchor']), p(out['count']), p(out['core']), p(counters))
    out['counters'] = dict(zip(('tests_count', 'shortcut_a', 'tests_hook', 'shortcut_b', 'tests_border', 'guard'), counters.tolist()))
    out['blob'] = (pts, cells, cstart, dims, hd, n, float(eps), int(min_points), cap, int(shortcuts))
    return out


def same(mine, ref):
    for k in ('labels', 'anchor', 'count'):
        assert np.array_equal(mine[k], ref[k]), k
    assert np.array_equal(mine['core'].astype(bool), ref['core']) and mine['n_clusters'] == ref['n_clusters']


def check(lib, P, eps, min_points, count_cap=None, expect_fired=True):
    """the restatement's arrays at four cell sizes: 0.3 eps and 0.57 eps have the shortcuts, eps and 3 eps forbid them"""
    ref = R.dbscan(P, eps, min_points, count_cap)
    for k, h in enumerate((0.3 * eps, 0.57 * eps, 1.0 * eps, 3.0 * eps)):
        mine = shim_dbscan(lib, P, eps, min_points, count_cap, h, seed=k)
        same(mine, ref)
        c = mine['counters']
        assert c['guard'] == (1 if k < 2 else 0)
        if k >= 2:
            assert c['shortcut_a'] == 0 and c['shortcut_b'] == 0
        off = shim_dbscan(lib, P, eps, min_points, count_cap, h, shortcuts=False, seed=k)
        same(off, ref)
        assert off['counters']['guard'] == 0 and off['counters']['shortcut_a'] == 0 and off['counters']['shortcut_b'] == 0
        if k < 2 and expect_fired:
            assert c['tests_count'] + c['tests_hook'] <= off['counters']['tests_count'] + off['counters']['tests_hook']
    return ref


def clumps(seed, offset=0.0):
    rng = np.random.default_rng(seed)
    parts = [rng.normal(c, 1.5, (200, 3)) for c in ((0, 0, 0), (30, 5, 0), (10, 40, 20))] + [rng.uniform(-20, 60, (200, 3))]
    return (np.concatenate(parts) + offset).astype(np.float32)


def test_each_shortcut_fires_on_a_small_cell_and_neither_on_a_large_one(lib):
    P = clumps(1)
    ref = R.dbscan(P, 4.0, 8)
    small, large = shim_dbscan(lib, P, 4.0, 8, h=0.57 * 4.0), shim_dbscan(lib, P, 4.0, 8, h=2.0 * 4.0)
    same(small, ref)
    same(large, ref)
    assert small['counters']['guard'] == 1 and small['counters']['shortcut_a'] > 0 and small['counters']['shortcut_b'] > 0
    assert large['counters']['guard'] == 0 and large['counters']['shortcut_a'] == 0 and large['counters']['shortcut_b'] == 0
    assert small['counters']['tests_count'] < shim_dbscan(lib, P, 4.0, 8, h=0.57 * 4.0, shortcuts=False)['counters']['tests_count']
    check(lib, P, 4.0, 8)
    check(lib, P, 4.0, 8, count_cap=30)
    check(lib, P, 4.0, 8, count_cap=10 ** 6)


def test_the_guard_and_the_arguments(lib):
    s3 = np.sqrt(3.0)
    assert lib.shim_guard(0.57, 1.0) == 1 and lib.shim_guard(0.57 * 25.0, 25.0) == 1
    assert lib.shim_guard(1.0 / (s3 * (1 + 2.0 / 1024)) * (1 - 1e-8), 1.0) == 1 and lib.shim_guard(1.0 / (s3 * (1 + 2.0 / 1024)), 1.0) == 0
    assert lib.shim_guard(1.0 / s3, 1.0) == 0 and lib.shim_guard(0.58, 1.0) == 0 and lib.shim_guard(0.57 * 1.1, 1.0) == 0      # one widening step
    ok = lib.shim_args_ok
    assert ok(1.0, 1, 1) == 1 and ok(2.0 ** 40, 1 << 30, 1 << 30) == 1 and ok(5e-324, 3, 7) == 1
    for eps in (0.0, -1.0, np.nan, np.inf, 2.0 ** 40 * 1.0000001):
        assert ok(eps, 3, 3) == 0
    assert ok(1.0, 0, 3) == 0 and ok(1.0, 4, 3) == 0 and ok(1.0, (1 << 30) + 1, (1 << 30) + 1) == 0 and ok(1.0, 3, (1 << 30) + 1) == 0


def test_the_lattices(lib):
    check(lib, R.lattice(7), 1.0, 7, expect_fired=False)
    check(lib, R.lattice(7), 1.0, 7, count_cap=100, expect_fired=False)
    check(lib, R.lattice(5, 0.25), 1.0, 20)                       # many lattice points per cell
    check(lib, R.chain(200, 1.0), 1.0, 2, expect_fired=False)
    check(lib, R.chain(200, 1.0), float(np.nextafter(1.0, 0.0)), 2, expect_fired=False)
    check(lib, R.chain(3, 1.0, wider=True), 1.0, 2, expect_fired=False)
    check(lib, R.bridge(), 2.0, 10, expect_fired=False)
    check(lib, np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1)), 0.5, 300, count_cap=1000)
    check(lib, np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1)), 0.5, 301)


def test_a_cell_with_exactly_min_points_and_one_fewer(lib):
    rng = np.random.default_rng(5)
    m = 9
    A = 0.2 + rng.uniform(0.0, 0.1, (m, 3))                       # m points in one cell of 0.57
    B = np.array([10.0, 0.0, 0.0]) + 0.2 + rng.uniform(0.0, 0.1, (m - 1, 3))
    P = np.concatenate([A, B, [[-5.0, -5.0, -5.0], [20.0, 5.0, 5.0]]]).astype(np.float32)      # (two lone points span the box)
    ref = check(lib, P, 1.0, m)
    assert ref['core'][:m].all() and not ref['core'][m:].any() and ref['n_clusters'] == 1
    mine = shim_dbscan(lib, P, 1.0, m, h=0.57)
    assert mine['counters']['shortcut_a'] == m and mine['counters']['shortcut_b'] == m - 1


@pytest.mark.parametrize('name', ['far', 'plane', 'axis', 'diagonal'])
def test_degenerate_extents(lib, name):
    rng = np.random.default_rng(7)
    if name == 'far':
        P = clumps(3, offset=1.0e6)                               # float32 steps of 1/16 out there
    elif name == 'plane':
        P = clumps(4)
        P[:, 2] = 3.0
    elif name == 'axis':
        P = np.zeros((400, 3), np.float32)
        P[:, 1] = np.sort(rng.uniform(0.0, 300.0, 400))
    else:
        P = np.repeat(rng.uniform(0.0, 200.0, 400).astype(np.float32)[:, None], 3, 1)
    check(lib, P, 4.0, 5, expect_fired=False)
    check(lib, P, 4.0, 5, count_cap=1000, expect_fired=False)


def test_the_same_core_under_the_sanitizers(lib, tmp_path):
    """the shim with a main of its own, built with -fsanitize=address,undefined and run as a program: no report, and the same bytes"""
    exe = os.path.join(str(tmp_path), 'shim_san')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DNWP_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)])
    for k, (P, eps, mp, cap, h) in enumerate([(clumps(1), 4.0, 8, 30, 0.57 * 4.0), (clumps(1), 4.0, 8, 8, 8.0), (R.lattice(7), 1.0, 7, 100, 0.3),
                                              (R.bridge(), 2.0, 10, 10, 0.57 * 2.0)]):
        mine = shim_dbscan(lib, P, eps, mp, cap, h)
        pts, cells, cstart, dims, hd, n, eps_, mp_, cap_, on = mine['blob']
        fin, fout = os.path.join(str(tmp_path), 'in%d.bin' % k), os.path.join(str(tmp_path), 'out%d.bin' % k)
        with open(fin, 'wb') as fh:
            fh.write(np.array([n, len(cstart) - 1, mp_, cap_, on], np.int64).tobytes())
            fh.write(np.array([hd, eps_], np.float64).tobytes())
            fh.write(dims.astype(np.int32).tobytes())
            fh.write(pts.tobytes() + cells.tobytes() + cstart.tobytes())
        res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        raw = open(fout, 'rb').read()
        C = int(np.frombuffer(raw, np.int32, 1)[0])
        arr = np.frombuffer(raw, np.int32, 3 * n, 4).reshape(3, n)
        core = np.frombuffer(raw, np.uint8, n, 4 + 12 * n)
        counters = np.frombuffer(raw[4 + 13 * n:], np.int64, 6)
        assert C == mine['n_clusters'] and np.array_equal(arr[0], mine['labels']) and np.array_equal(arr[1], mine['anchor'])
        assert np.array_equal(arr[2], mine['count']) and np.array_equal(core, mine['core'])
        assert counters.tolist() == list(mine['counters'].values())
