"""
The pair-count query, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_pairs_core.h holds the edges, the bin (as the literal sum and as
the search) and the walk of one query over a clamped box of cells as __host__ __device__ functions over a cell grid handed in as
arrays.  This test compiles them for the CPU (g++ -ffp-contract=off) behind a shim of its own -- one query after the other, the
device's visitor without its LDS -- and asks for the restatement's (tests/pair_counts_ref.py) hist and local bit for bit.  The grid is
binned here in NumPy with float32 cell indices, at four cell sizes: the default, a fifth of it, one cell for the whole cloud and a
widened grid.  The restatement uses no grid, so a mistake in the walk shows as a wrong count.  The same source with a main of its own
runs once under -fsanitize=address,undefined, as a program.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pair_counts_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nw_pairs_core.h"

struct shim_visit {
    double x, y, z;
    int self, m, search;
    const double *e2;
    unsigned *row;
    long long tests;
    int mismatch;
    void operator()(const nwq_pt &p)
    {
        if (p.i == self) return;
        ++tests;
        const double d2 = nwq_dist2(p, x, y, z);
        const int a = nwq_bin_sum(e2, NWQ_MAX_BINS, d2), b = nwq_bin_search(e2, d2);
        if (a != b || a != nwq_bin_sum(e2, m, d2)) mismatch = 1;
        const int bin = search ? b : a;
        if (bin < m) row[bin] += 1u;
    }
};

// pts in cell order, cstart the cells' starts, box = lo[3] hi[3] h (the floats of the grid as doubles); queries = NULL: auto mode.
// counters: distance tests, cells read -> 0, -1 for bad radii, -2 if the two forms of the bin ever differed
extern "C" int shim_pairs(const nwq_pt *pts, const int *cstart, const int *dims, const double *box, long long n, const float *queries, long long nq,
                          const double *radii, long long m, int search, unsigned long long *hist, unsigned *local, long long *counters)
{
    double e2[NWQ_MAX_BINS];
    if (!nwq_edges(radii, m, e2)) return -1;
    nwq_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = box[d]; g.hi[d] = box[3 + d]; g.dims[d] = dims[d]; }
    g.h = box[6];
    counters[0] = counters[1] = 0;
    for (long long b = 0; b < m; ++b) hist[b] = 0;
    const long long n_queries = queries ? nq : n;
    int mismatch = 0;
    for (long long p = 0; p < n_queries; ++p) {
        shim_visit v;
        long long row;
        if (queries) { v.x = (double)queries[3 * p]; v.y = (double)queries[3 * p + 1]; v.z = (double)queries[3 * p + 2]; v.self = -1; row = p; }
        else { v.x = (double)pts[p].x; v.y = (double)pts[p].y; v.z = (double)pts[p].z; v.self = pts[p].i; row = pts[p].i; }
        v.m = (int)m; v.search = search; v.e2 = e2; v.row = local + row * m; v.tests = 0; v.mismatch = 0;
        for (long long b = 0; b < m; ++b) v.row[b] = 0u;
        long long cells = 0;
        nwq_walk(pts, cstart, g, v.x, v.y, v.z, radii[m - 1], e2[m - 1], v, &cells);
        counters[0] += v.tests;
        counters[1] += cells;
        mismatch |= v.mismatch;
        for (long long b = 0; b < m; ++b) hist[b] += v.row[b];
    }
    return mismatch ? -2 : 0;
}

extern "C" int shim_edges(const double *radii, long long m, double *e2) { return nwq_edges(radii, m, e2) ? 1 : 0; }
extern "C" int shim_bin(const double *e2, int m, double d2, int search) { return search ? nwq_bin_search(e2, d2) : nwq_bin_sum(e2, m, d2); }

#ifdef NWQ_MAIN
// the same call on arrays read from a file: <in> holds 5 int64 (n, ncell, nq or -1 for auto, m, search), 7 doubles (the box), 3 int dims,
// m doubles (radii), then pts, cstart and the queries
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 5);
    const auto box = rd<double>(fh, 7);
    const auto dims = rd<int>(fh, 3);
    const auto radii = rd<double>(fh, c[3]);
    const auto pts = rd<nwq_pt>(fh, c[0]);
    const auto cstart = rd<int>(fh, c[1] + 1);
    const auto queries = rd<float>(fh, c[2] < 0 ? 0 : 3 * c[2]);
    fclose(fh);
    const size_t nq = (size_t)(c[2] < 0 ? c[0] : c[2]), m = (size_t)c[3];
    std::vector<unsigned long long> hist(m);
    std::vector<unsigned> local(nq * m);
    long long counters[2];
    const int r = shim_pairs(pts.data(), cstart.data(), dims.data(), box.data(), c[0], c[2] < 0 ? nullptr : queries.data(), c[2], radii.data(), c[3], (int)c[4],
                             hist.data(), local.data(), counters);
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(&r, sizeof(int), 1, fh);
    fwrite(hist.data(), sizeof(unsigned long long), m, fh);
    fwrite(local.data(), sizeof(unsigned), nq * m, fh);
    fwrite(counters, sizeof(long long), 2, fh);
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
    d = tmp_path_factory.mktemp('nwq_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwq_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f64, ll, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_longlong, ctypes.c_int
    L.shim_pairs.argtypes = [vp, vp, vp, vp, ll, vp, ll, vp, ll, i32, vp, vp, vp]
    L.shim_edges.argtypes = [vp, ll, vp]
    L.shim_bin.argtypes = [vp, i32, f64, i32]
    return L


def cell_sizes(P32, r_max):
    """the four cell sizes of the test: the library's default max(0.5 r_max, extent / 1024), a fifth of it (never below extent / 1024: the
    walk's proof needs that), one cell for the whole cloud, and the default widened by three tenths"""
    P32 = R.cloud32(P32)
    emax = float((P32.max(0).astype(np.float64) - P32.min(0).astype(np.float64)).max())
    floor_ = emax / 1024.0
    default = max(0.5 * r_max, floor_)
    if not np.float32(default) > 0:
        default = emax if emax > 0 else 1.0
    fifth = max(0.1 * r_max, floor_)
    if not np.float32(fifth) > 0:
        fifth = default
    return dict(default=default, fifth=fifth, one_cell=2.0 * emax if emax > 0 else 1.0, widened=default * 1.1 ** 3)


def point_grid(P32, h, seed=0):
    """the cloud binned as bq::build_grid<float> bins it: float32 cell indices floorf((x - lo) / h) clamped to dims = min(1025,
    floor(ext / h) + 1), a counting sort by cell id, the order inside a cell shuffled -> (pts, cstart, dims, box = lo hi h as doubles)"""
    P32 = R.cloud32(P32)
    lo, hi = P32.min(0), P32.max(0)
    h32 = np.float32(h)
    dims = np.minimum(1025.0, np.floor((hi.astype(np.float64) - lo.astype(np.float64)) / float(h)) + 1.0).astype(np.int32)
    t = np.floor((P32 - lo) / h32)                                # float32 throughout
    cells = np.minimum(np.maximum(t, np.float32(0)), (dims - 1).astype(np.float32)).astype(np.int32)
    cid = (cells[:, 2].astype(np.int64) * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
    order = np.lexsort((np.random.default_rng(seed).random(len(P32)), cid))
    ncell = int(dims[0]) * int(dims[1]) * int(dims[2])
    cstart = np.zeros(ncell + 1, np.int32)
    np.cumsum(np.bincount(cid, minlength=ncell), out=cstart[1:])
    pts = np.empty(len(P32), PT)
    pts['x'], pts['y'], pts['z'], pts['i'] = P32[order, 0], P32[order, 1], P32[order, 2], order
    box = np.concatenate([lo.astype(np.float64), hi.astype(np.float64), [float(h32)]])
    return pts, cstart, np.ascontiguousarray(dims), box


def shim_pairs(lib, cloud, radii, queries=None, h=None, search=False, seed=0):
    cloud = R.cloud32(cloud)
    radii = np.ascontiguousarray(radii, np.float64)
    m, n = len(radii), len(cloud)
    pts, cstart, dims, box = point_grid(cloud, cell_sizes(cloud, float(radii[-1]))['default'] if h is None else h, seed)
    Q = None if queries is None else R.cloud32(queries)
    nq = n if Q is None else len(Q)
    hist, local, counters = np.zeros(m, np.uint64), np.full((nq, m), 7, np.uint32), np.zeros(2, np.int64)
    r = lib.shim_pairs(p(pts), p(cstart), p(dims), p(box), n, None if Q is None else p(Q), -1 if Q is None else nq, p(radii), m, int(search), p(hist), p(local),
                       p(counters))
    assert r == 0, r
    return dict(hist=hist, cumulative=np.cumsum(hist, dtype=np.uint64), local=local, n_queries=nq, n_cloud=n, tests=int(counters[0]), cells=int(counters[1]),
                blob=(pts, cstart, dims, box, n, Q, radii, int(search)))


def check(lib, cloud, radii, queries=None):
    """the restatement's arrays at the four cell sizes, counted through the sum or through the search"""
    ref = R.pair_counts(cloud, radii) if queries is None else R.pair_counts(queries, radii, other=cloud)
    sizes = cell_sizes(cloud, float(np.asarray(radii, np.float64)[-1]))
    seen = {}
    for k, (name, h) in enumerate(sizes.items()):
        for search in ((False, True) if name == 'default' else (k % 2 == 1,)):       # (the shim compares the two forms on every pair anyway)
            mine = shim_pairs(lib, cloud, radii, queries, h, search, seed=k)
            R.same_as_restatement(mine, ref)
            seen[name] = mine
    if queries is None:                                           # one cell and a query inside the box: every pair is tested
        assert seen['one_cell']['tests'] == ref['n_cloud'] * (ref['n_cloud'] - 1) and seen['one_cell']['cells'] == ref['n_cloud']
    assert all(s['tests'] >= int(ref['hist'].sum()) for s in seen.values())
    return ref, seen


EDGES = {'lattice': [1.0, 1.5, 2.0], 'below': [float(np.nextafter(1.0, 0.0)), 1.5, 2.0], 'above': [float(np.nextafter(1.0, 2.0)), 1.5, 2.0],
         'seventeen': list(np.linspace(0.0, 3.2, 17)), 'sixty_four': list(np.linspace(0.05, 3.2, 64)), 'one': [1.0]}


def test_the_edges_and_the_bin(lib):
    e2 = np.zeros(64)
    ok = lambda r: lib.shim_edges(p(np.ascontiguousarray(r, np.float64)), len(r), p(e2))
    assert ok([1.0]) == 1 and ok([0.0]) == 1 and ok([0.0, 1.0, 2.0 ** 40]) == 1 and ok(list(np.arange(64.0))) == 1
    r = np.array([1.0, 1.5, 2.0])
    assert ok(r) == 1 and np.array_equal(e2[:3], r * r) and np.isinf(e2[3:]).all()
    assert ok([]) == 0 and ok(list(np.arange(65.0))) == 0
    for bad in ([np.nan], [1.0, np.nan], [np.inf], [-1.0, 1.0], [-0.5], [2.0, 1.0], [1.0, 1.0], [1.0, 2.0, 2.0], [2.0 ** 40 * 1.0000001]):
        assert ok(bad) == 0, bad
    assert ok([1.0, float(np.nextafter(1.0, 2.0))]) == 1                                               # distinct squares
    assert ok([1e-200, 2e-200]) == 0 and ok([0.0, 1e-200]) == 0                                        # both square to zero
    tiny = 1.0 + 2.0 ** -52
    assert tiny * tiny != 1.0 and ok([1.0, tiny]) == 1
    # the two forms of the bin against np.searchsorted, at the edges, one ulp beside them and far out
    rng = np.random.default_rng(0)
    for m in (1, 2, 15, 16, 17, 63, 64):
        radii = np.sort(rng.uniform(0.0, 10.0, m))
        radii[0] = 0.0 if m % 2 else radii[0]
        assert ok(radii) == 1
        probes = np.concatenate([e2[:m], np.nextafter(e2[:m], -1.0), np.nextafter(e2[:m], np.inf), rng.uniform(0.0, 120.0, 50), [0.0, 1e300, np.inf]])
        for d2 in probes[probes >= 0]:
            want = int(np.searchsorted(e2[:m], d2, 'left'))
            assert lib.shim_bin(p(e2), m, float(d2), 0) == want and lib.shim_bin(p(e2), m, float(d2), 1) == want, (m, d2)


@pytest.mark.parametrize('edges', list(EDGES))
def test_the_lattice(lib, edges):
    ref, _ = check(lib, R.lattice(7), EDGES[edges])
    if edges == 'lattice':
        assert ref['hist'].tolist() == [1764, 3024, 3198]
    if edges == 'below':
        assert ref['hist'].tolist() == [0, 4788, 3198]


def test_duplicates_and_one_point(lib):
    dup = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    ref, _ = check(lib, dup, [0.0, 0.5])
    assert ref['hist'].tolist() == [300 * 299, 0]
    ref, _ = check(lib, dup, [0.0])
    assert ref['hist'].tolist() == [300 * 299]
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    ref, _ = check(lib, one, [0.0, 1.0, 5.0])
    assert ref['hist'].tolist() == [0, 0, 0]
    ref, _ = check(lib, one, [0.0, 1.0, 5.0], queries=np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [100.0, 2.0, 3.0]], np.float32))
    assert ref['local'].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 0]]


@pytest.mark.parametrize('name', ['clustered', 'plane', 'axis', 'far'])
def test_clouds_and_degenerate_extents(lib, name):
    rng = np.random.default_rng(11)
    if name == 'clustered':
        P = R.clustered(700, 1)
    elif name == 'plane':
        P = R.clustered(600, 2)
        P[:, 2] = 3.0
    elif name == 'axis':
        P = np.zeros((400, 3), np.float32)
        P[:, 1] = rng.uniform(0.0, 300.0, 400)
    else:
        P = R.clustered(600, 3, offset=1.0e6)                     # float32 steps of 1/16 out there
    check(lib, P, [2.0, 4.0, 6.5, 9.0])
    check(lib, P, list(np.linspace(0.0, 12.0, 33)))
    check(lib, P, [1.0e5])                                        # everything in one bin
    check(lib, P, [1.0e-4])                                       # nothing but duplicates


@pytest.mark.parametrize('where', ['faces', 'outside', 'at_points', 'inside'])
def test_cross_queries(lib, where):
    rng = np.random.default_rng(5)
    P = R.clustered(500, 4)
    lo, hi = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    if where == 'faces':                                          # on the box's faces, edges and corners
        Q = rng.uniform(lo, hi, (120, 3))
        for k in range(len(Q)):
            for d in range(3):
                if (k >> d) & 1 or k % 3 == d:
                    Q[k, d] = lo[d] if (k >> (d + 3)) & 1 else hi[d]
    elif where == 'outside':                                      # up to ten diagonals away, in every direction
        u = rng.normal(size=(120, 3))
        Q = (lo + hi) / 2 + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(0.5, 10.0, (120, 1)) * diag
    elif where == 'at_points':
        Q = P[rng.integers(0, len(P), 77)]
    else:
        Q = rng.uniform(lo, hi, (130, 3))
    Q = Q.astype(np.float32)
    check(lib, P, [2.0, 4.0, 6.5, 9.0], queries=Q)
    check(lib, P, list(np.linspace(0.5, 40.0, 40)), queries=Q)
    check(lib, P, [0.0, 12.0 * diag], queries=Q)                  # every pair in bin 1 (coincident ones in bin 0)


def test_a_smaller_cell_tests_fewer_points(lib):
    P = R.clustered(1500, 8)
    _, seen = check(lib, P, [1.0, 2.0, 3.0])
    assert seen['fifth']['tests'] < seen['default']['tests'] < seen['widened']['tests'] < seen['one_cell']['tests']
    assert seen['fifth']['cells'] > seen['default']['cells'] > seen['one_cell']['cells']


def test_the_same_core_under_the_sanitizers(lib, tmp_path):
    """the shim with a main of its own, built with -fsanitize=address,undefined and run as a program: no report, and the same bytes"""
    exe = os.path.join(str(tmp_path), 'shim_san')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DNWQ_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)])
    P = R.clustered(400, 9)
    far = (P[:50].astype(np.float64) * 30.0 + 500.0).astype(np.float32)
    runs = [(P, [2.0, 4.0, 6.5], None, None, False), (P, list(np.linspace(0.0, 12.0, 64)), None, 0.3, True), (R.lattice(7), [1.0, 1.5, 2.0], None, 100.0, False),
            (P, [3.0, 9.0], far, None, True), (P[:1], [0.0, 1.0], P[:5], None, False)]
    for k, (cloud, radii, Q, h, search) in enumerate(runs):
        mine = shim_pairs(lib, cloud, radii, Q, h, search)
        pts, cstart, dims, box, n, Q32, r64, s = mine['blob']
        fin, fout = os.path.join(str(tmp_path), 'in%d.bin' % k), os.path.join(str(tmp_path), 'out%d.bin' % k)
        with open(fin, 'wb') as fh:
            fh.write(np.array([n, len(cstart) - 1, -1 if Q32 is None else len(Q32), len(r64), s], np.int64).tobytes())
            fh.write(box.tobytes() + dims.astype(np.int32).tobytes() + r64.tobytes() + pts.tobytes() + cstart.tobytes())
            if Q32 is not None:
                fh.write(Q32.tobytes())
        res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        raw = open(fout, 'rb').read()
        m, nq = len(r64), mine['n_queries']
        assert int(np.frombuffer(raw, np.int32, 1)[0]) == 0
        assert np.array_equal(np.frombuffer(raw, np.uint64, m, 4), mine['hist'])
        assert np.array_equal(np.frombuffer(raw, np.uint32, nq * m, 4 + 8 * m).reshape(nq, m), mine['local'])
        assert np.frombuffer(raw[4 + 8 * m + 4 * nq * m:], np.int64, 2).tolist() == [mine['tests'], mine['cells']]
