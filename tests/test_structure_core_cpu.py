"""
The local-shape query, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_structure_core.h holds the radius, the quantisation, the ten
moments, the covariance with its Jacobi iteration and the walk of one query over a clamped box of cells as __host__ __device__ functions
over a cell grid handed in as arrays.  This test compiles them for the CPU (g++ -ffp-contract=off) behind a shim of its own -- one query
after the other, the device's visitor and its two kernels' bodies -- and asks for the restatement's (tests/local_shape_ref.py) moments,
eigenvalues, vectors and flags bit for bit.  The grid is binned here in NumPy with float32 cell indices, at four cell sizes: the default,
a fifth of it, one cell for the whole cloud and a widened grid.  The restatement uses no grid, so a mistake in the walk shows as a wrong
integer.  The same source with a main of its own runs once under -fsanitize=address,undefined, as a program.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import local_shape_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nw_structure_core.h"

struct shim_visit {
    double x, y, z, r2, s;
    nwf_sums m;
    long long tests;
    void operator()(const nwf_pt &p)
    {
        ++tests;
        nwf_visit(&m, p.x, p.y, p.z, x, y, z, r2, s);
    }
};

// pts in cell order, cstart the cells' starts, box = lo[3] hi[3] h (the floats of the grid as doubles); queries = NULL: auto mode.
// counters: distance tests, cells read, neighbours summed, queries with n < 3 -> 0, -1 for a bad radius, -2 if a |u| ever exceeded 2^18
extern "C" int shim_shape(const nwf_pt *pts, const int *cstart, const int *dims, const double *box, long long n, const float *queries, long long nq,
                          double r, const double *view, long long *moments, double *lam, double *vec, unsigned char *flags, long long *counters)
{
    double r2 = 0.0, s = 0.0, step = 0.0;
    if (!nwf_radius(r, &r2)) return -1;
    nwf_scale(r, &s, &step);
    nwf_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = box[d]; g.hi[d] = box[3 + d]; g.dims[d] = dims[d]; }
    g.h = box[6];
    counters[0] = counters[1] = counters[2] = counters[3] = 0;
    const long long n_queries = queries ? nq : n;
    const long long top = (1ll << NWF_Q_BITS) * (1ll << NWF_Q_BITS);
    int over = 0;
    for (long long p = 0; p < n_queries; ++p) {
        shim_visit v;
        long long row;
        if (queries) { v.x = (double)queries[3 * p]; v.y = (double)queries[3 * p + 1]; v.z = (double)queries[3 * p + 2]; row = p; }
        else { v.x = (double)pts[p].x; v.y = (double)pts[p].y; v.z = (double)pts[p].z; row = pts[p].i; }
        v.r2 = r2; v.s = s; v.tests = 0;
        nwf_sums_init(&v.m);
        int cells = 0;
        nwf_walk(pts, cstart, g, v.x, v.y, v.z, r, r2, v, &cells);
        counters[0] += v.tests;
        counters[1] += cells;
        counters[2] += v.m.n;
        counters[3] += v.m.n < 3 ? 1 : 0;
        if (v.m.xx > v.m.n * top || v.m.yy > v.m.n * top || v.m.zz > v.m.n * top) over = 1;
        long long *out = moments + row * NWF_MOMENTS;
        out[0] = v.m.n; out[1] = v.m.sx; out[2] = v.m.sy; out[3] = v.m.sz; out[4] = v.m.xx; out[5] = v.m.xy; out[6] = v.m.xz;
        out[7] = v.m.yy; out[8] = v.m.yz; out[9] = v.m.zz;
        const double wx = view ? view[0] - v.x : 0.0, wy = view ? view[1] - v.y : 0.0, wz = view ? view[2] - v.z : 0.0;
        flags[row] = nwf_shape(v.m, step, view != nullptr, wx, wy, wz, lam + 3 * row, vec + 9 * row);
    }
    return over ? -2 : 0;
}

extern "C" int shim_radius(double r, double *out)
{
    if (!nwf_radius(r, out)) return 0;
    out[1] = nwf_pow2_above(r);
    nwf_scale(r, out + 2, out + 3);
    return 1;
}

#ifdef NWF_MAIN
// the same call on arrays read from a file: <in> holds 4 int64 (n, ncell, nq or -1 for auto, 1 if a viewpoint follows), 7 doubles (the
// box), 3 int dims, r and the viewpoint (4 doubles), then pts, cstart and the queries
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 4);
    const auto box = rd<double>(fh, 7);
    const auto dims = rd<int>(fh, 3);
    const auto rv = rd<double>(fh, 4);
    const auto pts = rd<nwf_pt>(fh, c[0]);
    const auto cstart = rd<int>(fh, c[1] + 1);
    const auto queries = rd<float>(fh, c[2] < 0 ? 0 : 3 * c[2]);
    fclose(fh);
    const size_t nq = (size_t)(c[2] < 0 ? c[0] : c[2]);
    std::vector<long long> moments(nq * NWF_MOMENTS);
    std::vector<double> lam(nq * 3), vec(nq * 9);
    std::vector<unsigned char> flags(nq);
    long long counters[4];
    const int r = shim_shape(pts.data(), cstart.data(), dims.data(), box.data(), c[0], c[2] < 0 ? nullptr : queries.data(), c[2], rv[0], c[3] ? rv.data() + 1 : nullptr,
                             moments.data(), lam.data(), vec.data(), flags.data(), counters);
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(&r, sizeof(int), 1, fh);
    fwrite(moments.data(), sizeof(long long), moments.size(), fh);
    fwrite(lam.data(), sizeof(double), lam.size(), fh);
    fwrite(vec.data(), sizeof(double), vec.size(), fh);
    fwrite(flags.data(), 1, flags.size(), fh);
    fwrite(counters, sizeof(long long), 4, fh);
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
    d = tmp_path_factory.mktemp('nwf_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwf_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f64, ll = ctypes.c_void_p, ctypes.c_double, ctypes.c_longlong
    L.shim_shape.argtypes = [vp, vp, vp, vp, ll, vp, ll, f64, vp, vp, vp, vp, vp, vp]
    L.shim_radius.argtypes = [f64, vp]
    return L


def cell_sizes(P32, r):
    """the four cell sizes of the test: the library's default max(0.5 r, extent / 1024), a fifth of it (never below extent / 1024: the
    walk's proof needs that), both widened to the library's cap on the cells, one cell for the whole cloud, and the default widened by
    three tenths more"""
    P32 = R.cloud32(P32)
    emax = float((P32.max(0).astype(np.float64) - P32.min(0).astype(np.float64)).max())
    floor_ = emax / 1024.0
    default = max(0.5 * r, floor_)
    if not (np.float32(default) > 0 and np.isfinite(np.float32(default))):
        default = emax if emax > 0 else 1.0
    fifth = max(0.1 * r, floor_)
    if not np.float32(fifth) > 0:
        fifth = default
    ext = P32.max(0).astype(np.float64) - P32.min(0).astype(np.float64)

    def fit(h):                                                   # widened by a tenth at a time to at most max(2 n, 65 536) cells, as the library does
        while np.prod(np.minimum(1025.0, np.floor(ext / h) + 1.0)) > max(2 * len(P32), 65536):
            h *= 1.1
        return h
    default, fifth = fit(default), fit(fifth)
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


def shim_shape(lib, cloud, r, queries=None, viewpoint=None, h=None, seed=0):
    cloud = R.cloud32(cloud)
    n = len(cloud)
    pts, cstart, dims, box = point_grid(cloud, cell_sizes(cloud, float(r))['default'] if h is None else h, seed)
    Q = None if queries is None else R.cloud32(queries)
    nq = n if Q is None else len(Q)
    view = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float64)
    M, lam, vec, flags = np.full((nq, 10), 7, np.int64), np.full((nq, 3), 7.0), np.full((nq, 3, 3), 7.0), np.full(nq, 77, np.uint8)
    counters = np.zeros(4, np.int64)
    rc = lib.shim_shape(p(pts), p(cstart), p(dims), p(box), n, None if Q is None else p(Q), -1 if Q is None else nq, float(r), None if view is None else p(view),
                        p(M), p(lam), p(vec), p(flags), p(counters))
    assert rc == 0, rc
    return dict(moments=M, eigenvalues=lam, vectors=vec, flags=flags, tests=int(counters[0]), cells=int(counters[1]), neighbours=int(counters[2]),
                few=int(counters[3]), blob=(pts, cstart, dims, box, n, Q, float(r), view))


def check(lib, cloud, r, queries=None, viewpoint=None):
    """the restatement's arrays at the four cell sizes"""
    ref = R.local_shape(cloud, r, viewpoint=viewpoint) if queries is None else R.local_shape(queries, r, other=cloud, viewpoint=viewpoint)
    seen = {}
    for k, (name, h) in enumerate(cell_sizes(cloud, float(r)).items()):
        mine = shim_shape(lib, cloud, r, queries, viewpoint, h, seed=k)
        R.same_as_restatement(mine, ref)
        assert mine['neighbours'] == int(ref['n'].sum()) and mine['few'] == int((ref['n'] < 3).sum()) and mine['tests'] >= mine['neighbours']
        seen[name] = mine
    if queries is None:                                           # one cell and a query inside the box: every point is tested
        assert seen['one_cell']['tests'] == len(ref['n']) ** 2 and seen['one_cell']['cells'] == len(ref['n'])
    return ref, seen


def test_the_radius_and_the_scale(lib):
    out = np.zeros(4)
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf, 2.0 ** 40 * 1.0000001, 1e-170):
        assert lib.shim_radius(float(bad), p(out)) == 0, bad
    for r in (1.0, 2.0, float(np.nextafter(2.0, 0.0)), float(np.nextafter(2.0, 3.0)), 3.0, 0.75, 30.0, 2.0 ** 40, 1e-150, 1e-3, 12345.678):
        assert lib.shim_radius(r, p(out)) == 1
        assert tuple(out) == R.scale(r), r
        assert out[1] >= r > out[1] / 2 and out[2] * out[3] == 1.0 and np.frexp(out[1])[0] == 0.5


def test_the_lattice(lib):
    L = R.lattice(7)
    for r in (2.0, float(np.nextafter(2.0, 0.0)), float(np.nextafter(2.0, 3.0)), 1.0, 1.5):
        ref, _ = check(lib, L, r)
        if r == 2.0:
            assert ref['moments'][171].tolist() == [33, 0, 0, 0, 26 * 2 ** 34, 0, 0, 26 * 2 ** 34, 0, 26 * 2 ** 34]
    ref, _ = check(lib, L, 2.0, queries=np.array([[3.0, 3.0, 3.0], [0.0, 0.0, 0.0], [3.0, 3.0, 8.0], [3.0, 3.0, 8.5]], np.float32))
    assert ref['n'].tolist() == [33, 11, 1, 0]


def test_duplicates_one_cell_and_few_points(lib):
    dup = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    ref, _ = check(lib, dup, 0.5)
    assert (ref['n'] == 300).all() and (ref['flags'] == R.FLAG_POINT).all()
    rng = np.random.default_rng(3)
    crowd = (np.array([40.0, 40.0, 40.0]) + rng.uniform(0.0, 1.0, (5000, 3))).astype(np.float32)       # 5 000 points in one cell of side 2
    lone = np.array([[0.0, 0.0, 0.0], [80.0, 80.0, 80.0]], np.float32)
    cloud = np.concatenate([crowd, lone])
    Q = np.concatenate([crowd[:40], lone, [[40.5, 40.5, 41.9]]]).astype(np.float32)
    mine = shim_shape(lib, cloud, 1.0, Q, h=2.0)
    R.same_as_restatement(mine, R.local_shape(Q, 1.0, other=cloud))
    assert mine['moments'][:40, 0].min() > 500
    for cloud in (np.array([[1.0, 2.0, 3.0]], np.float32), np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], np.float32)):
        ref, _ = check(lib, cloud, 1.0)
        assert (ref['flags'] == R.FLAG_FEW).all()
        check(lib, cloud, 1.0, queries=np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 4.0], [100.0, 2.0, 3.0]], np.float32), viewpoint=(0.0, 0.0, 9.0))


@pytest.mark.parametrize('name', ['mixed', 'plane', 'lattice_plane', 'axis', 'diagonal', 'far'])
def test_clouds_and_degenerate_extents(lib, name):
    rng = np.random.default_rng(11)
    view = None
    if name == 'mixed':
        P, view = R.mixed(700, 1), (30.0, 30.0, 500.0)
    elif name == 'plane':
        P = R.mixed(600, 2)
        P[:, 2] = 3.0
    elif name == 'lattice_plane':
        g = np.arange(11, dtype=np.float64)
        P = np.stack(np.meshgrid(g, g, [7.0], indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    elif name == 'axis':
        P = np.zeros((400, 3), np.float32)
        P[:, 1] = rng.uniform(0.0, 300.0, 400)
    elif name == 'diagonal':
        P = (np.arange(-20, 21, dtype=np.float64)[:, None] * np.array([[1.0, 2.0, -1.0]])).astype(np.float32)
    else:
        P = R.mixed(600, 3, offset=1.0e6)                         # float32 steps of 1/16 out there
    for r in (3.0, 7.5, 1.0e5, 1.0e-4):                           # the last two: the whole cloud, and nothing but the point itself
        ref, _ = check(lib, P, r, viewpoint=view)
    if name == 'lattice_plane':
        ref, _ = check(lib, P, 3.0)
        assert ref['n'][60] == 29 and (ref['eigenvalues'][:, 2] == 0.0).all() and (ref['normal'] == [0.0, 0.0, 1.0]).all()


@pytest.mark.parametrize('where', ['faces', 'outside', 'at_points', 'inside'])
def test_cross_queries(lib, where):
    rng = np.random.default_rng(5)
    P = R.mixed(500, 4)
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
    ref, _ = check(lib, P, 6.0, queries=Q)
    if where == 'outside':
        assert (ref['flags'] == R.FLAG_EMPTY).all()
    check(lib, P, 40.0, queries=Q, viewpoint=(1000.0, -50.0, 20.0))
    check(lib, P, 12.0 * diag, queries=Q)                         # every neighbourhood is the whole cloud


def test_a_smaller_cell_tests_fewer_points(lib):
    P = R.mixed(1500, 8)
    _, seen = check(lib, P, 8.0)
    assert seen['fifth']['tests'] < seen['default']['tests'] < seen['widened']['tests'] < seen['one_cell']['tests']
    assert seen['fifth']['cells'] > seen['default']['cells'] > seen['one_cell']['cells']


def test_the_same_core_under_the_sanitizers(lib, tmp_path):
    """the shim with a main of its own, built with -fsanitize=address,undefined and run as a program: no report, and the same bytes"""
    exe = os.path.join(str(tmp_path), 'shim_san')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DNWF_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)])
    P = R.mixed(400, 9)
    far = (P[:50].astype(np.float64) * 30.0 + 500.0).astype(np.float32)
    runs = [(P, 4.0, None, None, None), (P, 6.5, None, (0.0, 0.0, 100.0), 0.7), (R.lattice(7), 2.0, None, None, 100.0), (P, 9.0, far, None, None),
            (P[:1], 1.0, P[:5], (1.0, 2.0, 3.0), None)]
    for k, (cloud, r, Q, view, h) in enumerate(runs):
        mine = shim_shape(lib, cloud, r, Q, view, h)
        pts, cstart, dims, box, n, Q32, r64, v64 = mine['blob']
        fin, fout = os.path.join(str(tmp_path), 'in%d.bin' % k), os.path.join(str(tmp_path), 'out%d.bin' % k)
        with open(fin, 'wb') as fh:
            fh.write(np.array([n, len(cstart) - 1, -1 if Q32 is None else len(Q32), 0 if v64 is None else 1], np.int64).tobytes())
            fh.write(box.tobytes() + dims.astype(np.int32).tobytes())
            fh.write(np.concatenate([[r64], np.zeros(3) if v64 is None else v64]).astype(np.float64).tobytes())
            fh.write(pts.tobytes() + cstart.tobytes())
            if Q32 is not None:
                fh.write(Q32.tobytes())
        res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        raw = open(fout, 'rb').read()
        nq = len(mine['flags'])
        assert int(np.frombuffer(raw, np.int32, 1)[0]) == 0
        at = 4
        assert np.array_equal(np.frombuffer(raw, np.int64, nq * 10, at).reshape(nq, 10), mine['moments'])
        at += 80 * nq
        assert np.frombuffer(raw, np.uint64, nq * 3, at).tolist() == mine['eigenvalues'].view(np.uint64).ravel().tolist()
        at += 24 * nq
        assert np.frombuffer(raw, np.uint64, nq * 9, at).tolist() == mine['vectors'].view(np.uint64).ravel().tolist()
        at += 72 * nq
        assert np.array_equal(np.frombuffer(raw, np.uint8, nq, at), mine['flags'])
        at += nq
        assert np.frombuffer(raw[at:], np.int64, 4).tolist() == [mine['tests'], mine['cells'], mine['neighbours'], mine['few']]
