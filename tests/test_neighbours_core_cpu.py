"""
The k-th-neighbour query's rules, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_neighbours_core.h holds the squared distance, the list
of the k best, the ring bound and the quantisation as __host__ __device__ functions; this test compiles them for the CPU
(g++ -ffp-contract=off) behind a shim of its own and asks for the bits of the NumPy restatement (tests/neighbours_ref.py).  The same
functions also run in a stand-alone program under the address and undefined-behaviour sanitizers.  Both are built on demand in pytest's
temporary directory.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from ch_shrinkwrap_amd import neighbours     # noqa: F401  (the unit under test: without it there is nothing to restate)
import neighbours_ref as R
from conftest import ROOT

CORE = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_neighbours_core.h')

SHIM = r'''
#include "nw_neighbours_core.h"
extern "C" {
// the list after every insertion: slots at `stride` doubles apart inside rows of k * stride (unused slots keep their nan)
void shim_list_trace(const double *d2, long long n, int k, int stride, double *rows, int *cnt, int *at, double *mx)
{
    double s[NWK_CORE_MAX_K * 4];
    for (int j = 0; j < NWK_CORE_MAX_K * 4; ++j) s[j] = NAN;
    nwk_list L;
    nwk_list_init(&L);
    for (long long i = 0; i < n; ++i) {
        nwk_list_insert(s, stride, k, &L, d2[i]);
        for (int j = 0; j < k; ++j) rows[i * k + j] = s[j * stride];
        cnt[i] = L.cnt; at[i] = L.at; mx[i] = L.mx;
    }
}
// brute force through the list: min(r_k, r_cap) and its quantisation at float64 positions
void shim_kth(const float *p, long long n, const double *x, long long nx, int k, double r_cap, double *r_out, unsigned long long *q_out)
{
    for (long long i = 0; i < nx; ++i) {
        double s[NWK_CORE_MAX_K];
        nwk_list L;
        nwk_list_init(&L);
        for (long long j = 0; j < n; ++j) nwk_list_insert(s, 1, k, &L, nwk_dist2(p[3 * j], p[3 * j + 1], p[3 * j + 2], x[3 * i], x[3 * i + 1], x[3 * i + 2]));
        r_out[i] = nwk_result(nwk_list_kth(&L, k), r_cap);
        q_out[i] = std::isfinite(r_cap) ? nwk_quantise(r_out[i], r_cap) : 0ull;
    }
}
double shim_node_coord(float lo, float h, int index) { return nwk_node_coord(lo, h, index); }
double shim_ring_lbd(int r, double h) { return nwk_ring_lbd(r, h); }
int shim_walk_ends(int r, double h, double out2, int cnt, double mx, int k, double cap2)
{
    nwk_list L;
    L.cnt = cnt; L.at = 0; L.mx = mx;
    return nwk_walk_ends(r, h, out2, &L, k, cap2) ? 1 : 0;
}
double shim_cell_slack(void) { return NWK_CELL_SLACK; }
}
'''

MAIN = r'''
#include <cstdio>
#include <vector>
#include "nw_neighbours_core.h"
// every k, lists in columns of a shared array as on the device ([slot][lane]), more candidates than slots, ties and duplicates
int main()
{
    const int lanes = 7;
    unsigned long long state = 12345, checks = 0;
    for (int k = 1; k <= NWK_CORE_MAX_K; ++k) {
        std::vector<double> s((size_t)k * lanes, -7.0);
        std::vector<nwk_list> L(lanes);
        std::vector<std::vector<double>> seen(lanes);
        for (int l = 0; l < lanes; ++l) nwk_list_init(&L[l]);
        for (int i = 0; i < 200; ++i)
            for (int l = 0; l < lanes; ++l) {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                const double d2 = (double)((state >> 33) % 50);                          // few values: many ties
                nwk_list_insert(s.data() + l, lanes, k, &L[l], d2);
                seen[l].push_back(d2);
            }
        for (int l = 0; l < lanes; ++l) {
            std::vector<double> v = seen[l];
            std::sort(v.begin(), v.end());
            if (nwk_list_kth(&L[l], k) != v[k - 1]) { std::printf("k %d lane %d: %g, expected %g\n", k, l, nwk_list_kth(&L[l], k), v[k - 1]); return 1; }
            ++checks;
        }
    }
    if (nwk_quantise(nwk_result(INFINITY, 40.0), 40.0) != 0ull || nwk_quantise(0.0, 1099511627776.0) != (1ull << 60)) return 2;
    std::printf("ok %llu\n", checks);
    return 0;
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('nwk_shim'))
    src, lib = os.path.join(d, 'shim.cpp'), os.path.join(d, 'libnwk_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', os.path.dirname(CORE),
                           '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp, ll, i32, f64 = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double
    L.shim_list_trace.argtypes = [vp, ll, i32, i32, vp, vp, vp, vp]
    L.shim_list_trace.restype = None
    L.shim_kth.argtypes = [vp, ll, vp, ll, i32, f64, vp, vp]
    L.shim_kth.restype = None
    L.shim_node_coord.argtypes = [ctypes.c_float, ctypes.c_float, i32]
    L.shim_node_coord.restype = f64
    L.shim_ring_lbd.argtypes = [i32, f64]
    L.shim_ring_lbd.restype = f64
    L.shim_walk_ends.argtypes = [i32, f64, f64, i32, f64, i32, f64]
    L.shim_walk_ends.restype = i32
    L.shim_cell_slack.argtypes = []
    L.shim_cell_slack.restype = f64
    return L


def _kth(L, points, x, k, r_cap):
    p = np.ascontiguousarray(points, np.float32)
    x = np.ascontiguousarray(x, np.float64).reshape(-1, 3)
    r, q = np.empty(x.shape[0]), np.empty(x.shape[0], np.uint64)
    L.shim_kth(p.ctypes.data, p.shape[0], x.ctypes.data, x.shape[0], int(k), float(r_cap), r.ctypes.data, q.ctypes.data)
    return r, q


@pytest.mark.parametrize('k', [1, 2, 20, 31, 32])
@pytest.mark.parametrize('stride', [1, 3])
def test_list_update_gives_the_restatements_bits(shim, k, stride):
    rng = np.random.default_rng(k)
    d2 = np.concatenate([rng.uniform(0, 100, 150), rng.integers(0, 12, 150).astype(np.float64), [0.0, 0.0, 5.0, 5.0]])     # real values, ties, zeros
    rng.shuffle(d2)
    n = d2.size
    rows, cnt, at, mx = np.empty((n, k)), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n)
    shim.shim_list_trace(d2.ctypes.data, n, k, stride, rows.ctypes.data, cnt.ctypes.data, at.ctypes.data, mx.ctypes.data)
    ref_rows, ref_cnt, ref_at, ref_mx = R.list_trace(d2, k)
    assert np.array_equal(rows.view(np.uint64), ref_rows.view(np.uint64))
    assert np.array_equal(cnt, ref_cnt) and np.array_equal(at, ref_at) and np.array_equal(mx.view(np.uint64), ref_mx.view(np.uint64))
    # what the list is for: once full, its largest value is the k-th smallest of everything seen
    for i in range(k - 1, n, 17):
        assert mx[i] == np.sort(d2[:i + 1])[k - 1]


def test_brute_force_through_the_list_equals_the_restatement(shim):
    pts = R.random_cloud(700, 1)
    x = R.queries_around(pts, 300, 2).astype(np.float64) + 1e-3                   # float64 positions that are no float32 numbers
    for k, r_cap in ((1, np.inf), (20, np.inf), (32, 150.0), (20, 60.0)):
        r, q = _kth(shim, pts, x, k, r_cap)
        ref = R.kth_at(pts, x, k, r_cap)
        assert np.array_equal(r.view(np.uint64), ref.view(np.uint64))
        if np.isfinite(r_cap):
            assert np.array_equal(q, R.quantise(ref, r_cap)) and (ref == r_cap).any() and (ref < r_cap).any()
    # fewer points than k: the cap, whatever it is
    r, _ = _kth(shim, pts[:5], x[:4], 6, np.inf)
    assert np.isinf(r).all()
    r, q = _kth(shim, pts[:5], x[:4], 6, 12.5)
    assert (r == 12.5).all() and (q == 0).all()


def test_quantisation_and_node_coordinates(shim):
    p, lo, h, dims, index = R.coincident_node_case()
    x = R.node_positions(lo, h, dims)
    nodes = x.reshape(dims[2], dims[1], dims[0], 3)
    for a in range(3):
        for i in (0, 1, int(dims[a]) - 1):
            at = [0, 0, 0]
            at[a] = i
            assert shim.shim_node_coord(float(lo[a]), float(h), i) == nodes[at[2], at[1], at[0], a]
    lo2, h2 = np.float32(5e3), np.float32(7.3)                                       # (h is no float64-exact multiple here)
    assert shim.shim_node_coord(lo2, h2, 69) == float(lo2) + 69.5 * float(h2)
    r, q = _kth(shim, p, x, 3, 9.0)
    ref = R.node_field(p, lo, h, dims, 3, 9.0)
    assert np.array_equal(q.reshape(ref.shape), ref)
    r1, q1 = _kth(shim, p, x, 1, 9.0)
    assert r1.reshape(ref.shape)[index[2], index[1], index[0]] == 0.0 and q1.reshape(ref.shape)[index[2], index[1], index[0]] == 9 << 20
    # the largest cap the field takes
    assert _kth(shim, p[:1], p[:1].astype(np.float64), 1, 2.0 ** 40)[1][0] == 1 << 60


def test_ring_bound_and_the_end_of_the_walk(shim):
    slack = shim.shim_cell_slack()
    # float32 cells: two roundings of 2^-24 on a coordinate of at most 1025 cells, and the bound gives away more than twice that
    assert slack >= 2 * (2 * 2.0 ** -24 * 1025)
    h = 12.5
    assert shim.shim_ring_lbd(0, h) == 0.0 and shim.shim_ring_lbd(1, h) == 0.0
    for r in (2, 3, 10, 1025):
        lbd = shim.shim_ring_lbd(r, h)
        assert lbd == ((r - 1) - slack) * h * (1.0 - 1e-9) and lbd < (r - 1) * h
    k = 20
    # the k-th best is +inf until k candidates are held: only the cap can end the walk
    assert not shim.shim_walk_ends(50, h, 0.0, k - 1, 1.0, k, np.inf)
    assert shim.shim_walk_ends(50, h, 0.0, k - 1, 1.0, k, 100.0 ** 2)
    # strict: a ring whose bound equals the k-th best is still walked, so equally near points are all seen
    lbd = shim.shim_ring_lbd(3, h)
    assert not shim.shim_walk_ends(3, h, 0.0, k, lbd * lbd, k, np.inf)
    assert shim.shim_walk_ends(3, h, 0.0, k, np.nextafter(lbd * lbd, 0.0), k, np.inf)
    assert not shim.shim_walk_ends(3, h, 0.0, k, 1e9, k, lbd * lbd) and shim.shim_walk_ends(3, h, 0.0, k, 1e9, k, np.nextafter(lbd * lbd, 0.0))
    # a query outside the box: its distance from the box counts
    assert shim.shim_walk_ends(0, h, 101.0, k, 100.0, k, np.inf) and not shim.shim_walk_ends(0, h, 100.0, k, 100.0, k, np.inf)


def test_core_under_the_sanitizers_in_a_program_of_its_own(tmp_path):
    src, exe = str(tmp_path / 'main.cpp'), str(tmp_path / 'nwk_core_main')
    with open(src, 'w') as fh:
        fh.write('#include <algorithm>\n' + MAIN)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', os.path.dirname(CORE), '-o', exe, src])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and out.stdout.decode().startswith('ok %d' % (32 * 7)), out.stdout.decode()
