"""
The geodesic graph distance, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_geodesic_core.h holds the weights, the diagonal rule, which
lane relaxes which arc, one relaxation and one label step as __host__ __device__ functions.  This test compiles them for the CPU
(g++ -ffp-contract=off) behind a shim of its own -- the device's kernels one half-edge after the other, the rounds serially, in a
half-edge order that the caller can reverse -- and asks for the restatement's (tests/mesh_geodesic_ref.py) distance and source bit for
bit on the meshes where floating point is most likely to differ.  The same source with a main of its own runs once under
-fsanitize=address,undefined, as a program.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_geodesic_ref as R
from conftest import ROOT
from ch_shrinkwrap_amd.trimesh import geodesic_sphere

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nw_geodesic_core.h"

// k_gd_weights, k_gd_seed, rounds of k_gd_relax, rounds of k_gd_labels and k_gd_finish, serially.  backwards: the half-edges are taken in
// descending order within a round (no output may depend on it).  rounds[0], rounds[1] = the rounds of the two loops -> 0, -1 for bad
// arguments, -2 if a loop did not end within nv + 1 rounds
extern "C" int shim_geodesic(const float *pos, long long nv, const int *faces, long long nf, const int *twin, int diagonals, const int *ids, const double *d0,
                             long long ns, double cap, int backwards, double *dist, int *src, double *we, double *wd, int *other, long long *rounds)
{
    if (!nwt_cap_ok(cap) || !nwt_sources_ok(ids, d0, ns, nv) || (twin && !nwt_twins_ok(faces, twin, nf)) || (diagonals && !twin)) return -1;
    const long long nh = 3 * nf;
    for (long long h = 0; h < nh; ++h) wd[h] = -1.0;          // (every slot must be written by the set-up)
    for (long long h = 0; h < nh; ++h) {
        const nwt_halfedge r = nwt_halfedge_setup(pos, faces, twin, h);
        we[h] = r.we;
        other[h] = r.other;
        if (r.wd_valid) { wd[h] = r.wd; wd[twin[h]] = r.wd; }
        else if (r.other == NWT_EDGE_ALONE) wd[h] = INFINITY;
    }
    for (long long h = 0; h < nh; ++h) if (wd[h] < 0.0) return -3;
    std::vector<double> D(nv, INFINITY);
    for (long long i = 0; i < ns; ++i) { const double s = nwt_start_value(d0 ? d0[i] : 0.0); if (s < D[ids[i]]) D[ids[i]] = s; }
    rounds[0] = rounds[1] = 0;
    for (bool changed = true; changed;) {
        if (++rounds[0] > nv + 1) return -2;
        changed = false;
        for (long long k = 0; k < nh; ++k) {
            const long long h = backwards ? nh - 1 - k : k;
            int p, q; double w, cand;
            if (!nwt_lane_arc(faces, other, we, wd, h, diagonals != 0, &p, &q, &w)) continue;
            if (nwt_relax(D[p], w, cap, D[q], &cand)) { D[q] = cand; changed = true; }
            if (nwt_relax(D[q], w, cap, D[p], &cand)) { D[p] = cand; changed = true; }
        }
    }
    std::vector<int> S(nv, NWT_LABEL_NONE);
    for (long long i = 0; i < ns; ++i)
        if (nwt_start_value(d0 ? d0[i] : 0.0) == D[ids[i]] && (int)i < S[ids[i]]) S[ids[i]] = (int)i;
    for (bool changed = true; changed;) {
        if (++rounds[1] > nv + 1) return -2;
        changed = false;
        for (long long k = 0; k < nh; ++k) {
            const long long h = backwards ? nh - 1 - k : k;
            int p, q; double w;
            if (!nwt_lane_arc(faces, other, we, wd, h, diagonals != 0, &p, &q, &w)) continue;
            if (nwt_tight(D[p], w, cap, D[q]) && S[p] < S[q]) { S[q] = S[p]; changed = true; }
            if (nwt_tight(D[q], w, cap, D[p]) && S[q] < S[p]) { S[p] = S[q]; changed = true; }
        }
    }
    for (long long v = 0; v < nv; ++v) {
        const bool in_band = D[v] < INFINITY && D[v] <= cap;
        dist[v] = in_band ? D[v] : INFINITY;
        src[v] = in_band && S[v] != NWT_LABEL_NONE ? S[v] : -1;
    }
    return 0;
}

extern "C" double shim_diagonal(const float *a, const float *b, const float *c, const float *d) { return nwt_diagonal_weight(a, b, c, d); }
extern "C" int shim_sources_ok(const int *ids, const double *d0, long long n, long long nv) { return nwt_sources_ok(ids, d0, n, nv) ? 1 : 0; }
extern "C" int shim_cap_ok(double cap) { return nwt_cap_ok(cap) ? 1 : 0; }
extern "C" int shim_twins_ok(const int *faces, const int *twin, long long nf) { return nwt_twins_ok(faces, twin, nf) ? 1 : 0; }

#ifdef NWT_MAIN
// the same call on arrays read from a file: 6 int64 (nv, nf, ns, diagonals, has twin, backwards), the cap, then pos, faces, twin, ids, d0
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 6);
    const double cap = rd<double>(fh, 1)[0];
    const auto pos = rd<float>(fh, 3 * c[0]);
    const auto faces = rd<int>(fh, 3 * c[1]);
    const auto twin = rd<int>(fh, c[4] ? 3 * c[1] : 0);
    const auto ids = rd<int>(fh, c[2]);
    const auto d0 = rd<double>(fh, c[2]);
    fclose(fh);
    std::vector<double> dist(c[0]), we(3 * c[1]), wd(3 * c[1]);
    std::vector<int> src(c[0]), other(3 * c[1]);
    long long rounds[2];
    const int r = shim_geodesic(pos.data(), c[0], faces.data(), c[1], c[4] ? twin.data() : nullptr, (int)c[3], ids.data(), d0.data(), c[2], cap, (int)c[5], dist.data(),
                                src.data(), we.data(), wd.data(), other.data(), rounds);
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(&r, sizeof(int), 1, fh);
    fwrite(dist.data(), sizeof(double), dist.size(), fh);
    fwrite(src.data(), sizeof(int), src.size(), fh);
    fclose(fh);
    return 0;
}
#endif
'''

p = lambda a: None if a is None else a.ctypes.data
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _source(tmp):
    src = os.path.join(str(tmp), 'shim.cpp')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    return src


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwt_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwt_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f64, ll, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_longlong, ctypes.c_int
    L.shim_geodesic.argtypes = [vp, ll, vp, ll, vp, i32, vp, vp, ll, f64, i32, vp, vp, vp, vp, vp, vp]
    L.shim_diagonal.argtypes = [vp] * 4
    L.shim_diagonal.restype = f64
    L.shim_sources_ok.argtypes = [vp, vp, ll, ll]
    L.shim_cap_ok.argtypes = [f64]
    L.shim_twins_ok.argtypes = [vp, vp, ll]
    return L


def shim(lib, V, F, ids, d0=None, cap=np.inf, diagonals=True, backwards=False):
    V, F = R.mesh32(V, F)
    twin = R.twins(F) if diagonals else None
    ids = np.ascontiguousarray(ids, np.int32)
    d0 = None if d0 is None else np.ascontiguousarray(d0, np.float64)
    nh = 3 * F.shape[0]
    dist, src = np.full(V.shape[0], -7.0), np.full(V.shape[0], -7, np.int32)
    we, wd, other, rounds = np.zeros(nh), np.zeros(nh), np.zeros(nh, np.int32), np.zeros(2, np.int64)
    r = lib.shim_geodesic(p(V), V.shape[0], p(F), F.shape[0], p(twin), int(diagonals), p(ids), p(d0), ids.size, float(cap), int(backwards), p(dist), p(src),
                          p(we), p(wd), p(other), p(rounds))
    assert r == 0, r
    return dict(distance=dist, source=src, we=we, wd=wd, other=other, rounds=rounds, blob=(V, F, twin, ids, d0, float(cap), int(diagonals), int(backwards)))


def check(lib, V, F, ids, d0=None, cap=np.inf):
    """the restatement's bits, with and without diagonals, the half-edges forwards and backwards"""
    out = {}
    for diag in (True, False):
        ref = R.geodesic(V, F, ids, d0, max_distance=cap, diagonals=diag)
        for back in (False, True):
            mine = shim(lib, V, F, ids, d0, cap, diag, back)
            assert (bits(mine['distance']) == bits(ref['distance'])).all(), (diag, back)
            assert (mine['source'] == ref['source']).all(), (diag, back)
        if diag:                                              # every diagonal the restatement has, with its bits, in two slots
            wd = mine['wd'][np.isfinite(mine['wd'])]
            want = R.diagonals(V, F, R.twins(F))[2]
            assert np.array_equal(np.sort(bits(wd)), np.sort(bits(np.repeat(want, 2))))
        out[diag] = ref
    return out


def _sphere(seed, n=4, radius=20.0, noise=0.5):
    V, F = geodesic_sphere(n, radius)
    return (V + np.random.default_rng(seed).normal(scale=noise, size=V.shape)).astype(np.float32), F


def test_a_sphere_and_its_sources(lib):
    V, F = _sphere(1)
    check(lib, V, F, [0])
    check(lib, V, F, [5, 100, 5, 60], [0.0, 1.5, 0.25, 40.0])
    check(lib, V, F, np.arange(V.shape[0]))
    d = np.sort(R.geodesic(V, F, [0])['distance'])
    check(lib, V, F, [0], cap=d[50])
    check(lib, V, F, [0], cap=np.nextafter(d[50], 0.0))


def test_needles_of_aspect_ten_thousand(lib):
    V, F = R.grid_mesh(40, 5, dx=1.0e4, dy=1.0)
    V = (V + np.random.default_rng(2).normal(scale=0.05, size=V.shape)).astype(np.float32)
    check(lib, V, F, [0, 199])
    V, F = R.grid_mesh(5, 40, dx=1.0e-2, dy=1.0e2)
    check(lib, V, F, [7], [3.0])


def test_zero_length_edges_and_flat_faces(lib):
    V, F = _sphere(3)
    V[F[::7, 1]] = V[F[::7, 0]]                               # duplicate positions: zero-weight arcs and cycles of them, flat faces
    ref = check(lib, V, F, [0, 33])
    assert (R.arcs(V, F)[2] == 0).sum() > 10
    assert len(np.unique(ref[True]['distance'])) < V.shape[0] - 10
    V, F = R.grid_mesh(9, 9)
    V[:, 1] = 0.0                                             # every face flat: no diagonal exists
    ref = check(lib, V, F, [4])
    assert (bits(ref[True]['distance']) == bits(ref[False]['distance'])).all()
    V, F = R.grid_mesh(6, 6)
    V[:] = V[0]                                               # one point
    ref = check(lib, V, F, [3, 1])
    assert (ref[True]['distance'] == 0).all() and (ref[True]['source'] == 0).all()


def test_far_from_the_origin(lib):
    V, F = _sphere(4, radius=40.0, noise=1.0)
    V = (V.astype(np.float64) + 1.0e6).astype(np.float32)     # float32 steps of 1/16 out there
    check(lib, V, F, [0, 77], [0.0, 5.0])


def _hinges(n, seed):
    """n random two-face hinges in one mesh, in arbitrary planes: a, b, c on one side, d on the other or not"""
    rng = np.random.default_rng(seed)
    V = np.zeros((4 * n, 3))
    for k in range(n):
        a, e = rng.normal(scale=10.0, size=3), rng.normal(size=3)
        n1, n2 = np.cross(e, rng.normal(size=3)), np.cross(e, rng.normal(size=3))
        V[4 * k], V[4 * k + 1] = a, a + e
        V[4 * k + 2] = a + rng.uniform(-1.0, 2.0) * e + rng.uniform(0.0, 2.0) * n1
        V[4 * k + 3] = a + rng.uniform(-1.0, 2.0) * e + rng.uniform(0.0, 2.0) * n2
    base = 4 * np.arange(n)[:, None]
    F = np.concatenate([base + [0, 1, 2], base + [1, 0, 3]]).astype(np.int32)
    return V.astype(np.float32), F


def test_a_thousand_hinges_and_the_ends_of_the_edge(lib):
    V, F = _hinges(1000, 8)
    ref = check(lib, V, F, np.arange(2, 4000, 4))             # from every c
    n_diag = R.diagonals(V, F, R.twins(F))[2].size
    assert 200 < n_diag < 800                                 # both outcomes of the rule are well represented
    # the crossing point 2^-50 from the end a of the edge, on it, and 2^-50 beyond it; 2^-25 from the end b, and on it
    a, b, c = [0, 0, 0], [1, 0, 0], [0, 1, 0]
    f = lambda *v: [np.array(x, np.float32) for x in v]
    diag = lambda *v: lib.shim_diagonal(*[p(x) for x in f(*v)])
    assert diag(a, b, c, [2.0 ** -49, -1, 0]) == np.sqrt(2.0 ** -98 + 4.0)
    assert diag(a, b, c, [0, -1, 0]) == np.inf and diag(a, b, c, [-2.0 ** -49, -1, 0]) == np.inf
    assert np.isfinite(diag(a, b, [1, 1, 0], [1 - 2.0 ** -24, -1, 0])) and diag(a, b, [1, 1, 0], [1, -1, 0]) == np.inf
    assert diag(a, b, [0.5, 0, 0], [0.5, -1, 0]) == np.inf and diag(a, b, [0.5, 1, 0], [0.25, 0, 0]) == np.inf        # a flat face
    assert diag(a, a, c, [0.5, -1, 0]) == np.inf                                                                       # an edge without length
    for case in ([2.0 ** -49, -1, 0], [0, -1, 0], [-2.0 ** -49, -1, 0]):
        Vh = np.array([a, b, c, case], np.float32)
        check(lib, Vh, np.array([[0, 1, 2], [1, 0, 3]], np.int32), [2])


def test_the_argument_rules(lib):
    ids, d0 = np.array([0, 3, 3], np.int32), np.array([0.0, 1.0, 2.0])
    ok = lambda i, d, n=None, nv=5: lib.shim_sources_ok(p(i), p(d), len(i) if n is None else n, nv)
    assert ok(ids, d0) == 1 and ok(ids, None) == 1 and ok(ids, d0, nv=-1) == 1
    assert ok(ids, d0, n=0) == 0 and ok(ids, d0, n=(1 << 30) + 1) == 0 and lib.shim_sources_ok(None, None, 3, 5) == 0
    assert ok(np.array([0, 5], np.int32), None) == 0 and ok(np.array([-1], np.int32), None, nv=-1) == 0
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        assert ok(ids, np.array([0.0, bad, 1.0])) == 0
    assert ok(ids, np.array([0.0, -0.0, 1.0])) == 1
    assert [lib.shim_cap_ok(c) for c in (1.0, np.inf, 5e-324, 0.0, -1.0, np.nan, -np.inf)] == [1, 1, 1, 0, 0, 0, 0]
    V, F = geodesic_sphere(2, 1.0)
    twin = R.twins(F)
    assert lib.shim_twins_ok(p(F), p(twin), F.shape[0]) == 1
    for h, t in ((4, 3 * F.shape[0]), (4, -2), (4, 4), (4, twin[5])):
        bad = twin.copy()
        bad[h] = t
        assert lib.shim_twins_ok(p(F), p(bad), F.shape[0]) == 0
    # -0.0 as a start value is +0.0
    r = shim(lib, V, F, [0], [-0.0])
    assert bits(r['distance'][0:1])[0] == 0


def test_the_same_core_under_the_sanitizers(lib, tmp_path):
    """the shim with a main of its own, built with -fsanitize=address,undefined and run as a program: no report, and the same bytes"""
    exe = os.path.join(str(tmp_path), 'shim_san')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DNWT_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)])
    V, F = _sphere(5)
    Vh, Fh = _hinges(50, 9)
    Vb, Fb = R.grid_mesh(7, 3)
    runs = [(V, F, [0], None, np.inf, True, False), (V, F, [3, 9, 3], [0.0, 2.0, 1.0], 25.0, True, True), (V, F, [1], None, np.inf, False, False),
            (Vh, Fh, np.arange(2, 200, 4), None, np.inf, True, False), (Vb, Fb, [20], [1.0], 3.5, True, True)]
    for k, (V_, F_, ids, d0, cap, diag, back) in enumerate(runs):
        mine = shim(lib, V_, F_, ids, np.zeros(len(ids)) if d0 is None else d0, cap, diag, back)
        V32, F32, twin, ids32, d064, cap_, diag_, back_ = mine['blob']
        fin, fout = os.path.join(str(tmp_path), 'in%d.bin' % k), os.path.join(str(tmp_path), 'out%d.bin' % k)
        with open(fin, 'wb') as fh:
            fh.write(np.array([V32.shape[0], F32.shape[0], ids32.size, diag_, 0 if twin is None else 1, back_], np.int64).tobytes())
            fh.write(np.array([cap_]).tobytes() + V32.tobytes() + F32.tobytes() + (b'' if twin is None else twin.tobytes()) + ids32.tobytes() + d064.tobytes())
        res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        raw = open(fout, 'rb').read()
        nv = V32.shape[0]
        assert int(np.frombuffer(raw, np.int32, 1)[0]) == 0
        assert np.array_equal(np.frombuffer(raw, np.uint64, nv, 4), bits(mine['distance']))
        assert np.array_equal(np.frombuffer(raw, np.int32, nv, 4 + 8 * nv), mine['source'])
