"""
The level-set skeleton, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_skeleton_core.h holds the band rule, the piece index, the edge's
band range, the crossing point, the quantisation and a piece's terms as __host__ __device__ functions.  This test compiles them for the
CPU (g++ -ffp-contract=off) behind a shim of its own -- the device's kernels one lane after the other, in an order that the caller can
reverse -- and asks for the restatement's (tests/mesh_skeleton_ref.py) tables bit for bit on the meshes where floating point is most
likely to differ.  The same source with a main of its own runs once under -fsanitize=address,undefined, as a program.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_skeleton_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "nw_skeleton_core.h"

typedef unsigned long long u64;

static int find(std::vector<int> &parent, int v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; }

// k_sk_bands, the scan, k_sk_init, k_sk_hook, k_sk_compress, the ranks, k_sk_number, k_sk_sums, k_sk_arcs and k_sk_vertex, serially.
// backwards: half-edges and pieces are taken in descending order (no output may depend on it).  sizes = P, N, A.
// -> 0, -1 for bad arguments, -2 if cap is too small (sizes are then set)
extern "C" int shim_skeleton(const float *pos, long long nv, const int *faces, long long nf, const int *twin, const double *D, double w, int backwards, long long cap,
                             int *piece_start, int *piece_node, int *vertex_node, int *node_band, u64 *sums, int *arcs, long long *sizes, double *quantum)
{
    double low[3], q;
    if (!nwa_width_ok(w) || !nwa_twins_ok(faces, twin, nf) || !nwa_field_ok(D, nv, w) || !nwa_box(pos, nv, low, &q)) return -1;
    quantum[0] = low[0]; quantum[1] = low[1]; quantum[2] = low[2]; quantum[3] = q;
    std::vector<int> band(nv), lo(nf), span(nf);
    bool bad = false;
    for (long long v = 0; v < nv; ++v) band[v] = nwa_band(D[v], w, &bad);
    long long total = 0;
    for (long long f = 0; f < nf; ++f) {
        const nwa_face_bands fb = nwa_face(band[faces[3 * f]], band[faces[3 * f + 1]], band[faces[3 * f + 2]]);
        lo[f] = fb.lo; span[f] = fb.span;
        piece_start[f] = (int)total;
        total += fb.span;
        if (total > NWA_MAX_PIECES) return -1;
    }
    piece_start[nf] = (int)total;
    const int np = (int)total;
    sizes[0] = np; sizes[1] = sizes[2] = 0;
    if (np > cap) return -2;
    std::vector<int> parent(np), piece_face(np);
    for (int p = 0; p < np; ++p) { parent[p] = p; piece_face[p] = nwa_piece_face(piece_start, (int)nf, p); }
    const long long nh = 3 * nf;
    for (long long i = 0; i < nh; ++i) {
        const long long h = backwards ? nh - 1 - i : i, t = twin[h], f = h / 3, g = t / 3;
        if (!(t > h && span[f] > 0 && span[g] > 0)) continue;
        int k0, k1;
        nwa_edge_range(band[faces[h]], band[faces[nwa_next(h)]], &k0, &k1);
        for (int k = k0; k <= k1; ++k) {
            int a = find(parent, piece_start[f] - lo[f] + k), b = find(parent, piece_start[g] - lo[g] + k);
            if (a == b) continue;
            if (a > b) std::swap(a, b);
            parent[b] = a;
        }
    }
    std::vector<int> rank(np);
    int nn = 0;
    for (int p = 0; p < np; ++p) rank[p] = find(parent, p) == p ? nn++ : -1;
    sizes[1] = nn;
    for (int p = 0; p < np; ++p) {
        const int r = find(parent, p);
        piece_node[p] = rank[r];
        if (r == p) node_band[rank[r]] = lo[piece_face[p]] + (p - piece_start[piece_face[p]]);
    }
    for (long long i = 0; i < (long long)nn * NWA_S_COLUMNS; ++i) sums[i] = 0;
    std::vector<u64> keys;
    for (int i = 0; i < np; ++i) {
        const int p = backwards ? np - 1 - i : i, f = piece_face[p], k = lo[f] + (p - piece_start[f]);
        u64 add[NWA_S_COLUMNS];
        nwa_piece_terms(pos, D, faces + 3 * (long long)f, k, w, low, q, add);
        for (int c = 0; c < NWA_S_COLUMNS; ++c) sums[(long long)piece_node[p] * NWA_S_COLUMNS + c] += add[c];
        if (p + 1 < piece_start[f + 1]) keys.push_back(nwa_arc_key(piece_node[p], piece_node[p + 1]));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    sizes[2] = (long long)keys.size();
    if ((long long)keys.size() > cap) return -2;
    for (size_t i = 0; i < keys.size(); ++i) { arcs[2 * i] = (int)(keys[i] >> 32); arcs[2 * i + 1] = (int)(keys[i] & 0xffffffffull); }
    for (long long v = 0; v < nv; ++v) vertex_node[v] = -1;
    for (long long i = 0; i < nh; ++i) {
        const long long h = backwards ? nh - 1 - i : i, f = h / 3;
        if (span[f] <= 0) continue;
        const int v = faces[h], n = piece_node[piece_start[f] + (band[v] - lo[f])];
        if (vertex_node[v] < 0 || n < vertex_node[v]) vertex_node[v] = n;
    }
    return 0;
}

extern "C" int shim_band(double D, double w, int *bad) { bool b = false; const int r = nwa_band(D, w, &b); *bad = b ? 1 : 0; return r; }
extern "C" double shim_quantum(double e) { return nwa_quantum(e); }
extern "C" int shim_width_ok(double w) { return nwa_width_ok(w) ? 1 : 0; }
extern "C" int shim_twins_ok(const int *faces, const int *twin, long long nf) { return nwa_twins_ok(faces, twin, nf) ? 1 : 0; }

#ifdef NWA_MAIN
// the same call on arrays read from a file: 4 int64 (nv, nf, backwards, cap), w, then pos, faces, twin, D
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 4);
    const double w = rd<double>(fh, 1)[0];
    const auto pos = rd<float>(fh, 3 * c[0]);
    const auto faces = rd<int>(fh, 3 * c[1]);
    const auto twin = rd<int>(fh, 3 * c[1]);
    const auto D = rd<double>(fh, c[0]);
    fclose(fh);
    const long long cap = c[3];
    std::vector<int> piece_start(c[1] + 1), piece_node(cap), vertex_node(c[0]), node_band(cap), arcs(2 * cap);
    std::vector<u64> sums(cap * NWA_S_COLUMNS);
    long long sizes[3];
    double quantum[4];
    const int r = shim_skeleton(pos.data(), c[0], faces.data(), c[1], twin.data(), D.data(), w, (int)c[2], cap, piece_start.data(), piece_node.data(),
                                vertex_node.data(), node_band.data(), sums.data(), arcs.data(), sizes, quantum);
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(&r, sizeof(int), 1, fh);
    if (r == 0) {
        fwrite(sizes, sizeof(long long), 3, fh);
        fwrite(piece_start.data(), sizeof(int), piece_start.size(), fh);
        fwrite(piece_node.data(), sizeof(int), sizes[0], fh);
        fwrite(vertex_node.data(), sizeof(int), vertex_node.size(), fh);
        fwrite(node_band.data(), sizeof(int), sizes[1], fh);
        fwrite(sums.data(), sizeof(u64), sizes[1] * NWA_S_COLUMNS, fh);
        fwrite(arcs.data(), sizeof(int), 2 * sizes[2], fh);
    }
    fclose(fh);
    return 0;
}
#endif
'''

p = lambda a: None if a is None else a.ctypes.data
KEYS = ('piece_start', 'piece_node', 'vertex_node', 'node_band', 'node_sums', 'arcs')


def _source(tmp):
    src = os.path.join(str(tmp), 'shim.cpp')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    return src


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwa_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwa_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f64, ll, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_longlong, ctypes.c_int
    L.shim_skeleton.argtypes = [vp, ll, vp, ll, vp, vp, f64, i32, ll] + [vp] * 8
    L.shim_band.argtypes = [f64, f64, vp]
    L.shim_quantum.argtypes = [f64]
    L.shim_quantum.restype = f64
    L.shim_width_ok.argtypes = [f64]
    L.shim_twins_ok.argtypes = [vp, vp, ll]
    return L


def shim(lib, V, F, D, w, backwards=False, twin=None, cap=None, expect=0):
    V, F = R.mesh32(V, F)
    twin = R.twins(F) if twin is None else twin
    D = np.ascontiguousarray(D, np.float64)
    nv, nf = V.shape[0], F.shape[0]
    cap = 1 << 18 if cap is None else cap
    out = dict(piece_start=np.full(nf + 1, -7, np.int32), piece_node=np.full(cap, -7, np.int32), vertex_node=np.full(nv, -7, np.int32),
               node_band=np.full(cap, -7, np.int32), node_sums=np.zeros((cap, 12), np.uint64), arcs=np.full((cap, 2), -7, np.int32))
    sizes, quantum = np.zeros(3, np.int64), np.zeros(4)
    r = lib.shim_skeleton(p(V), nv, p(F), nf, p(twin), p(D), float(w), int(backwards), cap, p(out['piece_start']), p(out['piece_node']), p(out['vertex_node']),
                          p(out['node_band']), p(out['node_sums']), p(out['arcs']), p(sizes), p(quantum))
    assert r == expect, r
    if r != 0:
        return sizes
    P, N, A = [int(x) for x in sizes]
    out.update(piece_node=out['piece_node'][:P], node_band=out['node_band'][:N], node_sums=out['node_sums'][:N], arcs=out['arcs'][:A], low=quantum[:3].copy(),
               q=float(quantum[3]), blob=(V, F, twin, D, float(w)))
    return out


def same(mine, ref):
    for k in KEYS:
        assert mine[k].dtype == ref[k].dtype and mine[k].shape == ref[k].shape, k
        assert mine[k].tobytes() == ref[k].tobytes(), k
    assert mine['low'].tobytes() == np.asarray(ref['low'], np.float64).tobytes() and mine['q'] == ref['q']


def check(lib, V, F, D, w):
    """the restatement's bytes, lanes forwards and backwards"""
    ref = R.level_sets(V, F, D, w)
    for back in (False, True):
        same(shim(lib, V, F, D, w, back), ref)
    return ref


def _random_soup(n, seed, scale=10.0):
    """n random faces over a random cloud, glued into a manifold (with borders) by keeping only faces that do not repeat a half-edge"""
    rng = np.random.default_rng(seed)
    nv = n // 2 + 3
    V = rng.normal(scale=scale, size=(nv, 3)).astype(np.float32)
    seen, F = set(), []
    while len(F) < n:
        f = rng.choice(nv, 3, replace=False)
        he = [(int(f[k]), int(f[(k + 1) % 3])) for k in range(3)]
        if any(e in seen for e in he):
            continue
        seen.update(he)
        F.append(f)
    return V, np.array(F, np.int32)


def test_tube_torus_and_their_widths(lib):
    V, F = R.tube_mesh()
    for w in (1.3, 0.5, 0.07):
        check(lib, V, F, V[:, 2].astype(np.float64) + 0.011, w)
    V, F = R.torus_mesh()
    D = V[:, 0].astype(np.float64) * np.cos(0.3) + V[:, 1] * np.sin(0.3)
    for w in (2.0, 0.05):
        assert R.graph_numbers(check(lib, V, F, D - D.min() + 0.0123, w))[3] == 1


def test_needles_of_aspect_ten_thousand(lib):
    rng = np.random.default_rng(2)
    V, F = R.strip_mesh(200, dx=1.0e4, dy=1.0)
    V = (V + rng.normal(scale=0.05, size=V.shape)).astype(np.float32)
    check(lib, V, F, V[:, 0].astype(np.float64) * 1.0e-3 + V[:, 1], 0.37)
    check(lib, V, F, rng.uniform(0, 50, V.shape[0]), 1.7)
    V, F = R.strip_mesh(200, dx=1.0e-2, dy=1.0e2)
    check(lib, V, F, V[:, 1].astype(np.float64) + V[:, 0], 3.3)


def test_far_from_the_origin(lib):
    V, F = R.torus_mesh()
    V = (V.astype(np.float64) + 1.0e6).astype(np.float32)         # float32 steps of 1/16 out there
    D = V[:, 0].astype(np.float64) - float(V[:, 0].min()) + 0.0123
    ref = check(lib, V, F, D, 0.25)
    extent = float((V.max(0).astype(np.float64) - V.min(0)).max())
    assert 2 ** 19 <= extent / ref['q'] < 2 ** 20 and (ref['low'] > 9.9e5).all()     # the quantum follows the extent, not the offset
    check(lib, V, F, R.edge_dijkstra(V, F, 5), 0.4)


def test_zero_length_edges_and_flat_fields(lib):
    V, F = R.torus_mesh()
    V = V.copy()
    V[F[::7, 1]] = V[F[::7, 0]]                                   # duplicate positions: faces without area, segments without length
    D = R.edge_dijkstra(V, F, 0)
    assert (np.diff(np.sort(D)) == 0).sum() > 10
    check(lib, V, F, D, 0.5)
    check(lib, V, F, np.zeros(V.shape[0]), 1.0)                   # one band, no contour anywhere
    V[:] = V[0]                                                   # one point: extent 0, q = 1
    ref = check(lib, V, F, np.arange(V.shape[0], dtype=np.float64), 2.5)
    assert ref['q'] == 1.0 and ref['node_sums'][:, R.S_LENGTH].sum() == 0 and ref['node_sums'][:, R.S_SEGMENTS].sum() > 0


def test_one_face_spanning_a_thousand_bands(lib):
    V, F = R.strip_mesh(9)
    D = np.arange(V.shape[0], dtype=np.float64) * 0.5
    D[4] = 1000.3
    ref = check(lib, V, F, D, 1.0)
    span = np.diff(ref['piece_start'])
    assert span.max() >= 1000 and span.min() <= 2
    assert R.graph_numbers(ref)[2:] == (1, 0)


def test_a_thousand_random_faces_with_random_fields(lib):
    V, F = _random_soup(1000, 8)
    rng = np.random.default_rng(9)
    check(lib, V, F, rng.uniform(0, 30, V.shape[0]), 1.0)
    D = rng.uniform(-2, 30, V.shape[0])
    D[rng.integers(0, V.shape[0], 40)] = np.inf
    D[rng.integers(0, V.shape[0], 40)] = np.floor(D[:40] + 3.0)    # ties on k w
    ref = check(lib, V, F, D, 1.0)
    assert 0 < ref['live'].sum() < F.shape[0]
    check(lib, V, F, rng.uniform(0, 30, V.shape[0]), 0.2)


def test_the_argument_rules_and_the_quantum(lib):
    bad = ctypes.c_int(0)
    band = lambda D, w: (lib.shim_band(float(D), float(w), ctypes.addressof(bad)), bad.value)
    assert band(0.0, 1.0) == (0, 0) and band(-0.0, 1.0) == (0, 0) and band(2.0, 1.0) == (2, 0) and band(np.nextafter(2.0, 0), 1.0) == (1, 0)
    assert band(np.inf, 1.0) == (-1, 0) and band(-1e-300, 1.0) == (-1, 0) and band(-np.inf, 1.0) == (-1, 0)
    assert band(np.nan, 1.0) == (-1, 1) and band(2.0 ** 30, 1.0) == (1 << 30, 0) and band(2.0 ** 30 + 1, 1.0) == (-1, 1) and band(1.0, 1e-320) == (-1, 1)
    assert [lib.shim_width_ok(w) for w in (1.0, 5e-324, np.inf, 0.0, -1.0, np.nan)] == [1, 1, 0, 0, 0, 0]
    for e, q in ((1.0, 2.0 ** -19), (0.999, 2.0 ** -20), (8.0, 2.0 ** -16), (0.0, 1.0), (2.0 ** -149, 2.0 ** -168), (3.0e38, 2.0 ** 108)):
        assert lib.shim_quantum(e) == q and (e == 0 or e / q < 2 ** 20)
    V, F = R.torus_mesh(6, 4)
    twin = R.twins(F)
    assert lib.shim_twins_ok(p(F), p(twin), F.shape[0]) == 1
    for h, t in ((4, 3 * F.shape[0]), (4, -2), (4, 4), (4, twin[5])):
        b = twin.copy()
        b[h] = t
        assert lib.shim_twins_ok(p(F), p(b), F.shape[0]) == 0
    D = np.ones(V.shape[0])
    for D_, w in ((np.where(np.arange(V.shape[0]) == 3, np.nan, 1.0), 1.0), (D, 0.0), (D * 2.0 ** 31, 1.0)):
        shim(lib, V, F, D_, w, expect=-1)
    sizes = shim(lib, V, F, D, 1.0, cap=5, expect=-2)               # too small: the size is told
    assert sizes[0] == F.shape[0]


def test_the_same_core_under_the_sanitizers(lib, tmp_path):
    """the shim with a main of its own, built with -fsanitize=address,undefined and run as a program: no report, and the same bytes"""
    exe = os.path.join(str(tmp_path), 'shim_san')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DNWA_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)])
    Vt, Ft = R.torus_mesh()
    Vs, Fs = R.strip_mesh(9)
    Ds = np.arange(Vs.shape[0], dtype=np.float64) * 0.5
    Ds[4] = 1000.3
    Vr, Fr = _random_soup(300, 3)
    Dr = np.random.default_rng(4).uniform(-1, 20, Vr.shape[0])
    Dr[::17] = np.inf
    runs = [(Vt, Ft, R.edge_dijkstra(Vt, Ft, 0), 0.3, False), (Vt, Ft, Vt[:, 0].astype(np.float64) + 4.0123, 0.05, True), (Vs, Fs, Ds, 1.0, False),
            (Vr, Fr, Dr, 0.7, True), (Vt, Ft, np.full(Vt.shape[0], np.inf), 1.0, False)]
    for k, (V_, F_, D_, w, back) in enumerate(runs):
        mine = shim(lib, V_, F_, D_, w, back)
        V32, F32, twin, D64, w_ = mine['blob']
        fin, fout = os.path.join(str(tmp_path), 'in%d.bin' % k), os.path.join(str(tmp_path), 'out%d.bin' % k)
        with open(fin, 'wb') as fh:
            fh.write(np.array([V32.shape[0], F32.shape[0], int(back), 1 << 18], np.int64).tobytes())
            fh.write(np.array([w_]).tobytes() + V32.tobytes() + F32.tobytes() + twin.tobytes() + D64.tobytes())
        res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        raw = open(fout, 'rb').read()
        assert int(np.frombuffer(raw, np.int32, 1)[0]) == 0
        P, N, A = [int(x) for x in np.frombuffer(raw, np.int64, 3, 4)]
        assert (P, N, A) == (mine['piece_node'].size, mine['node_band'].size, mine['arcs'].shape[0])
        assert raw[28:] == b''.join(mine[key].tobytes() for key in KEYS)
