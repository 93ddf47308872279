"""
The mesh-to-mesh distance, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_proximity_core.h holds the triangle-triangle distance and
the capped walk of a face over a centroid grid handed in as arrays, as __host__ __device__ functions.  This test compiles them for the
CPU (g++ -ffp-contract=off) behind a shim of its own -- the pair function on aligned triangles, and the loop over A's faces with the
second evaluation of the winning pair -- and asks for the bits of the NumPy restatement (tests/mesh_proximity_ref.py): d2, partner,
kind, closest points and band membership.  The grid is binned here in NumPy, at four cell sizes.  The same source with a main of its
own runs once under -fsanitize=address,undefined.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_distance_ref as D
import mesh_proximity_ref as P
from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nw_proximity_core.h"
extern "C" void shim_pairs(const float *ta, const float *tb, long long n, double *d2, int *kind, double *ca, double *cb)
{
    for (long long i = 0; i < n; ++i)
        d2[i] = nwm_tri_tri(ta + 9 * i, ta + 9 * i + 3, ta + 9 * i + 6, tb + 9 * i, tb + 9 * i + 3, tb + 9 * i + 6, &kind[i], ca + 3 * i, cb + 3 * i);
}

// -> the number of faces whose second evaluation gives another d2 than the walk kept
extern "C" long long shim_mesh(const float *apos, const int *afaces, long long nfa, const float *bpos, const int *bfaces, long long nfb, const nwm_pt *pts,
                               const int *cstart, const double *rho, double rho_max, const double *glo, const double *ghi, double gh, const int *gdims,
                               double d_cap, double *d2_out, double *distance, int *partner, int *kind, double *ca, double *cb, long long *rings,
                               long long *centroids, long long *tests)
{
    nwm_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = glo[d]; g.hi[d] = ghi[d]; g.dims[d] = gdims[d]; }
    g.h = gh;
    long long bad = 0;
    for (long long f = 0; f < nfa; ++f) {
        const float *a0 = apos + 3 * (long long)afaces[3 * f], *a1 = apos + 3 * (long long)afaces[3 * f + 1], *a2 = apos + 3 * (long long)afaces[3 * f + 2];
        double cf[3];
        const double rho_f = nwd_face_centroid(a0, a1, a2, cf) * (1.0 + NWM_CORE_SLACK);
        nwm_best b;
        int n_cen = 0, n_tests = 0;
        rings[f] = nwm_walk(cf, rho_f, a0, a1, a2, bpos, bfaces, (int)nfb, pts, cstart, rho, rho_max, g, d_cap, b, n_cen, n_tests);
        centroids[f] = n_cen;
        tests[f] = n_tests;
        d2_out[f] = b.d2;
        partner[f] = nwm_partner(b, d_cap);
        const double again = nwm_finish(a0, a1, a2, bpos, bfaces, partner[f], &distance[f], &kind[f], ca + 3 * f, cb + 3 * f);
        if (partner[f] >= 0 && !(again == b.d2)) ++bad;
    }
    return bad;
}

#ifdef NWM_MAIN
// the same call on arrays read from a file: <in> holds 6 int64 counts (nva, nfa, nvb, nfb, npts, ncells), then the arrays
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 6);
    const auto apos = rd<float>(fh, 3 * c[0]);
    const auto afaces = rd<int>(fh, 3 * c[1]);
    const auto bpos = rd<float>(fh, 3 * c[2]);
    const auto bfaces = rd<int>(fh, 3 * c[3]);
    const auto pts = rd<nwm_pt>(fh, c[4]);
    const auto cstart = rd<int>(fh, c[5] + 1);
    const auto rho = rd<double>(fh, c[3]);
    const auto dbl = rd<double>(fh, 9);                       // rho_max, glo[3], ghi[3], gh, d_cap
    const auto gdims = rd<int>(fh, 3);
    fclose(fh);
    const size_t n = (size_t)c[1];
    std::vector<double> d2(n), dist(n), ca(3 * n), cb(3 * n);
    std::vector<int> partner(n), kind(n);
    std::vector<long long> rings(n), cen(n), tests(n);
    const long long bad = shim_mesh(apos.data(), afaces.data(), c[1], bpos.data(), bfaces.data(), c[3], pts.data(), cstart.data(), rho.data(), dbl[0], &dbl[1],
                                    &dbl[4], dbl[7], gdims.data(), dbl[8], d2.data(), dist.data(), partner.data(), kind.data(), ca.data(), cb.data(),
                                    rings.data(), cen.data(), tests.data());
    std::vector<double> pd2(n), pca(3 * n), pcb(3 * n);
    std::vector<int> pkind(n);
    std::vector<float> ta(9 * n), tb(9 * n);
    for (size_t f = 0; f < n; ++f)
        for (int k = 0; k < 3; ++k)
            for (int d = 0; d < 3; ++d) {
                ta[9 * f + 3 * k + d] = apos[3 * (size_t)afaces[3 * f + k] + d];
                tb[9 * f + 3 * k + d] = bpos[3 * (size_t)bfaces[3 * (f % (size_t)c[3]) + k] + d];
            }
    shim_pairs(ta.data(), tb.data(), (long long)n, pd2.data(), pkind.data(), pca.data(), pcb.data());
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(dist.data(), sizeof(double), n, fh);
    fwrite(ca.data(), sizeof(double), 3 * n, fh);
    fwrite(partner.data(), sizeof(int), n, fh);
    fwrite(kind.data(), sizeof(int), n, fh);
    fclose(fh);
    return bad ? 1 : 0;
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
    d = tmp_path_factory.mktemp('nwm_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwm_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f64, ll = ctypes.c_void_p, ctypes.c_double, ctypes.c_longlong
    L.shim_pairs.argtypes = [vp, vp, ll] + [vp] * 4
    L.shim_pairs.restype = None
    L.shim_mesh.argtypes = [vp, vp, ll, vp, vp, ll, vp, vp, vp, f64, vp, vp, f64, vp, f64] + [vp] * 9
    L.shim_mesh.restype = ll
    return L


def shim_pairs(lib, ta, tb):
    ta, tb = np.ascontiguousarray(ta, np.float32).reshape(-1, 3, 3), np.ascontiguousarray(tb, np.float32).reshape(-1, 3, 3)
    n = len(ta)
    d2, kind, ca, cb = np.empty(n), np.empty(n, np.int32), np.empty((n, 3)), np.empty((n, 3))
    lib.shim_pairs(p(ta), p(tb), n, p(d2), p(kind), p(ca), p(cb))
    return d2, kind, ca, cb


def shim_mesh(lib, va, fa, vb, fb, band, h_cell):
    va, fa, vb, fb = (np.ascontiguousarray(a, t) for a, t in ((va, np.float32), (fa, np.int32), (vb, np.float32), (fb, np.int32)))
    pts, cstart, rho, rho_max, glo, ghi, gdims = P.centroid_grid(vb, fb, h_cell)
    n = len(fa)
    out = dict(d2=np.empty(n), distance=np.empty(n), partner=np.empty(n, np.int32), kind=np.empty(n, np.int32), closest_a=np.empty((n, 3)),
               closest_b=np.empty((n, 3)), rings=np.empty(n, np.int64), centroids=np.empty(n, np.int64), tests=np.empty(n, np.int64))
    bad = lib.shim_mesh(p(va), p(fa), n, p(vb), p(fb), len(fb), p(pts), p(cstart), p(rho), rho_max, p(glo), p(ghi), float(h_cell), p(gdims), float(band),
                        *(p(out[k]) for k in ('d2', 'distance', 'partner', 'kind', 'closest_a', 'closest_b', 'rings', 'centroids', 'tests')))
    assert bad == 0                                                                           # the second evaluation gives the walk's d2
    out['blob'] = (va, fa, vb, fb, pts, cstart, rho, rho_max, glo, ghi, gdims)
    return out


def check_mesh(lib, va, fa, vb, fb, band, cells):
    ref = P.mesh_distance(va, fa, vb, fb, band)
    for h_cell in cells:
        mine = shim_mesh(lib, va, fa, vb, fb, band, h_cell)
        P.same_as_restatement(mine, ref)
        near = ref['in_band']
        assert np.array_equal(D.bits(mine['d2'][near]), D.bits(ref['d2'][near]))
        assert (np.sqrt(mine['d2'][~near]) > band).all()                                      # (inf where no face was examined)
    return ref


# ---- the pair function ------------------------------------------------------------------------------------------------------------------
def test_closed_forms_have_the_restatements_bits(lib):
    names = sorted(P.CLOSED_FORMS)
    d2, kind, ca, cb = shim_pairs(lib, [P.CLOSED_FORMS[n][0] for n in names], [P.CLOSED_FORMS[n][1] for n in names])
    for i, n in enumerate(names):
        assert d2[i] == P.CLOSED_FORMS[n][2] and kind[i] in P.CLOSED_FORMS[n][3], n
        r = P.tri_tri(P.CLOSED_FORMS[n][0], P.CLOSED_FORMS[n][1])
        assert (D.bits(d2[i]), kind[i]) == (D.bits(r[0]), r[1]) and np.array_equal(D.bits(ca[i]), D.bits(r[2])) and np.array_equal(D.bits(cb[i]), D.bits(r[3]))
    assert not np.signbit(d2).any()


def test_ten_thousand_random_pairs(lib):
    rng = np.random.default_rng(11)
    t = (rng.normal(size=(10000, 2, 3, 3)) + rng.normal(size=(10000, 2, 1, 3)) * rng.uniform(0, 2, (10000, 1, 1, 1))).astype(np.float32)
    mine = shim_pairs(lib, t[:, 0], t[:, 1])
    ref = P.pairwise(t[:, 0], t[:, 1])
    assert np.array_equal(mine[1], ref[1]) and sorted(set(ref[1].tolist())) == list(range(16))      # every kind is reached
    for a, b in zip((mine[0], mine[2], mine[3]), (ref[0], ref[2], ref[3])):
        assert np.array_equal(D.bits(a), D.bits(b))


def test_needles_flat_faces_far_pairs_and_near_parallel_edges(lib):
    v, f = D.needles()
    t = v[f]
    sets = [(t[:20], t[20:]), (t[:20] + np.float32(1e6), t[20:] + np.float32(1e6))]
    rng = np.random.default_rng(5)
    far = (rng.normal(size=(50, 2, 3, 3)) * 30 + 1e6).astype(np.float32)
    sets.append((far[:, 0], far[:, 1]))
    flat = np.array([[[0, 0, 0], [0, 0, 0], [1, 0, 0]], [[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[1, 2, 3], [1, 2, 3], [1, 2, 3]], [[0, 0, 0], [4, 0, 0], [0, 4, 0]]], np.float32)
    other = np.array([[[0.5, -1, -1], [0.5, 1, -1], [0.5, 0, 2]]] * 4, np.float32)
    sets += [(flat, other), (other, flat), (flat, flat[::-1])]
    sets.append(P.near_parallel_edges())
    sets.append(P.near_parallel_edges()[::-1])
    for ta, tb in sets:
        mine, ref = shim_pairs(lib, ta, tb), P.pairwise(ta, tb)
        assert np.array_equal(mine[1], ref[1])
        for a, b in zip((mine[0], mine[2], mine[3]), (ref[0], ref[2], ref[3])):
            assert np.array_equal(D.bits(a), D.bits(b))
        assert np.isfinite(mine[0]).all() and np.isfinite(mine[2]).all() and np.isfinite(mine[3]).all()


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def test_two_cubes_at_the_band_and_one_ulp_below(lib):
    va, fa, vb, fb, side_a, side_b = P.two_cubes(3.0)
    for band in (np.inf, 30.0, 3.0):
        ref = check_mesh(lib, va, fa, vb, fb, band, (0.7, 2.0, 3.0, 40.0))
        assert (ref['distance'][side_a] == 3.0).all() and (ref['partner'][side_a] >= 0).all()
    ref = check_mesh(lib, va, fa, vb, fb, np.nextafter(3.0, 0.0), (0.7, 2.0, 3.0, 40.0))
    assert ref['n_in_band'] == 0 and (ref['partner'] == -1).all()


def test_spheres_apart_and_crossing_at_four_cell_sizes(lib):
    for va, fa, vb, fb in (P.two_spheres(), P.crossing_spheres()):
        for band in (np.inf, 30.0):
            ref = check_mesh(lib, va, fa, vb, fb, band, (5.0, 14.0, 33.0, 400.0))
            assert 0 < ref['n_in_band'] and (band == np.inf or ref['n_in_band'] < len(fa))
    assert ref['n_zero'] > 20 and (ref['kind'][ref['d2'] == 0] == 0).all()


def test_a_face_spanning_three_times_the_mesh_in_a_and_in_b(lib):
    va, fa, vb, fb = P.two_spheres()
    for a, b in ((P.with_oversize_face(va, fa), (vb, fb)), ((va, fa), P.with_oversize_face(vb, fb))):
        ref = check_mesh(lib, a[0], a[1], b[0], b[1], 30.0, (5.0, 14.0, 60.0, 1000.0))
        assert 0 < ref['n_in_band'] < len(a[1])
    big = len(fb)
    assert (ref['partner'] == big).sum() > 3                                               # the oversize face of B is some faces' partner


def test_flat_faces_and_meshes_a_million_from_the_origin(lib):
    va, fa, vb, fb = P.two_spheres()
    check_mesh(lib, *P.with_flat_faces(va, fa), *P.with_flat_faces(vb, fb), 30.0, (5.0, 14.0, 33.0, 400.0))
    ref = check_mesh(lib, va + np.float32(1e6), fa, vb + np.float32(1e6), fb, 30.0, (5.0, 14.0, 33.0, 400.0))
    assert 0 < ref['n_in_band'] < len(fa)


def test_coincident_copies_go_to_the_smallest_id(lib):
    va, fa = P.soup([P.FLOOR])
    vb, fb = P.soup([[[0, 0, 2], [4, 0, 2], [0, 4, 2]]] * 300)
    ref = check_mesh(lib, va, fa, vb, fb, np.inf, (0.5, 1.0, 7.0))
    assert ref['partner'][0] == 0 and ref['distance'][0] == 2.0


def test_a_far_face_stops_after_the_rings_the_band_allows(lib):
    va, fa, vb, fb = P.nested_spheres()
    h_cell, band = 10.0, 30.0
    mine = shim_mesh(lib, va, fa, vb, fb, band, h_cell)
    rho_max = mine['blob'][7]
    rho_a = P.face_rho(va, fa)
    assert (mine['partner'] == -1).all() and np.isinf(mine['distance']).all() and np.isnan(mine['closest_a']).all()
    assert (mine['rings'] <= np.ceil((band + rho_a * (1 + 1e-9) + rho_max) / h_cell) + 1).all() and 5 <= mine['rings'].min() and mine['rings'].max() < 9
    assert mine['tests'].sum() == 0 and mine['blob'][10].max() >= 20                        # a walk without a band would cross 20 cells an axis


def test_a_main_of_its_own_under_the_sanitizers(lib, tmp_path):
    cxx = os.environ.get('CXX', 'g++')
    exe = os.path.join(str(tmp_path), 'nwm_main')
    flags = ['-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    # whether the compiler has the sanitizers' runtimes is asked of a program of one line; the shim's own compile errors fail the test
    probe = os.path.join(str(tmp_path), 'probe.cpp')
    with open(probe, 'w') as fh:
        fh.write('int main() { return 0; }\n')
    if subprocess.run([cxx] + flags + ['-o', os.path.join(str(tmp_path), 'probe'), probe], capture_output=True, text=True).returncode != 0:
        pytest.skip('the compiler has no sanitizer runtime')
    r = subprocess.run([cxx] + flags + ['-DNWM_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    va, fa, vb, fb = P.crossing_spheres()
    mine = shim_mesh(lib, va, fa, vb, fb, 30.0, 14.0)
    va, fa, vb, fb, pts, cstart, rho, rho_max, glo, ghi, gdims = mine['blob']
    src, dst = os.path.join(str(tmp_path), 'in.bin'), os.path.join(str(tmp_path), 'out.bin')
    with open(src, 'wb') as fh:
        fh.write(np.array([len(va), len(fa), len(vb), len(fb), len(pts), len(cstart) - 1], np.int64).tobytes())
        for a in (va, fa, vb, fb, pts, cstart, rho, np.array([rho_max] + glo.tolist() + ghi.tolist() + [14.0, 30.0]), gdims):
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(dst, 'rb').read()
    n = len(fa)
    assert np.array_equal(np.frombuffer(raw, np.uint64, n), D.bits(mine['distance']))
    assert np.array_equal(np.frombuffer(raw, np.uint64, 3 * n, 8 * n), D.bits(mine['closest_a']).ravel())
    assert np.array_equal(np.frombuffer(raw, np.int32, n, 32 * n), mine['partner'])
    assert np.array_equal(np.frombuffer(raw, np.int32, n, 36 * n), mine['kind'])
