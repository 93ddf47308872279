"""
The screened Poisson grid solver, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_poisson_core.h holds a sample's normal and weights, the
depth rule, a node's row of the system, one red-black update, the residual, the prolongation and the quantisation as __host__ __device__
functions.  This test compiles them for the CPU (g++ -ffp-contract=off) behind a shim of its own -- the kernels' bodies, one sample or one
node after the other -- and asks for the restatement's (tests/screened_poisson_ref.py) integers and bits.  The same source with a main of
its own runs once under -fsanitize=address,undefined, as a program.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import screened_poisson_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "nw_poisson_core.h"

// the two nodes and the upper weight of n coordinates of one axis, and their home nodes: out[4 i ..] = ia, ib, q, home
extern "C" void shim_axis(const float *p, long long n, float lo, double hl, int nl, int *out)
{
    for (long long i = 0; i < n; ++i) {
        nwo_axis(p[i], lo, hl, nl, out + 4 * i, out + 4 * i + 1, out + 4 * i + 2);
        out[4 * i + 3] = nwo_home(p[i], lo, hl, nl);
    }
}

// nq[3 i ..] and rc[i] of n normals
extern "C" void shim_normals(const float *nrm, long long n, int use_lengths, int *nq, int *rc)
{
    for (long long i = 0; i < n; ++i) rc[i] = nwo_normal(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2], use_lengths, nq + 3 * i);
}

extern "C" int shim_depth_used(long long n_used, const long long *occ, int depth, int fulldepth, double spn)
{
    return nwo_depth_used(n_used, (const int64_t *)occ, depth, fulldepth, spn);
}

extern "C" double shim_alpha(double pw, long long occ, long long n) { return nwo_alpha(pw, occ, n); }
extern "C" double shim_pow2_above(double m) { return nwo_pow2_above(m); }
extern "C" unsigned long long shim_quantise(double chi, double E) { return nwo_quantise(chi, E); }

// One level as the kernels run it.  acc: 4 n^3 int64 (W, then V's planes), zeroed here; coarse: the chi of the level below or NULL (chi = 0).
// doubles: rhs, diag, chi0 (before the sweeps), chi (after them), n^3 each; scal: residual before, after, M, E; F: n^3; ints: sum W, sum W Fl,
// sum W Fh, thr.  -> the number of samples used, -1 for a refused normal, -2 if M is 0
extern "C" long long shim_level(const float *xyz, const float *nrm, long long n, int use_lengths, const float *lo, float h, int depth, int level, int used,
                                double alpha, int sweeps, const double *coarse, long long *acc, double *rhs, double *diag, double *chi0, double *chi,
                                double *scal, unsigned long long *F, unsigned long long *ints)
{
    const int nl = 1 << level;
    const long long nodes = (long long)nl * nl * nl;
    const double hl = nwo_spacing(h, depth, level);
    memset(acc, 0, sizeof(long long) * 4 * nodes);
    long long n_used = 0;
    for (long long s = 0; s < n; ++s) {
        int q[3];
        const int rc = nwo_normal(nrm[3 * s], nrm[3 * s + 1], nrm[3 * s + 2], use_lengths, q);
        if (rc < 0) return -1;
        if (rc == 0) continue;
        ++n_used;
        int a[3], b[3], w[3];
        for (int d = 0; d < 3; ++d) nwo_axis(xyz[3 * s + d], lo[d], hl, nl, &a[d], &b[d], &w[d]);
        for (int c = 0; c < 8; ++c) {
            long long wt = 1;
            int at[3];
            for (int d = 0; d < 3; ++d) { at[d] = (c >> d) & 1 ? b[d] : a[d]; wt *= (c >> d) & 1 ? w[d] : (1 << NWO_WEIGHT_BITS) - w[d]; }
            const int64_t lin = nwo_lin(level, at[0], at[1], at[2]);
            acc[lin] += wt;
            for (int d = 0; d < 3; ++d) acc[(d + 1) * nodes + lin] += wt * q[d];
        }
    }
    const double s = (double)(1 << (used - level));
    for (int k = 0; k < nl; ++k) for (int j = 0; j < nl; ++j) for (int i = 0; i < nl; ++i) {
        const int64_t c = nwo_lin(level, i, j, k);
        nwo_system_node(acc, acc + nodes, level, i, j, k, alpha / s, 1.0 / (s * s), rhs + c, diag + c);
        chi[c] = coarse ? nwo_prolong_node(coarse, level, i, j, k) : 0.0;
        chi0[c] = chi[c];
    }
    double res[2] = {0.0, 0.0};
    for (int pass = 0; pass < 2; ++pass) {
        for (int k = 0; k < nl; ++k) for (int j = 0; j < nl; ++j) for (int i = 0; i < nl; ++i) {
            const int64_t c = nwo_lin(level, i, j, k);
            const double r = nwo_residual(rhs[c], diag[c], chi[c], nwo_neighbour_sum(chi, level, i, j, k));
            if (r > res[pass]) res[pass] = r;
        }
        if (pass == 0)
            for (int sw = 0; sw < sweeps; ++sw)
                for (int colour = 0; colour < 2; ++colour)
                    for (int k = 0; k < nl; ++k) for (int j = 0; j < nl; ++j) for (int i = 0; i < nl; ++i) {
                        if (((i + j + k) & 1) != colour) continue;
                        const int64_t c = nwo_lin(level, i, j, k);
                        chi[c] = nwo_update(rhs[c], nwo_neighbour_sum(chi, level, i, j, k), diag[c]);
                    }
    }
    double M = 0.0;
    for (long long c = 0; c < nodes; ++c) if (fabs(chi[c]) > M) M = fabs(chi[c]);
    scal[0] = res[0]; scal[1] = res[1]; scal[2] = M; scal[3] = 0.0;
    if (!(M > 0.0)) return -2;
    const double E = nwo_pow2_above(M);
    scal[3] = E;
    ints[0] = ints[1] = ints[2] = 0;
    for (long long c = 0; c < nodes; ++c) {
        F[c] = nwo_quantise(chi[c], E);
        ints[0] += (unsigned long long)acc[c];
        ints[1] += (unsigned long long)acc[c] * (F[c] & 0xffffull);
        ints[2] += (unsigned long long)acc[c] * (F[c] >> 16);
    }
    ints[3] = nwo_level(ints[1], ints[2], ints[0]);
    return n_used;
}

#ifdef NWO_MAIN
// the same call on arrays read from a file: 7 int64 (n, use_lengths, depth, level, used, sweeps, 1 if a coarse chi follows), lo[3] and h
// (4 floats), alpha (1 double), xyz, normals, the coarse chi
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 7);
    const auto box = rd<float>(fh, 4);
    const auto alpha = rd<double>(fh, 1);
    const auto xyz = rd<float>(fh, 3 * c[0]);
    const auto nrm = rd<float>(fh, 3 * c[0]);
    const int level = (int)c[3];
    const size_t nodes = (size_t)1 << (3 * level);
    const auto coarse = rd<double>(fh, c[6] ? nodes / 8 : 0);
    fclose(fh);
    std::vector<long long> acc(4 * nodes);
    std::vector<double> rhs(nodes), diag(nodes), chi0(nodes), chi(nodes), scal(4);
    std::vector<unsigned long long> F(nodes), ints(4);
    const long long r = shim_level(xyz.data(), nrm.data(), c[0], (int)c[1], box.data(), box[3], (int)c[2], level, (int)c[4], alpha[0], (int)c[5],
                                   c[6] ? coarse.data() : nullptr, acc.data(), rhs.data(), diag.data(), chi0.data(), chi.data(), scal.data(), F.data(), ints.data());
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(&r, sizeof(long long), 1, fh);
    fwrite(acc.data(), sizeof(long long), acc.size(), fh);
    fwrite(rhs.data(), sizeof(double), nodes, fh);
    fwrite(diag.data(), sizeof(double), nodes, fh);
    fwrite(chi0.data(), sizeof(double), nodes, fh);
    fwrite(chi.data(), sizeof(double), nodes, fh);
    fwrite(scal.data(), sizeof(double), 4, fh);
    fwrite(F.data(), sizeof(unsigned long long), nodes, fh);
    fwrite(ints.data(), sizeof(unsigned long long), 4, fh);
    fclose(fh);
    return 0;
}
#endif
'''

p = lambda a: a.ctypes.data


def _source(tmp):
    src = os.path.join(str(tmp), 'shim.cpp')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    return src


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwo_shim')
    src, so = _source(d), os.path.join(str(d), 'libnwo_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', so, src])
    L = ctypes.CDLL(so)
    vp, f32, f64, ll, i32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_int
    L.shim_axis.argtypes = [vp, ll, f32, f64, i32, vp]
    L.shim_axis.restype = None
    L.shim_normals.argtypes = [vp, ll, i32, vp, vp]
    L.shim_normals.restype = None
    L.shim_depth_used.argtypes = [ll, vp, i32, i32, f64]
    L.shim_alpha.argtypes, L.shim_alpha.restype = [f64, ll, ll], f64
    L.shim_pow2_above.argtypes, L.shim_pow2_above.restype = [f64], f64
    L.shim_quantise.argtypes, L.shim_quantise.restype = [f64, f64], ctypes.c_ulonglong
    L.shim_level.argtypes = [vp, vp, ll, i32, vp, f32, i32, i32, i32, f64, i32, vp] + [vp] * 8
    L.shim_level.restype = ll
    return L


@pytest.mark.parametrize('lo,h,depth,level', [(-110.0, 220.0 / 128, 7, 7), (-110.0, 220.0 / 128, 7, 4), (0.0, 1.0, 3, 2), (1.0e6, 0.37, 5, 5), (-3.3, 1e-3, 9, 9)])
def test_the_weights_of_random_and_special_positions(lib, lo, h, depth, level):
    rng = np.random.default_rng(level)
    nl, h32, lo32 = 1 << level, np.float32(h), np.float32(lo)
    hl = R.level_spacing(h32, depth, level)
    x = np.concatenate([rng.uniform(float(lo32) - 2 * hl, float(lo32) + (nl + 2) * hl, 10000).astype(np.float32), R.special_positions(lo32, hl, nl)])
    out = np.full((len(x), 4), -7, np.int32)
    lib.shim_axis(p(x), len(x), lo32, hl, nl, p(out))
    ia, ib, wa, wb = R.axis_weights(x, lo32, hl, nl)
    assert np.array_equal(out[:, 0], ia) and np.array_equal(out[:, 1], ib) and np.array_equal(out[:, 2], wb) and np.array_equal(128 - out[:, 2], wa)
    assert np.array_equal(out[:, 3], R.axis_home(x, lo32, hl, nl))
    assert out[:, 2].min() >= 0 and out[:, 2].max() <= 128 and out[:, :2].min() >= 0 and out[:, :2].max() <= nl - 1
    assert (out[:, 2] == 64).any() and (out[:, 2] == 0).any() and (out[:, 0] == out[:, 1]).any()


def test_the_normals(lib):
    rng = np.random.default_rng(4)
    N = np.concatenate([rng.normal(size=(2000, 3)), np.eye(3), -np.eye(3), np.zeros((2, 3)), 1e-30 * rng.normal(size=(5, 3)), 1e30 * rng.normal(size=(5, 3)),
                        [[1e-45, 0, 0], [3e38, 3e38, 3e38], [0.25, 0, 0], [0.6, 0.8, 0.0]]]).astype(np.float32)
    nq, rc = np.full((len(N), 3), -7, np.int32), np.full(len(N), -7, np.int32)
    lib.shim_normals(p(N), len(N), 0, p(nq), p(rc))
    ref, used = R.quantise_normals(N)
    assert np.array_equal(nq, ref) and np.array_equal(rc == 1, used) and (rc >= 0).all() and int((rc == 0).sum()) == 2
    assert np.abs(nq).max() == 4096 and nq[2000].tolist() == [4096, 0, 0] and nq[2005].tolist() == [0, 0, -4096]
    small = np.clip(N[:2008] * np.float32(0.25), -1.0, 1.0).astype(np.float32)
    lib.shim_normals(p(small), len(small), 1, p(nq), p(rc))
    ref, used = R.quantise_normals(small, use_lengths=True)
    keep = np.abs(small).max(1) <= 1
    assert keep.all() and np.array_equal(nq[:len(small)], ref) and np.array_equal(rc[:len(small)] == 1, used)
    big = np.array([[0.5, 1.5, 0.0], [0.0, 0.0, -1.0000001]], np.float32)
    lib.shim_normals(p(big), 2, 1, p(nq), p(rc))
    assert rc[:2].tolist() == [-1, -1]
    with pytest.raises(ValueError):
        R.quantise_normals(big, use_lengths=True)


def test_the_depth_rule_and_the_scalars(lib):
    rng = np.random.default_rng(1)
    for _ in range(300):
        depth = int(rng.integers(3, 10))
        occ = np.zeros(depth + 1, np.int64)
        occ[2:] = np.sort(rng.integers(1, 5000, depth - 1))
        n, full, spn = int(rng.integers(1, 6000)), int(rng.integers(0, 11)), float(rng.choice([0.0, 0.5, 1.0, 1.5, 15.0]))
        assert lib.shim_depth_used(n, p(occ), depth, full, spn) == R.depth_used(n, {l: int(occ[l]) for l in range(2, depth + 1)}, depth, full, spn)
    occ = np.array([0, 0, 8, 20, 40, 80], np.int64)                   # exactly at N / occ_l: 60 < 1.5 * 40 is false, so level 4 is taken
    assert lib.shim_depth_used(60, p(occ), 5, 0, 1.5) == 4 and lib.shim_depth_used(59, p(occ), 5, 0, 1.5) == 3 and lib.shim_depth_used(59, p(occ), 5, 4, 1.5) == 4
    assert lib.shim_alpha(4.0, 1234, 5000) == R.alpha_of(4.0, 1234, 5000)
    for m in (1.0, 0.5, 0.75, 3.0, 4.0, float(np.nextafter(4.0, 5.0)), 1e-300, 2.0 ** -1030, 1e300):
        assert lib.shim_pow2_above(m) == R.pow2_above(m) >= m > R.pow2_above(m) / 2
    assert lib.shim_quantise(1.0, 1.0) == 1 << 32 and lib.shim_quantise(-1.0, 1.0) == 0 and lib.shim_quantise(0.0, 8.0) == 1 << 31


def cloud(n=400, seed=0):
    P, N = R.sphere_cloud(n, radius=100.0, sigma=3.0, seed=seed)
    N[::17] = 0.0                                                     # some samples are skipped
    return P, N


def shim_level(lib, P, N, lo, h, depth, level, used, alpha, sweeps, coarse, use_lengths=0):
    n = 1 << level
    acc = np.full((4, n, n, n), 7, np.int64)
    rhs, diag, chi0, chi = (np.full((n, n, n), 7.0) for _ in range(4))
    scal, F, ints = np.zeros(4), np.zeros((n, n, n), np.uint64), np.zeros(4, np.uint64)
    lo = np.ascontiguousarray(lo, np.float32)
    rc = lib.shim_level(p(P), p(N), len(P), use_lengths, p(lo), np.float32(h), depth, level, used, alpha, sweeps, None if coarse is None else p(coarse),
                        p(acc), p(rhs), p(diag), p(chi0), p(chi), p(scal), p(F), p(ints))
    return dict(rc=rc, W=acc[0], V=acc[1:], rhs=rhs, diag=diag, chi0=chi0, chi=chi, res=(scal[0], scal[1]), M=scal[2], E=scal[3], F=F,
                ints=[int(x) for x in ints])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def reference_levels(P, N, lo, h, depth, alpha, sweeps):
    """levels 2 .. depth of the restatement with `sweeps` sweeps at each of them"""
    nq, used = R.quantise_normals(N)
    out, chi = {}, None
    for l in range(2, depth + 1):
        W, V = R.splat(P, nq, used, lo, h, depth, l)
        rhs, diag = R.system(W, V, alpha, 1 << (depth - l))
        chi0 = np.zeros_like(rhs) if l == 2 else R.prolong(chi)
        chi = chi0.copy()
        before = R.residual(chi, rhs, diag)
        R.relax(chi, rhs, diag, sweeps)
        out[l] = dict(W=W, V=V, rhs=rhs, diag=diag, chi0=chi0, chi=chi.copy(), res=(before, R.residual(chi, rhs, diag)), n_used=int(used.sum()))
        out[l].update(R.field(chi, W))
    return out


def same_level(mine, ref):
    assert mine['rc'] == ref['n_used']
    assert np.array_equal(mine['W'], ref['W']) and np.array_equal(mine['V'], ref['V'])
    for k in ('rhs', 'diag', 'chi0', 'chi'):
        assert np.array_equal(bits(mine[k]), bits(ref[k])), k
    assert bits(np.array(mine['res'])).tolist() == bits(np.array(ref['res'])).tolist()
    assert mine['M'] == ref['M'] and mine['E'] == ref['E'] and np.array_equal(mine['F'], ref['F'])
    assert mine['ints'] == [ref['sumW'], ref['limbs'][0], ref['limbs'][1], ref['thr']]


def test_a_full_level_at_4_8_and_16_nodes(lib):
    P, N = cloud()
    lo, h = R.cube_for(P, 4)
    alpha = 0.731
    ref = reference_levels(P, N, lo, h, 4, alpha, 3)
    coarse = None
    for l in (2, 3, 4):
        mine = shim_level(lib, P, N, lo, h, 4, l, 4, alpha, 3, coarse)
        same_level(mine, ref[l])
        assert int(mine['W'].sum()) == mine['rc'] << 21 and mine['res'][1] < mine['res'][0]
        coarse = mine['chi']
    assert set(np.unique(ref[3]['diag'] - (alpha / 2) * (ref[3]['W'] / 2.0 ** 21))) == {3.0, 4.0, 5.0, 6.0}


def test_the_same_core_under_the_sanitizers(lib, tmp_path):
    """the shim with a main of its own, built with -fsanitize=address,undefined and run as a program: no report, and the same bytes"""
    exe = os.path.join(str(tmp_path), 'shim_san')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-DNWO_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)])
    P, N = cloud(300, seed=3)
    P = np.concatenate([P, [[1e4, -1e4, 0.0], [3e38, 3e38, -3e38]]]).astype(np.float32)           # far outside the cube: clamped to the border
    N = np.concatenate([N, [[0, 0, 1], [1, 0, 0]]]).astype(np.float32)
    lo, h = R.cube_for(P[:300], 3)
    coarse = None
    for k, level in enumerate((2, 3)):
        mine = shim_level(lib, P, N, lo, h, 3, level, 3, 1.25, 2, coarse)
        fin, fout = os.path.join(str(tmp_path), 'in%d.bin' % k), os.path.join(str(tmp_path), 'out%d.bin' % k)
        with open(fin, 'wb') as fh:
            fh.write(np.array([len(P), 0, 3, level, 3, 2, 0 if coarse is None else 1], np.int64).tobytes())
            fh.write(np.concatenate([lo, [h]]).astype(np.float32).tobytes() + np.array([1.25]).tobytes() + P.tobytes() + N.tobytes())
            if coarse is not None:
                fh.write(coarse.tobytes())
        res = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        raw = open(fout, 'rb').read()
        nodes = 1 << (3 * level)
        want = (np.array([mine['rc']], np.int64).tobytes() + mine['W'].tobytes() + mine['V'].tobytes() + mine['rhs'].tobytes() + mine['diag'].tobytes()
                + mine['chi0'].tobytes() + mine['chi'].tobytes() + np.array(list(mine['res']) + [mine['M'], mine['E']]).tobytes() + mine['F'].tobytes()
                + np.array(mine['ints'], np.uint64).tobytes())
        assert len(raw) == 8 + 8 * nodes * 9 + 32 + 32 and raw == want
        coarse = mine['chi']
