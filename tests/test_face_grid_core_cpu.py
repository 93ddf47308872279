"""
The HIP-free half of the mesh query units' face grid (ch_shrinkwrap_amd/csrc/nw_bq_core.h), settled on the CPU: the one definition of a
face's float64 centroid and radius, which nwd_face_centroid and nwx_face_centroid forward to; the cell size a grid starts from (the floor,
"1 for a mesh without extent", the fallback) under the three units' candidates; and the rule by which FaceGrid::bin keeps the grid at hand.
The shim is compiled with g++ -ffp-contract=off in pytest's temporary directory.  Every expected value is computed here, from NumPy
float64 restatements of the arithmetic and from the expressions the six set_mesh bodies held before they shared one.
"""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')
F32, F64 = np.float32, np.float64
SLACK = 1e-9                                    # BQ_FACE_RHO_SLACK
RULE = (16, 1 << 26, 1025, 400)                 # FACE_GRID_RULE

SHIM = r'''
#include "nw_bq_core.h"
#include "nw_distance_core.h"
#include "nw_intersections_core.h"
#include "nw_proximity_core.h"
extern "C" double shim_slack() { return BQ_FACE_RHO_SLACK; }
extern "C" void shim_rule(long long *out)
{
    out[0] = bq::FACE_GRID_RULE.cells_per_point; out[1] = bq::FACE_GRID_RULE.max_cells; out[2] = bq::FACE_GRID_RULE.max_dim; out[3] = bq::FACE_GRID_RULE.widen_steps;
}
// which = 0: bq::face_centroid, 1: nwd_face_centroid, 2: nwx_face_centroid through nwx_load on a one-face mesh
extern "C" void shim_centroids(int which, const float *corners, long long n, double *cen, double *rho)
{
    const int32_t one_face[3] = {0, 1, 2};
    for (long long f = 0; f < n; ++f) {
        const float *a = corners + 9 * f, *b = a + 3, *c = a + 6;
        if (which == 0) rho[f] = bq::face_centroid(a, b, c, cen + 3 * f);
        else if (which == 1) rho[f] = nwd_face_centroid(a, b, c, cen + 3 * f);
        else {
            nwx_v3 m;
            rho[f] = nwx_face_centroid(nwx_load(a, one_face, 0), &m);
            cen[3 * f] = m.x; cen[3 * f + 1] = m.y; cen[3 * f + 2] = m.z;
        }
    }
}
// unit = 0: the fixed grids (distance, intersections, rays), 1: the bands of the volume and mapping units, 2: the proximity unit's band;
// rho_mean = sum / nf as FaceGrid::set_faces keeps it
extern "C" double shim_cell(int unit, double rho_sum, long long nf, double rho_max, double d_cap, double emax)
{
    const double m = rho_sum / (double)nf;
    return bq::face_cell(unit == 0 ? 2.0 * m : unit == 1 ? bq::band_cell(m, rho_max, d_cap) : nwm_band_cell(m, rho_max, d_cap), emax);
}
extern "C" int shim_bins(long long nf, const double *ext, double h0, double *h_start, double *h, int *dims)
{
    return (int)bq::face_bins(nf, ext, h0, h_start, h, dims);
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('face_grid_shim')
    src, lib = os.path.join(str(d), 'shim.cpp'), os.path.join(str(d), 'libface_grid_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    # (plain g++, no HIP header on the include path: the headers must not need one)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-Werror',
                           '-Wno-unused-function', '-I', CSRC, '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp, ll, dbl = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double
    L.shim_slack.restype = dbl
    L.shim_rule.argtypes = [vp]
    L.shim_centroids.argtypes = [ctypes.c_int, vp, ll, vp, vp]
    L.shim_cell.argtypes = [ctypes.c_int, dbl, ll, dbl, dbl, dbl]
    L.shim_cell.restype = dbl
    L.shim_bins.argtypes = [ll, vp, dbl, vp, vp, vp]
    return L


def bits(x):
    return np.ascontiguousarray(x, F64).view(np.uint64)


# ---- the centroid and the radius --------------------------------------------------------------------------------------------------------
def centroid_ref(corners):
    """(n, 3, 3) float32 corners -> (cen, rho) in float64, the five steps in their order: ((a + b) + c) / 3 per axis; e = corner - cen;
    (ex ex + ey ey) + ez ez; fmax over the three, starting from 0; sqrt"""
    p = corners.astype(F64)
    cen = ((p[:, 0] + p[:, 1]) + p[:, 2]) / 3.0
    rho2 = np.zeros(len(p))
    for k in range(3):
        e = p[:, k] - cen
        rho2 = np.fmax(rho2, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    return cen, np.sqrt(rho2)


def faces_under_test():
    rng = np.random.default_rng(20261)
    named = {
        'equal corners': np.tile(F32([3.25, -7.5, 11.0]), (3, 1)),
        'collinear': F32([[0, 0, 0], [1, 2, 3], [3, 6, 9]]),
        'needle, aspect 1e4': F32([[0, 0, 0], [1e4, 0, 0], [5e3, 1, 0]]),
        'edge 1 at 1e6': F32([[1e6, 1e6, 1e6], [1e6 + 1, 1e6, 1e6], [1e6, 1e6 + 1, 1e6]]),
        'corners at +-3e38': F32([[3e38, -3e38, 3e38], [-3e38, 3e38, 3e38], [3e38, 3e38, -3e38]]),
        'denormal corners': np.array([[1, 0, 0], [0, 3, 0], [0, 0, 7]], np.uint32).view(F32).reshape(3, 3),
    }
    rand = (rng.standard_normal((1000, 3, 3)) * np.exp(rng.uniform(-8, 8, (1000, 1, 1)))).astype(F32)
    rand[::5] += F32(1e4) * rng.standard_normal((200, 1, 3)).astype(F32)           # a fifth of them far from the origin
    return named, np.concatenate([rand] + [v[None] for v in named.values()])


def test_the_constants_are_the_ones_the_units_had(shim):
    out = np.zeros(4, np.int64)
    shim.shim_rule(out.ctypes.data)
    assert tuple(int(v) for v in out) == RULE
    assert shim.shim_slack() == SLACK


def test_one_centroid_and_radius_bit_for_bit(shim):
    named, corners = faces_under_test()
    assert corners.dtype == F32 and corners.shape == (1006, 3, 3) and np.isfinite(corners).all()
    d = named['denormal corners']
    assert (d[d != 0] < np.finfo(F32).tiny).all() and (d[d != 0] > 0).all() and np.count_nonzero(d) == 3
    cen_ref, rho_ref = centroid_ref(corners)
    assert np.isfinite(cen_ref).all() and np.isfinite(rho_ref).all()
    assert rho_ref[1000] == 0.0 and (rho_ref[1001:] > 0.0).all()                     # three equal corners: rho == 0
    assert rho_ref[-1] < 1e-44 and rho_ref[-2] > 3e38
    got = []
    for which in range(3):
        cen, rho = np.full((len(corners), 3), np.nan), np.full(len(corners), np.nan)
        shim.shim_centroids(which, np.ascontiguousarray(corners).ctypes.data, len(corners), cen.ctypes.data, rho.ctypes.data)
        got.append((cen, rho))
        assert np.array_equal(bits(cen), bits(cen_ref)), which
        assert np.array_equal(bits(rho), bits(rho_ref)), which
    # the two forwards return the bits of the one definition
    for cen, rho in got[1:]:
        assert np.array_equal(bits(cen), bits(got[0][0])) and np.array_equal(bits(rho), bits(got[0][1]))


def test_every_corner_lies_within_the_enlarged_radius(shim):
    """in exact rational arithmetic: |corner - cen|^2 <= (rho (1 + 1e-9))^2 with cen and the enlarged rho as the kernels store them"""
    _, corners = faces_under_test()
    cen, rho = np.zeros((len(corners), 3)), np.zeros(len(corners))
    shim.shim_centroids(0, np.ascontiguousarray(corners).ctypes.data, len(corners), cen.ctypes.data, rho.ctypes.data)
    stored = rho * (1.0 + SLACK)
    for f in range(len(corners)):
        r2 = Fraction(float(stored[f])) ** 2
        for k in range(3):
            d2 = sum((Fraction(float(corners[f, k, a])) - Fraction(float(cen[f, a]))) ** 2 for a in range(3))
            assert d2 <= r2, (f, k, float(d2), float(r2))


# ---- the cell size ----------------------------------------------------------------------------------------------------------------------
def cmax(a, b):
    return b if a < b else a                                   # std::max


def cmin(a, b):
    return a if not b < a else b                               # std::min


def settle(h, emax):
    """the tail the six set_mesh / starting_cell bodies shared: h is kept unless it is not a positive finite number"""
    return h if (h > 0.0 and np.isfinite(h)) else emax


def cell_fixed(rho_sum, nf, rho_max, d_cap, emax):
    """nwd_, nwx_, nwc_set_mesh: g.h = 1; if emax > 0: g.h = max(2 sum / nf, emax / 1024), then the fallback"""
    if not emax > 0.0:
        return 1.0
    return settle(cmax(2.0 * rho_sum / float(nf), emax / 1024.0), emax)


def cell_band(rho_sum, nf, rho_max, d_cap, emax):
    """nwv_, nwl_ starting_cell with rho_mean = sum / nf: max(max(2 m, (d_cap + rho_max) / 2), emax / 1024)"""
    if not emax > 0.0:
        return 1.0
    m = rho_sum / float(nf)
    return settle(cmax(cmax(2.0 * m, (d_cap + rho_max) / 2.0), emax / 1024.0), emax)


def cell_proximity(rho_sum, nf, rho_max, d_cap, emax):
    """nwm_ starting_cell without a cell size of the caller's: max(2 m, min((d_cap + rho_max) / 2, 16 m)), then the floor"""
    if not emax > 0.0:
        return 1.0
    m = rho_sum / float(nf)
    h = cmax(2.0 * m, cmin((d_cap + rho_max) / 2.0, 16.0 * m))
    return settle(cmax(h, emax / 1024.0), emax)


CELL_RULES = [cell_fixed, cell_band, cell_proximity]


@pytest.mark.parametrize('unit', [0, 1, 2])
def test_starting_cell_size_is_what_each_unit_computed(shim, unit):
    with np.errstate(all='ignore'):
        seen = set()
        for emax in (0.0, 1e-30, 1.0, 1e30):
            for rho_sum, nf, rho_max in ((0.0, 1, 0.0), (0.0, 320, 0.0), (1.0, 3, 0.4), (223.6067977, 320, 0.9), (1e-3, 7, 1e-3), (1e25, 3, 5e24),
                                         (4.9e-324, 3, 4.9e-324), (1e300, 7, 1e300)):
                for d_cap in (1e-3, 0.5, 3.0, 1e6, 2.0 ** 40, np.inf):
                    want = CELL_RULES[unit](rho_sum, nf, rho_max, d_cap, emax)
                    got = shim.shim_cell(unit, rho_sum, nf, rho_max, d_cap, emax)
                    assert bits(got) == bits(want), (unit, emax, rho_sum, nf, rho_max, d_cap, got, want)
                    assert got > 0.0 and np.isfinite(got)
                    seen.add('one' if emax == 0.0 else 'floor' if got == emax / 1024.0 else 'emax' if got == emax else 'candidate')
        # every branch is taken: no extent, the floor (a mean rho of 0), the candidate, and under an infinite band the fallback to emax,
        # which only the volume and mapping units' candidate can reach (the proximity unit's is capped at 16 m)
        assert seen == ({'one', 'floor', 'emax', 'candidate'} if unit == 1 else {'one', 'floor', 'candidate'})


def test_twice_the_mean_is_the_mean_of_twice(shim):
    """2 (sum / F) == (2 sum) / F in float64 (doubling is exact): the one form that is kept gives what nwd_set_mesh's gave"""
    rng = np.random.default_rng(7)
    for rho_sum, nf in zip(np.exp(rng.uniform(-30, 30, 2000)), rng.integers(1, 1 << 29, 2000)):
        assert bits(2.0 * (rho_sum / float(nf))) == bits(2.0 * rho_sum / float(nf))
        assert bits(shim.shim_cell(0, rho_sum, int(nf), 0.0, 1.0, 1e-300)) == bits(2.0 * rho_sum / float(nf))


# ---- when the centroids are binned anew -------------------------------------------------------------------------------------------------
def size_grid_ref(n, ext, h):
    cap = min(max(RULE[0] * n, 65536), RULE[1])
    for _ in range(RULE[3]):
        dims = [int(min(float(RULE[2]), np.floor(e / h) + 1.0)) for e in ext]
        if dims[0] * dims[1] * dims[2] <= cap:
            break
        h *= 1.1
    return dims[0] * dims[1] * dims[2] <= cap, h, dims


def bins(L, nf, ext, h0, h_start, h, dims):
    ext = np.ascontiguousarray(ext, F64)
    hs, hh, dd = ctypes.c_double(h_start), ctypes.c_double(h), np.array(dims, np.int32)
    r = L.shim_bins(nf, ext.ctypes.data, h0, ctypes.byref(hs), ctypes.byref(hh), dd.ctypes.data)
    return r, hs.value, hh.value, [int(d) for d in dd]


def test_the_grid_at_hand_is_kept_for_the_same_starting_cell(shim):
    KEPT, NEW, NONE = 0, 1, 2
    ext = [20.0, 20.0, 0.0]
    # no grid at hand (h_start == 0): sized anew; h_start stays 0 until the caller has binned
    r, hs, h, dims = bins(shim, 320, ext, 2.5, 0.0, -1.0, [-1, -1, -1])
    ok, h_ref, dims_ref = size_grid_ref(320, ext, 2.5)
    assert ok and (r, hs) == (NEW, 0.0) and bits(h) == bits(h_ref) and dims == dims_ref == [9, 9, 1]
    # the same starting cell: kept, nothing is touched -- also when the grid had been widened from it (h != h_start)
    assert bins(shim, 320, ext, 2.5, 2.5, 2.75, [8, 8, 1]) == (KEPT, 2.5, 2.75, [8, 8, 1])
    # another one, by one ulp: anew
    h0 = float(np.nextafter(2.5, 3.0))
    r, hs, h, dims = bins(shim, 320, ext, h0, 2.5, 2.5, [9, 9, 1])
    assert (r, hs) == (NEW, 0.0) and bits(h) == bits(h0) and dims == size_grid_ref(320, ext, h0)[2]
    # a starting cell far too fine: widened by tenths to the cap, as size_grid_ref does
    r, hs, h, dims = bins(shim, 320, [20.0, 20.0, 20.0], 1e-3, 2.5, 2.5, [9, 9, 9])
    ok, h_ref, dims_ref = size_grid_ref(320, [20.0, 20.0, 20.0], 1e-3)
    assert ok and h_ref > 0.4 and (r, hs) == (NEW, 0.0) and bits(h) == bits(h_ref) and dims == dims_ref
    # no cell size within 400 widenings: refused, and the grid at hand is forgotten
    r, hs, h, dims = bins(shim, 320, [1e30, 1e30, 1e30], 1.0, 2.5, 2.5, [9, 9, 9])
    assert not size_grid_ref(320, [1e30, 1e30, 1e30], 1.0)[0] and (r, hs) == (NONE, 0.0) and dims == [1025, 1025, 1025]
    # a starting cell that is not a number is never the one at hand
    assert bins(shim, 320, ext, float('nan'), float('nan'), 2.5, [9, 9, 1])[:2] == (NONE, 0.0)
