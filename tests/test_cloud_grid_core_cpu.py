"""
The HIP-free half of the cloud query units' cloud grid (ch_shrinkwrap_amd/csrc/nw_bq_core.h), settled on the CPU: the cell size a cloud
grid starts from (bq::cloud_cell), its limits (bq::CLOUD_GRID_RULE), the decision to keep the grid at hand or to bin anew under any rule
(bq::keep_or_rebin) and the cloud point in cell order (bq::PtF32), which is the point of the clustering, pairs and structure cores.
This test compiles the header and those three cores with g++ into a shim of its own, built on demand in pytest's temporary directory,
and compares with restatements here; the starting cells are also compared with the bodies the three units had before they shared one.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')
F32, F64 = np.float32, np.float64
RULE = (2, 1 << 26, 1025, 400)                  # CLOUD_GRID_RULE
FACE_RULE = (16, 1 << 26, 1025, 400)            # FACE_GRID_RULE
KEPT, NEW, NONE = 0, 1, 2

SHIM = r'''
#include <cstddef>
#include <type_traits>
#include "nw_bq_core.h"
#include "nw_clustering_core.h"
#include "nw_pairs_core.h"
#include "nw_structure_core.h"
static_assert(std::is_same<nwp_pt, bq::PtF32>::value && std::is_same<nwq_pt, bq::PtF32>::value && std::is_same<nwf_pt, bq::PtF32>::value,
              "the three cores' point is the cloud grid's");
extern "C" double shim_cloud_cell(double candidate, double emax) { return bq::cloud_cell(candidate, emax); }
// the candidates of the three units: NWP_CELL_OF_EPS of eps, NWQ_CELL_OF_RMAX of the largest radius, NWF_CELL_OF_R of the radius
extern "C" double shim_unit_cell(int unit, double x, double emax)
{
    return bq::cloud_cell((unit == 0 ? NWP_CELL_OF_EPS : unit == 1 ? NWQ_CELL_OF_RMAX : NWF_CELL_OF_R) * x, emax);
}
extern "C" void shim_rule(long long *out)
{
    out[0] = bq::CLOUD_GRID_RULE.cells_per_point; out[1] = bq::CLOUD_GRID_RULE.max_cells; out[2] = bq::CLOUD_GRID_RULE.max_dim; out[3] = bq::CLOUD_GRID_RULE.widen_steps;
}
extern "C" int shim_size(long long n, const double *ext, double *h, int *dims, long long *cap)
{
    *cap = bq::grid_cap(bq::CLOUD_GRID_RULE, n);
    return bq::size_grid(bq::CLOUD_GRID_RULE, n, ext, h, dims) ? 1 : 0;
}
// which = 0: keep_or_rebin under CLOUD_GRID_RULE, 1: under FACE_GRID_RULE, 2: face_bins
extern "C" int shim_bins(int which, long long n, const double *ext, double h0, double *h_start, double *h, int *dims)
{
    if (which == 2) return (int)bq::face_bins(n, ext, h0, h_start, h, dims);
    return (int)bq::keep_or_rebin(which == 0 ? bq::CLOUD_GRID_RULE : bq::FACE_GRID_RULE, n, ext, h0, h_start, h, dims);
}
extern "C" void shim_layout(long long *out)
{
    out[0] = sizeof(bq::PtF32); out[1] = alignof(bq::PtF32); out[2] = offsetof(bq::PtF32, x); out[3] = offsetof(bq::PtF32, y);
    out[4] = offsetof(bq::PtF32, z); out[5] = offsetof(bq::PtF32, i);
    out[6] = std::is_same<nwp_pt, bq::PtF32>::value; out[7] = std::is_same<nwq_pt, bq::PtF32>::value; out[8] = std::is_same<nwf_pt, bq::PtF32>::value;
    out[9] = std::is_same<decltype(bq::PtF32::i), int>::value && std::is_same<decltype(bq::PtF32::x), float>::value;
}
'''


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('cloud_grid_shim')
    src, lib = os.path.join(str(d), 'shim.cpp'), os.path.join(str(d), 'libcloud_grid_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    # (plain g++, no HIP header on the include path: the headers must not need one)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-Werror',
                           '-I', CSRC, '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp, ll, dbl = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double
    L.shim_cloud_cell.argtypes, L.shim_cloud_cell.restype = [dbl, dbl], dbl
    L.shim_unit_cell.argtypes, L.shim_unit_cell.restype = [ctypes.c_int, dbl, dbl], dbl
    L.shim_rule.argtypes = [vp]
    L.shim_size.argtypes = [ll, vp, vp, vp, vp]
    L.shim_bins.argtypes = [ctypes.c_int, ll, vp, dbl, vp, vp, vp]
    L.shim_layout.argtypes = [vp]
    return L


def bits(x):
    return int(F64(x).view(np.uint64))


# ---- the starting cell ------------------------------------------------------------------------------------------------------------------
def positive_finite_float(x):
    with np.errstate(over='ignore', invalid='ignore'):
        f = F32(x)
    return bool(f > 0) and bool(np.isfinite(f))


def cloud_cell_ref(candidate, emax):
    """h = max(candidate, emax / 1024) (std::max: the first unless it is smaller); if (float)h is no positive finite float: emax if it
    is positive and a finite float, else 1"""
    floor = F64(emax) / F64(1024.0)
    h = floor if F64(candidate) < floor else F64(candidate)
    if not positive_finite_float(h):
        with np.errstate(over='ignore'):
            h = F64(emax) if (emax > 0.0 and bool(np.isfinite(F32(emax)))) else F64(1.0)
    return float(h)


# (candidate, emax) -> what comes out
CELL_CASES = [
    ('zero extent, zero candidate', 0.0, 0.0, 1.0),
    ('zero extent, positive candidate', 0.75, 0.0, 0.75),
    ('a candidate below the floor', 1e-3, 2048.0, 2.0),
    ('a candidate above the floor', 3.0, 2048.0, 3.0),
    ('a candidate whose float is 0, no extent', 1e-50, 0.0, 1.0),
    ('a candidate whose float is 0, an extent', 1e-50, 2048.0, 2.0),
    ('a candidate whose float is 0, an extent whose floor is 0 as a float', 1e-50, 1e-44, 1e-44),
    ('an infinite candidate, a finite extent', np.inf, 10.0, 10.0),
    ('a candidate beyond float, a finite extent', 1e39, 10.0, 10.0),
    ('an infinite candidate, an extent beyond float', np.inf, 1e39, 1.0),
    ('a candidate beyond float, an extent beyond float', 1e39, 1e39, 1.0),
    ('a candidate that is not a number', np.nan, 10.0, 10.0),
    ('a candidate that is not a number, no extent', np.nan, 0.0, 1.0),
    ('a negative candidate', -1.0, 10.0, 10.0 / 1024.0),
]


@pytest.mark.parametrize('case', CELL_CASES, ids=[c[0] for c in CELL_CASES])
def test_cloud_cell_is_the_restatement_bit_for_bit(shim, case):
    _, candidate, emax, expected = case
    got = shim.shim_cloud_cell(candidate, emax)
    print('candidate %r emax %r -> %.17g' % (candidate, emax, got))
    assert bits(got) == bits(cloud_cell_ref(candidate, emax)) == bits(expected)


# The three bodies the units had before they shared bq::cloud_cell, restated from their source (nw_clustering.hip, nw_pairs.hip,
# nw_structure.hip; the box is the float box of bq::bounds<float>):
#     double emax = 0.0;
#     for (int d = 0; d < 3; ++d) emax = std::max(emax, (double)ctx->g.hi[d] - (double)ctx->g.lo[d]);
#     double h = std::max(K * x, emax / 1024.0);
#     if (!((float)h > 0.0f) || !std::isfinite((float)h)) h = (emax > 0.0 && std::isfinite((float)emax)) ? emax : 1.0;
#     return h;
# with K * x = NWP_CELL_OF_EPS * eps, ctx->cell_of_rmax * r_max (NWQ_CELL_OF_RMAX unless the developer knob is set), NWF_CELL_OF_R * r.
CELL_OF = (0.57, 0.5, 0.5)


def former_emax(lo, hi):
    emax = F64(0.0)
    for d in range(3):
        e = F64(hi[d]) - F64(lo[d])
        emax = e if emax < e else emax
    return float(emax)


def former_starting_cell(unit, x, emax):
    with np.errstate(over='ignore', invalid='ignore'):
        cand = F64(CELL_OF[unit]) * F64(x)
        floor = F64(emax) / F64(1024.0)
        h = floor if cand < floor else cand
        fh, fe = F32(h), F32(emax)
        if not (fh > 0) or not np.isfinite(fh):
            h = F64(emax) if (emax > 0.0 and np.isfinite(fe)) else F64(1.0)
    return float(h)


@pytest.mark.parametrize('unit', [0, 1, 2], ids=['clustering', 'pairs', 'structure'])
def test_the_starting_cell_is_what_each_unit_computed(shim, unit):
    rng = np.random.default_rng(20 + unit)
    pairs = [(c[1], c[2]) for c in CELL_CASES]
    # 1 000 random (x, box) pairs: x and the extents log-uniform over sixty decades, so that each branch is taken many times
    for _ in range(1000):
        x = float(10.0 ** rng.uniform(-50.0, 42.0))
        lo = (rng.normal(size=3) * 10.0 ** rng.uniform(-3.0, 6.0)).astype(F32)
        ext = np.where(rng.random(3) < 0.25, 0.0, 10.0 ** rng.uniform(-45.0, 38.5, 3))
        with np.errstate(over='ignore'):
            hi = (lo.astype(F64) + ext).astype(F32)
        hi = np.where(np.isfinite(hi), hi, lo)
        pairs.append((x, former_emax(lo, np.maximum(lo, hi))))
    seen = set()
    for x, emax in pairs:
        got = shim.shim_unit_cell(unit, x, emax)
        ref = former_starting_cell(unit, x, emax)
        assert bits(got) == bits(ref), (x, emax, got, ref)
        with np.errstate(over='ignore', invalid='ignore'):
            cand = float(F64(CELL_OF[unit]) * F64(x))
        assert bits(got) == bits(cloud_cell_ref(cand, emax))
        seen.add('one' if got == 1.0 and emax != 1.0 and cand != 1.0 else 'emax' if got == emax else 'floor' if got == emax / 1024.0 else 'candidate')
    print(sorted(seen))
    assert seen == {'one', 'emax', 'floor', 'candidate'}


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def size(L, n, ext, h):
    ext = np.ascontiguousarray(ext, F64)
    hh, dims, cap = ctypes.c_double(h), np.zeros(3, np.int32), ctypes.c_longlong()
    ok = L.shim_size(n, ext.ctypes.data, ctypes.byref(hh), dims.ctypes.data, ctypes.byref(cap))
    return bool(ok), hh.value, [int(d) for d in dims], cap.value


def size_grid_ref(rule, n, ext, h):
    cap = min(max(rule[0] * n, 65536), rule[1])
    dims = [0, 0, 0]
    for _ in range(rule[3]):
        dims = [int(min(float(rule[2]), np.floor(e / h) + 1.0)) for e in ext]
        if dims[0] * dims[1] * dims[2] <= cap:
            break
        h *= 1.1
    return dims[0] * dims[1] * dims[2] <= cap, h, dims, cap


def test_the_cloud_grid_rule(shim):
    out = np.zeros(4, np.int64)
    shim.shim_rule(out.ctypes.data)
    assert tuple(int(v) for v in out) == RULE == (2, 1 << 26, 1025, 400)
    ext = [100.0, 100.0, 100.0]
    for n, cap_expected in ((1, 65536), (32768, 65536), (1 << 25, 1 << 26), (1 << 30, 1 << 26), (40000, 80000)):
        ok, h, dims, cap = size(shim, n, ext, 1e-3)            # far too fine: widened by tenths to the cap, 1 025 cells an axis at first
        ok_ref, h_ref, dims_ref, cap_ref = size_grid_ref(RULE, n, ext, 1e-3)
        print('n %d: cap %d, h %.17g, dims %s' % (n, cap, h, dims))
        assert cap == cap_ref == cap_expected
        assert ok and ok_ref and bits(h) == bits(h_ref) and dims == dims_ref and dims[0] * dims[1] * dims[2] <= cap
    # at most 1 025 cells an axis, whatever the extent: a line of 2^30 points has the cap to spare
    ok, h, dims, cap = size(shim, 1 << 30, [1e6, 0.0, 0.0], 1.0)
    assert ok and h == 1.0 and dims == [1025, 1, 1]
    ok, h, dims, cap = size(shim, 1 << 30, [1024.0, 0.0, 0.0], 1.0)
    assert ok and dims == [1025, 1, 1]
    ok, h, dims, cap = size(shim, 1 << 30, [1023.5, 0.0, 0.0], 1.0)
    assert ok and dims == [1024, 1, 1]


# ---- keep or bin anew -------------------------------------------------------------------------------------------------------------------
def bins(L, which, n, ext, h0, h_start, h, dims):
    ext = np.ascontiguousarray(ext, F64)
    hs, hh, dd = ctypes.c_double(h_start), ctypes.c_double(h), np.array(dims, np.int32)
    r = L.shim_bins(which, n, ext.ctypes.data, h0, ctypes.byref(hs), ctypes.byref(hh), dd.ctypes.data)
    return r, hs.value, hh.value, [int(d) for d in dd]


def test_the_grid_at_hand_is_kept_for_the_same_starting_cell(shim):
    ext = [20.0, 20.0, 0.0]
    # no grid at hand (h_start == 0): sized anew; h_start stays 0 until the caller has binned
    r, hs, h, dims = bins(shim, 0, 320, ext, 2.5, 0.0, -1.0, [-1, -1, -1])
    assert (r, hs) == (NEW, 0.0) and bits(h) == bits(2.5) and dims == [9, 9, 1]
    # the same starting cell: kept, nothing is touched -- also when the grid had been widened from it (h != h_start)
    assert bins(shim, 0, 320, ext, 2.5, 2.5, 2.75, [8, 8, 1]) == (KEPT, 2.5, 2.75, [8, 8, 1])
    # another one, by one ulp: anew
    h0 = float(np.nextafter(2.5, 3.0))
    r, hs, h, dims = bins(shim, 0, 320, ext, h0, 2.5, 2.5, [9, 9, 1])
    assert (r, hs) == (NEW, 0.0) and bits(h) == bits(h0) and dims == size_grid_ref(RULE, 320, ext, h0)[2]
    # a starting cell far too fine: widened by tenths to the cap of the rule it was called with
    for which, rule in ((0, RULE), (1, FACE_RULE)):
        r, hs, h, dims = bins(shim, which, 100000, [20.0, 20.0, 20.0], 1e-3, 2.5, 2.5, [9, 9, 9])
        ok, h_ref, dims_ref, _ = size_grid_ref(rule, 100000, [20.0, 20.0, 20.0], 1e-3)
        assert ok and (r, hs) == (NEW, 0.0) and bits(h) == bits(h_ref) and dims == dims_ref
    assert size_grid_ref(RULE, 100000, [20.0] * 3, 1e-3)[2] != size_grid_ref(FACE_RULE, 100000, [20.0] * 3, 1e-3)[2]      # (the rule counts)
    # no cell size within 400 widenings: refused, and the grid at hand is forgotten
    r, hs, h, dims = bins(shim, 0, 320, [1e30, 1e30, 1e30], 1.0, 2.5, 2.5, [9, 9, 9])
    assert not size_grid_ref(RULE, 320, [1e30, 1e30, 1e30], 1.0)[0] and (r, hs) == (NONE, 0.0) and dims == [1025, 1025, 1025]
    # a starting cell that is not a number is never the one at hand
    assert bins(shim, 0, 320, ext, float('nan'), float('nan'), 2.5, [9, 9, 1])[:2] == (NONE, 0.0)


def test_face_bins_is_the_same_rule_under_the_face_grids_limits(shim):
    rng = np.random.default_rng(5)
    calls = [(320, [20.0, 20.0, 0.0], 2.5, 0.0), (320, [20.0, 20.0, 0.0], 2.5, 2.5), (320, [1e30, 1e30, 1e30], 1.0, 2.5),
             (320, [20.0, 20.0, 0.0], float('nan'), float('nan')), (100000, [20.0, 20.0, 20.0], 1e-3, 2.5)]
    for _ in range(200):
        h0 = float(10.0 ** rng.uniform(-4.0, 2.0))
        calls.append((int(rng.integers(1, 1 << 22)), list(10.0 ** rng.uniform(-2.0, 4.0, 3)), h0, h0 if rng.random() < 0.3 else float(rng.random())))
    outcomes = set()
    for n, ext, h0, h_start in calls:
        a = bins(shim, 1, n, ext, h0, h_start, -3.0, [7, 7, 7])
        b = bins(shim, 2, n, ext, h0, h_start, -3.0, [7, 7, 7])
        assert (a[0], bits(a[1]), bits(a[2]), a[3]) == (b[0], bits(b[1]), bits(b[2]), b[3]), (n, ext, h0, h_start)
        outcomes.add(a[0])
    assert outcomes == {KEPT, NEW, NONE}


# ---- the point --------------------------------------------------------------------------------------------------------------------------
def test_the_cloud_point_is_sixteen_bytes_with_the_index_in_the_fourth_word(shim):
    out = np.full(10, -1, np.int64)
    shim.shim_layout(out.ctypes.data)
    size_of, align_of, ox, oy, oz, oi = (int(v) for v in out[:6])
    assert size_of == 16 and align_of == 16 and (ox, oy, oz, oi) == (0, 4, 8, 12)
    assert tuple(out[6:9]) == (1, 1, 1)                          # nwp_pt, nwq_pt and nwf_pt are bq::PtF32, not look-alikes
    assert out[9] == 1                                           # three floats and an int
    for core, name in (('nw_clustering_core.h', 'nwp_pt'), ('nw_pairs_core.h', 'nwq_pt'), ('nw_structure_core.h', 'nwf_pt')):
        txt = open(os.path.join(CSRC, core)).read()
        assert 'typedef bq::PtF32 %s;' % name in txt and 'struct alignas(16) %s' % name not in txt
    # one float point: the shared header's, and nothing else in csrc/ defines a struct of that shape for the cloud
    assert open(os.path.join(CSRC, 'nw_bq_core.h')).read().count('struct alignas(16) PtF32') == 1
    assert 'typedef PtF32 point;' in open(os.path.join(CSRC, 'nw_bq.h')).read()
