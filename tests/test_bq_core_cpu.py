"""
What the query units share and need no GPU for, settled on the CPU: ch_shrinkwrap_amd/csrc/nw_bq_core.h holds the sizing of the point
grid (the widening loop, the cells per axis and the cap, parameterised by each user's rule) and the bin rule and bin walk of the 64-bit
radix select.  This test compiles it with g++ into a shim of its own, built on demand in pytest's temporary directory, and compares
  - the sizing under the metric's rule with grid_of of tests/test_hip_evaluation_edges.py, on that file's reference clouds;
  - the sizing under hole punching's rule with a restatement here, on the six grids of test_candidate_faces_off_the_origin;
  - the select with numpy.sort on the value lists of tests/isosurface_ref.py.
The starting cell size is each unit's own (nw_evaluation.hip, nw_holepunch.hip) and is restated here from those.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from isosurface_ref import SELECT_VALUES
from test_hip_evaluation_edges import NEAREST_CASES, grid_of, reference_cloud
from test_hip_holepunch import OFFSETS, _step1_scene

CORE = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_bq_core.h')
F32 = np.float32

SHIM = r'''
#include "nw_bq_core.h"
extern "C" int shim_size_grid(int cells_per_point, long long max_cells, int max_dim, int widen_steps, long long n, const double *ext, double *h, int *dims,
                              long long *cap)
{
    const bq::GridRule rule = {cells_per_point, max_cells, max_dim, widen_steps};
    *cap = bq::grid_cap(rule, n);
    return bq::size_grid(rule, n, ext, h, dims) ? 1 : 0;
}
extern "C" int shim_select_bin(const unsigned *hist, long long *rank)
{
    int64_t r = *rank;
    const int b = bq::select_bin(hist, r);
    *rank = r;
    return b;
}
// the loop of bq::select_u64 with the histogram pass on the host: bin radix_bin(key, prefix, shift) of every key
extern "C" int shim_select(const unsigned long long *keys, long long n, int shift, long long rank, unsigned long long *key_out, long long *rank_out)
{
    uint64_t prefix = 0;
    int64_t r = rank;
    for (; shift >= 0; shift -= 8) {
        unsigned hist[256] = {0};
        for (long long i = 0; i < n; ++i) {
            const int b = bq::radix_bin(keys[i], prefix, shift);
            if (b >= 0) ++hist[b];
        }
        const int b = bq::select_bin(hist, r);
        if (b < 0) return 0;
        prefix = (prefix << 8) | (uint64_t)b;
    }
    *key_out = prefix;
    *rank_out = r;
    return 1;
}
'''

RULE_EVALUATION = (2, 1 << 28, 1025, 400)       # NWE_GRID_RULE
RULE_HOLEPUNCH = (4, 1 << 30, 2048, 200)        # NWH_GRID_RULE


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('bq_shim')
    src, lib = os.path.join(str(d), 'shim.cpp'), os.path.join(str(d), 'libbq_shim.so')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    # (plain g++, no HIP header on the include path: the header must not need one)
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-Werror',
                           '-I', os.path.dirname(CORE), '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    L.shim_size_grid.argtypes = [ctypes.c_int, ll, ctypes.c_int, ctypes.c_int, ll, vp, vp, vp, vp]
    L.shim_select_bin.argtypes = [vp, vp]
    L.shim_select.argtypes = [vp, ll, ctypes.c_int, ll, vp, vp]
    return L


def size_grid(L, rule, n, ext, h):
    """-> (fits, h, dims, cap)"""
    ext = np.ascontiguousarray(ext, np.float64)
    hh, dims, cap = ctypes.c_double(h), np.zeros(3, np.int32), ctypes.c_longlong()
    ok = L.shim_size_grid(rule[0], rule[1], rule[2], rule[3], n, ext.ctypes.data, ctypes.byref(hh), dims.ctypes.data, ctypes.byref(cap))
    return bool(ok), hh.value, tuple(int(d) for d in dims), cap.value


def test_the_core_header_includes_no_hip_header():
    txt = open(CORE).read()
    assert 'hip_runtime' not in txt and '#include <hip' not in txt


# ---- grid sizing, the metric's rule -----------------------------------------------------------------------------------------------------
def evaluation_start_h(ref):
    """the cell size nearest_dev of nw_evaluation.hip starts the widening from (the first half of grid_of)"""
    n = ref.shape[0]
    ext = ref.max(0) - ref.min(0)
    emax = float(ext.max())
    if not emax > 0.0:
        return ext, 1.0
    e = np.maximum(ext, 1e-3 * emax)
    return ext, max(float(np.cbrt(e[0] * e[1] * e[2] / n)), emax / 1024.0)


@pytest.mark.parametrize('name', NEAREST_CASES)
def test_grid_sizing_under_the_metrics_rule(shim, name):
    ref = reference_cloud(name)
    g = grid_of(ref)
    ext, h0 = evaluation_start_h(ref)
    ok, h, dims, cap = size_grid(shim, RULE_EVALUATION, ref.shape[0], ext, h0)
    print('%s: start h %.17g, h %.17g (grid_of %.17g), dims %s, cap %d, widened %d' % (name, h0, h, g.h, dims, cap, g.widened))
    assert ok and cap == g.cap
    assert np.float64(h).view(np.uint64) == np.float64(g.h).view(np.uint64)
    assert dims == g.dims
    assert (h != h0) == (g.widened > 0)


# ---- grid sizing, hole punching's rule --------------------------------------------------------------------------------------------------
def holepunch_grid(pts, cell_size):
    """nwh_set_points' sizing restated: float32 box and extent, the starting cell size in double, then the widening with hole punching's
    constants -> (ext, start h, h, dims, cap, widened)"""
    n = pts.shape[0]
    assert pts.dtype == F32
    ext = pts.max(0) - pts.min(0)                              # float32 differences
    emax = max(F32(ext.max()), F32(1e-3))
    e = np.maximum(ext.astype(np.float64), 1e-3 * float(emax))
    h = float(cell_size) if cell_size > 0 else float(np.cbrt(e[0] * e[1] * e[2] / n))
    h0 = h = max(h, float(emax) / 2048.0)
    cap = min(max(4 * n, 65536), 1 << 30)
    for widened in range(200):
        dims = np.minimum(2048.0, np.floor(ext.astype(np.float64) / h) + 1.0).astype(np.int64)
        if dims.prod() <= cap:
            break
        h *= 1.1
    return ext, emax, h0, h, tuple(int(d) for d in dims), cap, widened


@pytest.mark.parametrize('offset', list(OFFSETS))
@pytest.mark.parametrize('grid', ['auto', 'quarter', 'triple', 'capped', 'coplanar', 'single', 'fine'])
def test_grid_sizing_under_hole_punchings_rule(shim, grid, offset):
    """The six grids of test_candidate_faces_off_the_origin, none of which is widened, and `fine`: the `auto` scene with cells of 1 nm,
    which takes the widening loop to the cap."""
    pts, _, _, cell = _step1_scene('auto' if grid == 'fine' else grid, offset)
    if grid == 'fine':
        cell = 1.0
    ext, emax, h0, h_ref, dims_ref, cap_ref, widened = holepunch_grid(pts, cell)
    print('%s %s: n %d, ext %s, start h %.9g, h %.9g, dims %s, cap %d, widened %d' % (grid, offset, pts.shape[0], ext, h0, h_ref, dims_ref, cap_ref, widened))
    # the branch the case is named for
    if grid == 'auto':
        assert cell == 0.0 and widened == 0 and h0 > float(emax) / 2048.0          # the cube root, as it is
    elif grid == 'quarter':
        assert h0 == 12.5 and widened == 0 and np.prod(dims_ref) > 50000            # the caller's cell size, finer than `auto`, as it is
    elif grid == 'triple':
        assert h0 == 150.0 and widened == 0 and max(dims_ref) < 10                  # the caller's cell size, a handful of cells
    elif grid == 'capped':
        assert h0 == float(emax) / 2048.0 > 12.5 and dims_ref[0] == 2048           # the outlier's axis at the 2048 cells an axis may have
    elif grid == 'coplanar':
        assert ext[2] == 0.0 and dims_ref[2] == 1 and min(dims_ref[:2]) > 1         # no extent on one axis: a single layer of cells
    elif grid == 'single':
        assert (ext == 0.0).all() and emax == F32(1e-3) and dims_ref == (1, 1, 1)  # no extent at all: the floor of emax, one cell
    elif grid == 'fine':
        assert h0 == 1.0 and widened > 10 and np.prod(np.floor(ext / h0) + 1.0) > cap_ref > 0.5 * np.prod(dims_ref)      # widened to the cap
    else:
        raise KeyError(grid)
    ok, h, dims, cap = size_grid(shim, RULE_HOLEPUNCH, pts.shape[0], ext, h0)
    assert ok and cap == cap_ref
    assert np.float64(h).view(np.uint64) == np.float64(h_ref).view(np.uint64)
    assert dims == dims_ref


def test_grid_sizing_reports_a_grid_that_never_fits(shim):
    """a rule without widening steps left: the dims of the starting cell size are over the cap"""
    ok, h, dims, cap = size_grid(shim, (2, 1 << 28, 1025, 1), 10, [1000.0, 1000.0, 1000.0], 1.0)
    assert not ok and cap == 65536 and dims == (1001, 1001, 1001) and h == 1.1


# ---- the radix select -------------------------------------------------------------------------------------------------------------------
def select(L, values, rank, shift=56):
    keys = np.ascontiguousarray(values, np.uint64)
    key, left = ctypes.c_ulonglong(), ctypes.c_longlong()
    ok = L.shim_select(keys.ctypes.data, keys.size, shift, rank, ctypes.byref(key), ctypes.byref(left))
    return (key.value, left.value) if ok else None


@pytest.mark.parametrize('name', list(SELECT_VALUES))
def test_select_against_numpy_sort(shim, name):
    values = np.array(SELECT_VALUES[name], np.uint64)
    order = np.sort(values)
    if name in ('byte_ff', 'three_bytes_ffff'):                # the median's low byte(s) are 0xFF: the walk ends in the last bin
        assert int(order[(values.size - 1) // 2]) & 0xFF == 0xFF
    for rank in range(values.size):
        key, left = select(shim, values, rank)
        assert key == int(order[rank])
        assert left == rank - int((order < order[rank]).sum())       # the rank among the equal keys
        # started at the highest byte that holds a bit (nwi_threshold_auto skips the zero bytes above it)
        shift = 8 * ((int(values.max()).bit_length() - 1) // 8)
        assert select(shim, values, rank, shift) == (key, left)
    assert select(shim, values, values.size) is None and select(shim, values, -1) is None


def test_select_bin_at_the_last_bin_and_beyond(shim):
    hist = np.zeros(256, np.uint32)
    hist[3], hist[255] = 2, 3

    def walk(rank):
        r = ctypes.c_longlong(rank)
        return shim.shim_select_bin(hist.ctypes.data, ctypes.byref(r)), r.value

    assert walk(0) == (3, 0) and walk(1) == (3, 1)
    assert walk(2) == (255, 0) and walk(4) == (255, 2)         # bin 255 holds the rank
    assert walk(5)[0] == -1 and walk(10 ** 12)[0] == -1        # the histogram does not hold the rank
    assert walk(-1)[0] == -1
    assert shim.shim_select_bin(np.zeros(256, np.uint32).ctypes.data, ctypes.byref(ctypes.c_longlong(0))) == -1
