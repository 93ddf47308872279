"""
The volume's rules, settled without a GPU: ch_shrinkwrap_amd/csrc/nw_volume_core.h holds the node position, the capped walk over a
centroid grid handed in as arrays, the band rule, the predecessor rule and the quantisation as __host__ __device__ functions.  This
test compiles them for the CPU (g++ -ffp-contract=off) behind a shim of its own -- the loop over the nodes, the seed by brute force,
the sweep both as the three stages of lines the device runs and as one pass along nwv_predecessor -- and asks for the bits of the
NumPy restatement (tests/mesh_volume_ref.py): u, face, band membership and field, the signs by same_as_restatement's rule.  The grid
is binned here in NumPy, at four cell sizes.  The same source with a main of its own runs once under -fsanitize=address,undefined.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_distance_ref as D
import mesh_volume_ref as V
from conftest import ROOT
from ch_shrinkwrap_amd.trimesh import icosphere

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')

SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "nw_volume_core.h"
// -> 0, or 1 if the staged sweep and the pass along nwv_predecessor disagree
extern "C" int shim_volume(const float *pos, const int *faces, const int *twin, long long nf, const nwv_pt *pts, const int *cstart, const double *rho,
                           double rho_max, const double *glo, const double *ghi, double gh, const int *gdims, const float *lo, float h,
                           const int *dims, double d_cap, double *u_out, double *sd_out, int *face_out, unsigned long long *field_out,
                           unsigned char *mask_out, long long *rings_out, long long *centroids_out)
{
    nwv_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = glo[d]; g.hi[d] = ghi[d]; g.dims[d] = gdims[d]; }
    g.h = gh;
    const long long nx = dims[0], ny = dims[1], nz = dims[2], n = nx * ny * nz;
    for (long long idx = 0; idx < n; ++idx) {
        const long long i = idx % nx, j = (idx / nx) % ny, k = idx / (nx * ny);
        const double q[3] = {nwv_node_coord(lo[0], h, i), nwv_node_coord(lo[1], h, j), nwv_node_coord(lo[2], h, k)};
        nwv_best b;
        int n_cen = 0, capped = 0;
        rings_out[idx] = nwv_walk(q, pos, faces, (int)nf, pts, cstart, rho, rho_max, g, d_cap, b, n_cen);
        centroids_out[idx] = n_cen;
        u_out[idx] = b.d;
        sd_out[idx] = nwv_node_value(q, b, d_cap, pos, faces, twin, &face_out[idx], &capped);
    }
    int bad = 0;
    if (twin) {
        // the seed: all faces, no cap
        const double q[3] = {nwv_node_coord(lo[0], h, 0), nwv_node_coord(lo[1], h, 0), nwv_node_coord(lo[2], h, 0)};
        double best = INFINITY, bc[3] = {0, 0, 0}, N[3];
        int bf = -1, bfeat = 0;
        for (long long f = 0; f < nf; ++f) {
            double c[3];
            int feat;
            const double d2 = nwd_point_triangle(q, pos + 3 * (long long)faces[3 * f], pos + 3 * (long long)faces[3 * f + 1], pos + 3 * (long long)faces[3 * f + 2], c, &feat);
            if (d2 < best) { best = d2; bf = (int)f; bfeat = feat; bc[0] = c[0]; bc[1] = c[1]; bc[2] = c[2]; }
        }
        nwd_pseudonormal(pos, faces, twin, bf, bfeat, N);
        const double seed = (best > 0.0 && nwd_sign(q, bc, N) < 0.0) ? -1.0 : 1.0;
        std::vector<double> other(sd_out, sd_out + n);
        if (face_out[0] == -1) { sd_out[0] = nwv_out_of_band(d_cap, seed); other[0] = sd_out[0]; }
        for (int stage = 0; stage < 3; ++stage) {
            int64_t n_lines, pitch, len, stride;
            nwv_sweep_stage(stage, nx, ny, nz, &n_lines, &pitch, &len, &stride);
            for (int64_t L = 0; L < n_lines; ++L)
                for (int64_t t = 1; t < len; ++t) {
                    const int64_t idx = L * pitch + t * stride;
                    if (face_out[idx] == -1) sd_out[idx] = nwv_out_of_band(d_cap, sd_out[idx - stride]);
                }
        }
        for (long long idx = 1; idx < n; ++idx)
            if (face_out[idx] == -1) other[idx] = nwv_out_of_band(d_cap, other[nwv_predecessor(idx % nx, (idx / nx) % ny, idx / (nx * ny), nx, ny)]);
        for (long long idx = 0; idx < n; ++idx) bad |= other[idx] != sd_out[idx];
    }
    for (long long idx = 0; idx < n; ++idx) { field_out[idx] = nwv_quantise(sd_out[idx], d_cap); mask_out[idx] = sd_out[idx] < 0.0; }
    return bad;
}

#ifdef NWV_MAIN
// the same call on arrays read from a file: <in> holds 8 int64 counts (nv, nf, has_twin, npts, ncells, nx, ny, nz), then the arrays
template <class T> static std::vector<T> rd(FILE *fh, size_t n) { std::vector<T> v(n); if (n && fread(v.data(), sizeof(T), n, fh) != n) exit(3); return v; }
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    const std::vector<long long> c = rd<long long>(fh, 8);
    const auto pos = rd<float>(fh, 3 * c[0]);
    const auto faces = rd<int>(fh, 3 * c[1]);
    const auto twin = rd<int>(fh, c[2] ? 3 * c[1] : 0);
    const auto pts = rd<nwv_pt>(fh, c[3]);
    const auto cstart = rd<int>(fh, c[4] + 1);
    const auto rho = rd<double>(fh, c[1]);
    const auto dbl = rd<double>(fh, 9);                       // rho_max, glo[3], ghi[3], gh, d_cap
    const auto gdims = rd<int>(fh, 3);
    const auto lo = rd<float>(fh, 4);                         // lo[3], h
    fclose(fh);
    const int dims[3] = {(int)c[5], (int)c[6], (int)c[7]};
    const size_t n = (size_t)(c[5] * c[6] * c[7]);
    std::vector<double> u(n), sd(n);
    std::vector<int> face(n);
    std::vector<unsigned long long> field(n);
    std::vector<unsigned char> mask(n);
    std::vector<long long> rings(n), cen(n);
    const int bad = shim_volume(pos.data(), faces.data(), c[2] ? twin.data() : nullptr, c[1], pts.data(), cstart.data(), rho.data(), dbl[0], &dbl[1], &dbl[4],
                                dbl[7], gdims.data(), lo.data(), lo[3], dims, dbl[8], u.data(), sd.data(), face.data(), field.data(), mask.data(),
                                rings.data(), cen.data());
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    fwrite(sd.data(), sizeof(double), n, fh);
    fwrite(field.data(), sizeof(unsigned long long), n, fh);
    fwrite(face.data(), sizeof(int), n, fh);
    fclose(fh);
    return bad;
}
#endif
'''


def centroid_grid(vertices, faces, h_cell):
    """the centroid grid as the device bins it, in NumPy: (pts (F,) of nwv_pt in cell order, cstart, rho, rho_max, lo, hi, dims)"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    cen = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / 3.0
    rho = np.sqrt(((v[f] - cen[:, None, :]) ** 2).sum(2).max(1)) * (1.0 + 1e-9) + 1e-300
    lo, hi = cen.min(0), cen.max(0)
    dims = (np.floor((hi - lo) / h_cell) + 1).astype(np.int32)
    cell3 = np.minimum(np.maximum(np.floor((cen - lo) / h_cell), 0), dims - 1).astype(np.int64)
    cell = (cell3[:, 2] * dims[1] + cell3[:, 1]) * dims[0] + cell3[:, 0]
    order = np.argsort(cell, kind='stable')[::-1]                                           # (the order within a cell must not show)
    order = order[np.argsort(cell[order], kind='stable')]
    pts = np.zeros(len(f), np.dtype([('x', np.float64), ('y', np.float64), ('z', np.float64), ('i', np.int64)]))
    pts['x'], pts['y'], pts['z'], pts['i'] = cen[order, 0], cen[order, 1], cen[order, 2], order
    cstart = np.zeros(int(dims.prod()) + 1, np.int32)
    cstart[1:] = np.cumsum(np.bincount(cell, minlength=int(dims.prod())))
    return pts, cstart, rho, float(rho.max()), lo, hi, dims


def _source(tmp):
    src = os.path.join(str(tmp), 'shim.cpp')
    with open(src, 'w') as fh:
        fh.write(SHIM)
    return src


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp('nwv_shim')
    src, lib = _source(d), os.path.join(str(d), 'libnwv_shim.so')
    subprocess.check_call([os.environ.get('CXX', 'g++'), '-O2', '-std=c++14', '-fPIC', '-shared', '-ffp-contract=off', '-Wall', '-I', CSRC, '-o', lib, src])
    L = ctypes.CDLL(lib)
    vp, f64 = ctypes.c_void_p, ctypes.c_double
    L.shim_volume.argtypes = [vp, vp, vp, ctypes.c_longlong, vp, vp, vp, f64, vp, vp, f64, vp, vp, ctypes.c_float, vp, f64] + [vp] * 7
    L.shim_volume.restype = ctypes.c_int

    def run(vertices, faces, lo, h, dims, d_cap, h_cell, signed=True):
        v = np.ascontiguousarray(vertices, np.float32)
        f = np.ascontiguousarray(faces, np.int32)
        tw = np.ascontiguousarray(D.twins(f), np.int32) if signed else None
        pts, cstart, rho, rho_max, glo, ghi, gdims = centroid_grid(v, f, h_cell)
        lo32, dims32 = np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(dims, np.int32)
        n = int(np.prod(dims32))
        out = dict(u=np.empty(n), sd=np.empty(n), face=np.empty(n, np.int32), field=np.empty(n, np.uint64), mask=np.empty(n, np.uint8),
                   rings=np.empty(n, np.int64), centroids=np.empty(n, np.int64))
        p = lambda a: a.ctypes.data
        bad = L.shim_volume(p(v), p(f), None if tw is None else p(tw), f.shape[0], p(pts), p(cstart), p(rho), rho_max, p(glo), p(ghi), float(h_cell),
                            p(gdims), p(lo32), float(h), p(dims32), float(d_cap), *(p(out[k]) for k in ('u', 'sd', 'face', 'field', 'mask', 'rings', 'centroids')))
        assert bad == 0                                                                       # the staged sweep is the predecessor pass
        out['blob'] = (v, f, tw, pts, cstart, rho, rho_max, glo, ghi, gdims, lo32, dims32)
        return out
    return run


def check(mine, ref, signed, d_cap):
    band = ref['in_band']
    assert np.array_equal(D.bits(mine['u'][band]), D.bits(ref['u'][band]))                    # exact wherever it matters ...
    assert (mine['u'][~band] > d_cap).all()                                                   # ... and beyond the band elsewhere
    return V.same_as_restatement(mine, ref, signed)


CELLS = (0.3, 1.0, 2.7, 40.0)


@pytest.mark.parametrize('d_cap', [1.0, 2.0, 2.5])
def test_the_cube_lattice_at_four_cell_sizes(shim, d_cap):
    v, f = V.cube4()
    lo, h, dims = V.CUBE_LATTICE
    ref = V.volume(v, f, lo, h, dims, d_cap)
    for h_cell in CELLS:
        mine = shim(v, f, lo, h, dims, d_cap, h_cell)
        assert check(mine, ref, True, d_cap) == 729
    un = V.volume(v, f, lo, h, dims, d_cap, signed=False)
    assert check(shim(v, f, lo, h, dims, d_cap, 1.0, signed=False), un, False, d_cap) == 729


def test_the_node_at_exactly_d_cap(shim):
    v, f = V.cube4()
    lo, h, dims = V.CUBE_LATTICE
    at2 = np.flatnonzero(V.cube4_sdf(V.nodes(lo, h, dims)) == 2.0)
    for h_cell in CELLS:
        assert (shim(v, f, lo, h, dims, 2.0, h_cell)['face'][at2] >= 0).all()
        below = shim(v, f, lo, h, dims, np.nextafter(2.0, 0.0), h_cell)
        assert (below['face'][at2] == -1).all() and (below['sd'][at2] == np.nextafter(2.0, 0.0)).all()


def test_needles_of_aspect_ten_thousand(shim):
    v, f = D.needles()
    lo, h, dims, d_cap = [-420.0, -410.0, -400.0], 75.0, (12, 11, 12), 80.0
    ref = V.volume(v, f, lo, h, dims, d_cap, signed=False)
    assert 50 < ref['in_band'].sum() < ref['in_band'].size - 50
    for h_cell in (30.0, 150.0, 900.0, 5000.0):
        assert check(shim(v, f, lo, h, dims, d_cap, h_cell, signed=False), ref, False, d_cap) == ref['sd'].size


def test_a_mesh_a_million_from_the_origin(shim):
    v, f = icosphere(2, 50.0)
    v = (v + np.float32(1e6)).astype(np.float32)
    lo, h, dims, d_cap = np.float32([1e6 - 66.0] * 3), 12.0, (11, 11, 11), 20.0
    ref = V.volume(v, f, lo, h, dims, d_cap)
    assert ref['mask'].sum() > 100 and (~ref['in_band'] & ref['mask']).sum() > 10 and (~ref['in_band'] & ~ref['mask']).sum() > 10
    for h_cell in (5.0, 21.0, 64.0, 300.0):
        assert check(shim(v, f, lo, h, dims, d_cap, h_cell), ref, True, d_cap) > 1000


def spanning_face():
    """icosphere(2) at R = 10 and one separate face three times as wide as the mesh"""
    v, f = icosphere(2, 10.0)
    big = np.array([[-30.0, -30.0, 14.0], [30.0, -30.0, 14.0], [0.0, 30.0, 14.0]], np.float32)
    return np.concatenate([v, big]).astype(np.float32), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)


def test_one_face_spanning_three_times_the_mesh(shim):
    v, f = spanning_face()
    lo, h, dims, d_cap = [-13.3, -13.1, -12.9], 2.0, (13, 13, 15), 3.0
    ref = V.volume(v, f, lo, h, dims, d_cap, signed=False)
    big = ref['face'] == len(f) - 1
    assert big.sum() > 50 and (ref['face'] >= 0).sum() > big.sum() + 50
    for h_cell in (1.0, 3.0, 9.0, 100.0):
        assert check(shim(v, f, lo, h, dims, d_cap, h_cell, signed=False), ref, False, d_cap) == ref['sd'].size


def test_a_far_node_stops_after_the_rings_the_band_allows(shim):
    """ceil((d_cap + rho_max) / h_cell) + 1 rings with nothing found; a walk without a band would cross the whole grid"""
    v, f = icosphere(3, 50.0)
    lo, h, dims, d_cap, h_cell = [-4.0, -4.0, -4.0], 2.0, (4, 4, 4), 6.0, 5.0                 # nodes near the centre: 44 from the surface
    mine = shim(v, f, lo, h, dims, d_cap, h_cell)
    rho_max = mine['blob'][6]
    assert (mine['face'] == -1).all() and (mine['sd'] == -d_cap).all()
    assert mine['rings'].max() <= int(np.ceil((d_cap + rho_max) / h_cell)) + 1 < 10
    assert mine['centroids'].max() == 0


def test_a_main_of_its_own_under_the_sanitizers(shim, tmp_path):
    cxx = os.environ.get('CXX', 'g++')
    exe = os.path.join(str(tmp_path), 'nwv_main')
    r = subprocess.run([cxx, '-O1', '-g', '-std=c++14', '-ffp-contract=off', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-DNWV_MAIN', '-I', CSRC, '-o', exe, _source(tmp_path)], capture_output=True, text=True)
    if r.returncode != 0 and ('asan' in r.stderr or 'ubsan' in r.stderr or 'sanitize' in r.stderr):
        pytest.skip('the compiler has no sanitizer runtime')
    assert r.returncode == 0, r.stderr
    v, f = V.cube4()
    lo, h, dims = V.CUBE_LATTICE
    mine = shim(v, f, lo, h, dims, 2.0, 1.0)
    v, f, tw, pts, cstart, rho, rho_max, glo, ghi, gdims, lo32, dims32 = mine['blob']
    src, dst = os.path.join(str(tmp_path), 'in.bin'), os.path.join(str(tmp_path), 'out.bin')
    with open(src, 'wb') as fh:
        fh.write(np.array([len(v), len(f), 1, len(pts), len(cstart) - 1] + dims32.tolist(), np.int64).tobytes())
        for a in (v, f, tw, pts, cstart, rho, np.array([rho_max] + glo.tolist() + ghi.tolist() + [1.0, 2.0]), gdims, np.append(lo32, np.float32(h))):
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(dst, 'rb').read()
    n = 729
    assert np.array_equal(np.frombuffer(raw, np.float64, n).view(np.uint64), D.bits(mine['sd']))
    assert np.array_equal(np.frombuffer(raw, np.uint64, n, 8 * n), mine['field'])
    assert np.array_equal(np.frombuffer(raw, np.int32, n, 16 * n), mine['face'])
