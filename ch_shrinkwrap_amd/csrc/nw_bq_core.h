// The part of nw_bq.h that needs no HIP: the sizing of a point grid and when to bin anew, the cloud query units' cloud grid (the point in
// cell order, the limits, the cell size), the mesh query units' face grid (a face's centroid and radius, the cell size) and the walk of
// a radix select.  The query units get it through nw_bq.h, nw_distance_core.h and nw_intersections_core.h include it for the centroid
// and nw_neighbours_core.h for the point; tests/test_bq_core_cpu.py compiles it for the CPU with g++.  Without a HIP compiler BQ_HD is
// plain `inline`.
#pragma once
#include <cstdint>
#include <cmath>
#include <algorithm>

#if defined(__HIPCC__)
#define BQ_HD __host__ __device__ __forceinline__
#else
#define BQ_HD inline
#endif

namespace bq {

// ---- sizing of a point grid -------------------------------------------------------------------------------------------------------------
// what differs between the users of the grid: at most min(max(cells_per_point * n, 65536), max_cells) cells (cell ids and the scan are
// int), at most max_dim cells an axis, and how often the cell size may grow by a tenth to get there
struct GridRule {
    int cells_per_point;
    int64_t max_cells;
    int max_dim;
    int widen_steps;
};

inline int64_t grid_cap(const GridRule &rule, int64_t n) { return std::min<int64_t>(std::max<int64_t>(rule.cells_per_point * n, 65536), rule.max_cells); }

// dims[d] = floor(ext[d] / h) + 1 (at most max_dim) with the caller's starting h, widened by a tenth at a time until the cells fit the
// cap of n points -> whether they do
inline bool size_grid(const GridRule &rule, int64_t n, const double ext[3], double *h, int dims[3])
{
    const int64_t cap = grid_cap(rule, n);
    for (int it = 0; it < rule.widen_steps; ++it) {
        int64_t cells = 1;
        for (int d = 0; d < 3; ++d) { dims[d] = (int)std::min<double>((double)rule.max_dim, std::floor(ext[d] / *h) + 1.0); cells *= dims[d]; }
        if (cells <= cap) break;
        *h *= 1.1;
    }
    return (int64_t)dims[0] * dims[1] * dims[2] <= cap;
}

// The sizing half of CloudGrid::bin and FaceGrid::bin (nw_bq.h).  *h_start = the cell size the grid at hand was sized from (0: there is
// none).  A grid sized from the same h0 is kept; else *h_start = 0 and h, dims are sized anew from h0 under `rule`, and the caller sets
// *h_start = h0 once it has binned.
enum Bins { BINS_KEPT = 0, BINS_NEW = 1, BINS_NONE = 2 };      // NONE: no cell size keeps the grid within its cap

inline Bins keep_or_rebin(const GridRule &rule, int64_t n, const double ext[3], double h0, double *h_start, double *h, int dims[3])
{
    if (*h_start == h0) return BINS_KEPT;
    *h_start = 0.0;
    *h = h0;
    return size_grid(rule, n, ext, h, dims) ? BINS_NEW : BINS_NONE;
}

// ---- the cloud grid of the cloud query units (neighbours, clustering, pairs, local shape) -------------------------------------------------
// a cloud point in cell order: its float coordinates and its index in the caller's array (GridOf<float>::point of nw_bq.h)
struct alignas(16) PtF32 {
    float x, y, z;
    int i;
};

// at most max(2 n, 65536) cells, up to 2^26; at most 1025 an axis (NWK_CELL_SLACK rests on it); 400 widening steps
const GridRule CLOUD_GRID_RULE = {2, 1ll << 26, 1025, 400};

// The cell size a cloud grid starts from: the unit's candidate (a fraction of eps, of the largest radius, of the radius), never below a
// 1024th of the widest axis of the cloud's box (emax), so that no cell index is clamped but by its rounding: the walks' proofs need it.
// A cell size that is no positive finite float gives way to the extent, and a cloud without extent gets one cell of side 1.
inline double cloud_cell(double candidate, double emax)
{
    double h = std::max(candidate, emax / 1024.0);
    if (!((float)h > 0.0f) || !std::isfinite((float)h)) h = (emax > 0.0 && std::isfinite((float)emax)) ? emax : 1.0;
    return h;
}

// ---- the face grid of the mesh query units: a face's ball, the cell size, the decision to bin -------------------------------------------
// The centroid of a face in float64, ((a + b) + c) / 3 per axis, and rho = the largest distance from it to a corner (the root of the
// largest of (ex ex + ey ey) + ez ez over the corners, e = corner - centroid, starting from 0): every point of the face lies within rho
// of the centroid.  The one definition: the set-up kernels store it and the walks that compute it again rely on getting the same bits,
// so nothing may be contracted into an fma (-ffp-contract=off).  S = float (vertex positions) or double (positions already widened).
template <class S> BQ_HD double face_centroid(const S *a, const S *b, const S *c, double cen[3])
{
    double rho2 = 0.0;
    for (int d = 0; d < 3; ++d) cen[d] = (((double)a[d] + (double)b[d]) + (double)c[d]) / 3.0;
    const S *v[3] = {a, b, c};
    for (int k = 0; k < 3; ++k) {
        const double ex = (double)v[k][0] - cen[0], ey = (double)v[k][1] - cen[1], ez = (double)v[k][2] - cen[2];
        rho2 = fmax(rho2, (ex * ex + ey * ey) + ez * ez);
    }
    return sqrt(rho2);
}

// the stored rho_f is face_centroid's times 1 + this: far above the rounding of a float64 distance, far below what matters, so that
// rounding can only make a bound weaker
#define BQ_FACE_RHO_SLACK 1e-9

// at most max(16 F, 65536) cells, up to 2^26; at most 1025 an axis; 400 widening steps
const GridRule FACE_GRID_RULE = {16, 1ll << 26, 1025, 400};

// The cell size a face grid starts from: the unit's candidate, at least a 1024th of the widest axis of the centroids' box (emax); 1 for a
// mesh without extent, emax where that is not a positive finite number (an infinite band).  The candidates: 2 m for the fixed grids of
// the distance, intersection and ray units (m = the mean rho_f: a face or two per occupied cell of a surface), band_cell for the volume
// and mapping units, nwm_band_cell (nw_proximity_core.h) for the proximity unit.  m = sum / F, and 2 (sum / F) = (2 sum) / F because
// doubling is exact: only this form is kept.
inline double face_cell(double candidate, double emax)
{
    if (!(emax > 0.0)) return 1.0;
    const double h = std::max(candidate, emax / 1024.0);
    return (h > 0.0 && std::isfinite(h)) ? h : emax;
}

// the candidate of a band d_cap: 2 m or half of d_cap + rho_max, whichever is larger -- a far query then ends its walk after three or
// four rings, a few hundred cell ranges
inline double band_cell(double rho_mean, double rho_max, double d_cap) { return std::max(2.0 * rho_mean, (d_cap + rho_max) / 2.0); }

// FaceGrid::bin's decision: keep_or_rebin under FACE_GRID_RULE
inline Bins face_bins(int64_t nf, const double ext[3], double h0, double *h_start, double *h, int dims[3])
{
    return keep_or_rebin(FACE_GRID_RULE, nf, ext, h0, h_start, h, dims);
}

// ---- radix select over 64-bit keys, a byte per pass from the top ------------------------------------------------------------------------
// the byte of `key` at `shift` if its bits above that byte equal `prefix` (there are none above shift 56), else -1
BQ_HD int radix_bin(uint64_t key, uint64_t prefix, int shift)
{
    const uint64_t above = shift >= 56 ? 0ull : key >> (shift + 8);
    return above == prefix ? (int)((key >> shift) & 255u) : -1;
}

// the bin that holds the element of 0-based rank `rank`, which becomes its rank within that bin; -1 if the histogram holds
// fewer (or the rank is negative)
inline int select_bin(const unsigned hist[256], int64_t &rank)
{
    for (int b = 0; b < 256 && rank >= 0; ++b) {
        if (rank < (int64_t)hist[b]) return b;
        rank -= hist[b];
    }
    return -1;
}

}  // namespace bq
