// The part of nw_bq.h that needs no HIP: the sizing of a point grid and the walk of a radix select.  The query units get it through
// nw_bq.h; tests/test_bq_core_cpu.py compiles it for the CPU with g++.  Without a HIP compiler BQ_HD is plain `inline`.
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
