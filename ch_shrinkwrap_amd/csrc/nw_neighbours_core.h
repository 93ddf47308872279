// The rules of the k-th-neighbour query (include/nw_neighbours.h), shared by the kernels of nw_neighbours.hip and by whoever compiles
// this header for the CPU (tests/test_neighbours_core_cpu.py builds a shim from it with g++ -ffp-contract=off):
//   - the squared distance, in the header's order of operations;
//   - the list of the k smallest squared distances one query holds, and what the walk may stop at;
//   - the lower bound of a ring of cells;
//   - the quantisation of a node's value into the uint64 field nwi_extract reads.
// Nothing may be contracted into an fma: compile with -ffp-contract=off.  No HIP header is needed: without a HIP compiler NWK_HD is
// plain `inline`.  nw_bq_core.h (HIP-free as well) is included for the cores on top of this one: bq::PtF32, the cloud point in cell order.
#pragma once
#include <cmath>
#include <cstdint>

#include "nw_bq_core.h"

#if defined(__HIPCC__)
#define NWK_HD __host__ __device__ __forceinline__
#else
#define NWK_HD inline
#endif

#define NWK_CORE_MAX_K 32
// Cells are float32 expressions (bq::cell_1d<float>: floorf((x - lo) / h), two roundings of 2^-24 each): a point's cell coordinate is
// off by at most 2 * 2^-24 * 1025 < 2^-12 of a cell on a grid of at most 1025 cells an axis, so two points whose cell indices differ by
// r are at least (r - 1 - 2^-11) cells apart along that axis.  The ring bound gives away 2^-10.
#define NWK_CELL_SLACK (1.0 / 1024.0)

// d^2 between the float32 point p and the float64 position x
NWK_HD double nwk_dist2(float px, float py, float pz, double x, double y, double z)
{
    const double ex = (double)px - x, ey = (double)py - y, ez = (double)pz - z;
    return (ex * ex + ey * ey) + ez * ez;
}

// The k smallest squared distances seen so far, as a multiset: slot j is s[j * stride] (on the device a column of LDS, [slot][lane]).
// Which slot holds which value depends on the order of arrival; the multiset, and with it the k-th smallest, does not.
struct nwk_list {
    int cnt;          // slots in use, at most k
    int at;           // the slot of the largest value
    double mx;        // the largest value held (meaningless while cnt = 0)
};

NWK_HD void nwk_list_init(nwk_list *L) { L->cnt = 0; L->at = 0; L->mx = -1.0; }

// the k-th smallest squared distance so far: +inf until k candidates are held
NWK_HD double nwk_list_kth(const nwk_list *L, int k) { return L->cnt == k ? L->mx : INFINITY; }

NWK_HD void nwk_list_insert(double *s, int stride, int k, nwk_list *L, double d2)
{
    if (L->cnt < k) {                                          // filling: every candidate is kept
        s[L->cnt * stride] = d2;
        if (L->cnt == 0 || d2 > L->mx) { L->mx = d2; L->at = L->cnt; }
        L->cnt += 1;
        return;
    }
    if (!(d2 < L->mx)) return;                                 // (strictly below the largest: an equal value changes nothing)
    s[L->at * stride] = d2;
    double m = s[0];
    int at = 0;
    for (int j = 1; j < k; ++j) {
        const double v = s[j * stride];
        if (v > m) { m = v; at = j; }
    }
    L->mx = m;
    L->at = at;
}

// lower bound of the distance, along one axis, between the projected query and any point in a cell of ring r
NWK_HD double nwk_ring_lbd(int r, double h_cell)
{
    const double cells = (double)(r - 1) - NWK_CELL_SLACK;
    return (cells > 0.0 ? cells : 0.0) * h_cell * (1.0 - 1e-9);
}

// whether the walk ends before ring r: nothing in it or beyond can be among the k nearest or within the cap (strict: ties are all seen)
NWK_HD bool nwk_walk_ends(int r, double h_cell, double out2, const nwk_list *L, int k, double cap2)
{
    const double lbd = nwk_ring_lbd(r, h_cell);
    const double kth = nwk_list_kth(L, k);
    return lbd * lbd + out2 > (kth < cap2 ? kth : cap2);
}

// the result of a query from its k-th smallest squared distance: min(r_k, r_cap)
NWK_HD double nwk_result(double kth2, double r_cap)
{
    const double r = sqrt(kth2);
    return r < r_cap ? r : r_cap;
}

// a node's value in the field: floor((r_cap - r) * 2^20), r = nwk_result(...) <= r_cap <= 2^40
NWK_HD uint64_t nwk_quantise(double r, double r_cap) { return (uint64_t)floor((r_cap - r) * 1048576.0); }

// a node's coordinate along one axis
NWK_HD double nwk_node_coord(float lo, float h, int index) { return (double)lo + ((double)index + 0.5) * (double)h; }
