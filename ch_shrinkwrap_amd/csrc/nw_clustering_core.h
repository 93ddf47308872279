// The definition of the DBSCAN query (include/nw_clustering.h), shared by the kernels of nw_clustering.hip and by whoever compiles this
// header for the CPU (tests/test_clustering_core_cpu.py builds a shim from it with g++ -ffp-contract=off):
//   - what a valid (eps, min_points, count_cap) is;
//   - near(i, j): d2(i, j) <= eps2 on squares, d2 = nwk_dist2 (nw_neighbours_core.h: float64, no fma), eps2 = eps * eps in float64;
//   - the cell size a grid starts from and the guard of the two shortcuts, with its proof;
//   - the ring walk of one point over the grid, ended by nwk_ring_lbd(r, h)^2 > eps2 or by its visitor;
//   - the three visitors: the capped neighbour count, the unions of a core point with the core points near it (those with a smaller
//     index; under shortcut (b) one of them a cell), and the border rule (the core point near it that minimises
//     (d2, index)).
// The squared distance, the ring bound and NWK_CELL_SLACK are nw_neighbours_core.h's: included, not copied.  Nothing may be contracted
// into an fma: compile with -ffp-contract=off.  No HIP header is needed: without a HIP compiler NWK_HD is plain `inline`.
#pragma once
#include "nw_neighbours_core.h"

#define NWP_MAX_N (1ll << 30)
#define NWP_MAX_EPS 1099511627776.0 // 2^40
// The cell size a grid starts from, as a share of eps: the largest round figure under 1 / (sqrt(3) (1 + 2 NWK_CELL_SLACK)) = 0.5762, so
// that a grid that was not widened has both shortcuts.  The walk then ends before ring 3 ((3 - 1 - 2^-10) 0.57 > 1): 125 cells at most.
#define NWP_CELL_OF_EPS 0.57

// a cloud point in cell order: its coordinates and its index in the caller's array (the cloud grid's, nw_bq_core.h)
typedef bq::PtF32 nwp_pt;

// whether the three numbers are a query (a nan fails every comparison)
NWK_HD bool nwp_args_ok(double eps, long long min_points, long long count_cap)
{
    return eps > 0.0 && eps <= NWP_MAX_EPS && min_points >= 1 && min_points <= NWP_MAX_N && count_cap >= min_points && count_cap <= NWP_MAX_N;
}

// near(i, j), p = point j, (x, y, z) = (double) point i.  (ex * ex + ey * ey) + ez * ez is the same number for (i, j) and (j, i): the
// differences are each other's negations, exactly.
NWK_HD bool nwp_near(const nwp_pt &p, double x, double y, double z, double eps2) { return nwk_dist2(p.x, p.y, p.z, x, y, z) <= eps2; }

// The guard of the shortcuts: whether any two points of one cell are near whatever their coordinates are.
// Proof.  A point's cell index along an axis is the float32 expression floorf((x - lo) / h), clamped to the grid; by
// nw_neighbours_core.h's bound it is the floor of a cell coordinate that is off by less than 2^-12 of a cell from the exact
// (x - lo) / h.  The grid is sized so that only that rounding can push an index past the last cell (the starting cell size is at least
// 1/1024 of the widest extent: nothing else is clamped).  Two points with the same index therefore differ by less than
// (1 + 2 * 2^-12 + 2^-12) h < (1 + 2 NWK_CELL_SLACK) h along every axis, and their exact distance is below sqrt(3) (1 + 2 NWK_CELL_SLACK) h.
// If that is below eps / (1 + 1e-9), the float64 d2 (three roundings of 2^-53 each) is below the float64 eps2 (one rounding).
// A grid that was widened past this bound has no shortcut: the exact walk does everything.
NWK_HD bool nwp_shortcuts_ok(double h_cell, double eps)
{
    return 1.7320508075688774 * h_cell * (1.0 + 2.0 * NWK_CELL_SLACK) * (1.0 + 1e-9) < eps;
}

// what a visitor answers: go on, end the walk, or leave the rest of the cell at hand
#define NWP_GO 0
#define NWP_STOP 1
#define NWP_NEXT_CELL 2

// The walk of the point in cell (cx, cy, cz) over rings r_first, r_first + 1, ... of cells around its own: visit(q, pts[q]) for every point
// of every cell of a ring, until visit answers NWP_STOP or the ring's lower bound says that nothing further out is near.  Ring 0 is the
// point's own cell.  -> the rings walked.
template <class Visit>
NWK_HD int nwp_walk(const nwp_pt *pts, const int *cstart, const int *dims, double h, int cx, int cy, int cz, double eps2, int r_first, Visit &visit)
{
    const int rx = cx > dims[0] - 1 - cx ? cx : dims[0] - 1 - cx, ry = cy > dims[1] - 1 - cy ? cy : dims[1] - 1 - cy,
              rz = cz > dims[2] - 1 - cz ? cz : dims[2] - 1 - cz;
    const int rmax = rx > ry ? (rx > rz ? rx : rz) : (ry > rz ? ry : rz);
    int rings = 0;
    for (int r = r_first; r <= rmax; ++r) {
        const double lbd = nwk_ring_lbd(r, h);
        if (lbd * lbd > eps2) break;
        ++rings;
        const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < dims[2] - 1 ? cz + r : dims[2] - 1;
        const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < dims[1] - 1 ? cy + r : dims[1] - 1;
        const int xa = cx - r > 0 ? cx - r : 0, xb = cx + r < dims[0] - 1 ? cx + r : dims[0] - 1;
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const long long row = ((long long)z * dims[1] + y) * dims[0];
                const bool shell = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
                // a row of the ring's shell, or the two cells where the ring crosses the row
                for (int part = 0; part < (shell ? 1 : 2); ++part) {
                    int c0, c1;
                    if (shell) { c0 = xa; c1 = xb; }
                    else if (part == 0) { if (cx - r < 0) continue; c0 = c1 = cx - r; }
                    else { if (cx + r >= dims[0]) continue; c0 = c1 = cx + r; }
                    int b = cstart[row + c0];
                    for (int c = c0; c <= c1; ++c) {
                        const int e = cstart[row + c + 1];
                        for (int q = b; q < e; ++q) {
                            const int what = visit(q, pts[q]);
                            if (what == NWP_STOP) return rings;
                            if (what == NWP_NEXT_CELL) break;
                        }
                        b = e;
                    }
                }
            }
        }
    }
    return rings;
}

// n_eps up to the cap: the walk ends once cnt has reached it
struct nwp_count_visit {
    double x, y, z, eps2;
    int cnt, cap;
    long long tests;
    NWK_HD int operator()(int, const nwp_pt &p)
    {
        ++tests;
        cnt += nwp_near(p, x, y, z, eps2) ? 1 : 0;
        return cnt >= cap ? NWP_STOP : NWP_GO;
    }
};

// the unions of core point i: with every core point near it that has a smaller index (each edge once, from its larger end).  With the
// shortcuts (by_cell; the walk then starts at ring 1) shortcut (b) has made every cell's core points one component already, so one near
// pair joins two cells for good: after the first union with a point of a cell the rest of that cell is left.  Every edge (i, j), j < i,
// is still covered: i's lane either meets j or has joined j's cell through another of its core points.  U::unite is the device's lock-free hook or the CPU shim's sequential one.  is_core is in cell order, as pts.
template <class U> struct nwp_hook_visit {
    double x, y, z, eps2;
    int i;
    bool by_cell;
    const unsigned char *is_core;
    U *u;
    long long tests;
    NWK_HD int operator()(int q, const nwp_pt &p)
    {
        if (p.i >= i || !is_core[q]) return NWP_GO;
        ++tests;
        if (!nwp_near(p, x, y, z, eps2)) return NWP_GO;
        u->unite(i, p.i);
        return by_cell ? NWP_NEXT_CELL : NWP_GO;
    }
};

// the border rule: the core point near i that minimises (d2, index); best_i = -1 while there is none
struct nwp_border_visit {
    double x, y, z, eps2;
    const unsigned char *is_core;
    double best_d2;
    int best_i;
    long long tests;
    NWK_HD int operator()(int q, const nwp_pt &p)
    {
        if (!is_core[q]) return NWP_GO;
        ++tests;
        const double d2 = nwk_dist2(p.x, p.y, p.z, x, y, z);
        if (d2 <= eps2 && (best_i < 0 || d2 < best_d2 || (d2 == best_d2 && p.i < best_i))) { best_d2 = d2; best_i = p.i; }
        return NWP_GO;
    }
};
