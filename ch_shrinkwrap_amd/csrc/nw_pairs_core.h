// The definition of the pair-count query (include/nw_pairs.h), shared by the kernels of nw_pairs.hip and by whoever compiles this header
// for the CPU (tests/test_pairs_core_cpu.py builds a shim from it with g++ -ffp-contract=off):
//   - what a valid list of radii is, and the squared edges e2[b] = r_b * r_b in float64;
//   - bin(d2) = #{ b : e2[b] < d2 }, as the literal sum and as a search; a pair at exactly an edge belongs to the bin the edge closes;
//   - the cell size a grid starts from;
//   - the walk of one query over the cloud's cell grid: a clamped box of cells, cells skipped by their distance, with its proof.
// The squared distance and NWK_CELL_SLACK are nw_neighbours_core.h's: included, not copied.  Squares are compared: no root is taken
// anywhere.  Nothing may be contracted into an fma: compile with -ffp-contract=off.  No HIP header is needed: without a HIP compiler
// NWK_HD is plain `inline`.
#pragma once
#include "nw_neighbours_core.h"

#define NWQ_MAX_N (1ll << 30)
#define NWQ_MAX_R 1099511627776.0   // 2^40
#define NWQ_MAX_BINS 64
#define NWQ_NARROW_BINS 16          // up to here the bin is the literal sum against uniform operands; above it, a search
// The cell size a grid starts from, as a share of the largest radius.  A first choice that nobody has measured on more than one cloud:
// profiles/pairs.txt sweeps it on config C3, where 0.25 is a few per cent faster with eight times the cells.  A smaller cell hugs the
// ball more closely and reads more cells, a larger one reads fewer cells and tests more points that are too far.
#define NWQ_CELL_OF_RMAX 0.5

// a cloud point in cell order: its coordinates and its index in the caller's array (the cloud grid's, nw_bq_core.h)
typedef bq::PtF32 nwq_pt;

// d2 of a pair, p = the cloud point, (x, y, z) = (double) query.  (ex * ex + ey * ey) + ez * ez is the same number with the two points
// swapped: the differences are each other's negations, exactly.  In auto mode (i, j) and (j, i) therefore fall into the same bin.
NWK_HD double nwq_dist2(const nwq_pt &p, double x, double y, double z) { return nwk_dist2(p.x, p.y, p.z, x, y, z); }

// Whether radii[0 .. m) are edges: 1 <= m <= NWQ_MAX_BINS, finite, 0 <= r_0 < r_1 < ... <= 2^40, and their squares still strictly
// ascending (two radii that square to one double are refused; a nan fails every comparison).  e2[0 .. m) = the squares, and
// e2[m .. NWQ_MAX_BINS) = +inf: no d2 is above those, so a sum or a search over a padded list is the sum over the m edges.
NWK_HD bool nwq_edges(const double *radii, long long m, double *e2)
{
    if (!radii || m < 1 || m > NWQ_MAX_BINS) return false;
    for (int b = 0; b < NWQ_MAX_BINS; ++b) e2[b] = INFINITY;
    for (int b = 0; b < (int)m; ++b) {
        const double r = radii[b];
        if (!(r >= 0.0 && r <= NWQ_MAX_R)) return false;
        e2[b] = r * r;
        if (b > 0 && !(e2[b] > e2[b - 1])) return false;
    }
    return true;
}

// bin(d2), the definition: how many of the first `width` entries of the padded list lie strictly below d2
NWK_HD int nwq_bin_sum(const double *e2, int width, double d2)
{
    int bin = 0;
    for (int b = 0; b < width; ++b) bin += e2[b] < d2 ? 1 : 0;
    return bin;
}

// the same number by a search over all NWQ_MAX_BINS entries of the padded list (ascending, the padding at the end): after the loop
// `bin` counts the entries below d2 among the first 63, and the last comparison is false unless all 63 are
NWK_HD int nwq_bin_search(const double *e2, double d2)
{
    int bin = 0;
    for (int step = NWQ_MAX_BINS / 2; step > 0; step >>= 1) bin += e2[bin + step - 1] < d2 ? step : 0;
    return bin + (e2[bin] < d2 ? 1 : 0);
}

// The cells along one axis that can hold a cloud point within r of the query coordinate q: [*c0, *c1], never empty.
// Proof.  Let x be the coordinate of a cloud point with |x - q| <= r (in exact arithmetic; otherwise the point is further than r from
// the query and lies in no bin).  Rounding is monotone and x is a double, so fl(q - r) <= x, fl(fl(q - r) - lo) <= fl(x - lo) and
// a = fl(fl(fl(q - r) - lo) / h) <= fl(fl(x - lo) / h) = t64, the point's cell coordinate in float64 arithmetic.  The point's cell index
// is the float32 expression floorf((x - lo) / h) clamped to [0, dim - 1]; by nw_neighbours_core.h's bound its cell coordinate is off by
// less than 2^-12 of a cell from the exact one on a grid of at most 1025 cells an axis, and t64 by far less, so the index is at least
// floor(a - NWK_CELL_SLACK) clamped, which is *c0; the same with the signs turned gives *c1.  The clamp is the cloud's own clamp and
// monotone as well: a query far outside the box walks the slab of cells at the box's face.  Nothing can overflow: |q| is a float, r is at
// most 2^40, the quotient is clamped as a double before it becomes an int.
NWK_HD void nwq_axis_cells(double q, double r, double lo, double h, int dim, int *c0, int *c1)
{
    const double top = (double)(dim - 1);
    double a = floor(((q - r) - lo) / h - NWK_CELL_SLACK), b = floor(((q + r) - lo) / h + NWK_CELL_SLACK);
    a = a > 0.0 ? a : 0.0;
    b = b > 0.0 ? b : 0.0;
    *c0 = (int)(a < top ? a : top);
    *c1 = (int)(b < top ? b : top);
}

// A lower bound of |x - q| over the cloud points x of cell c along one axis (0 if q may lie among them).
// Proof.  Every cloud point lies in [lo, hi], the box's own float corners, exactly.  A point of cell c > 0 has a float32 cell coordinate
// of at least c, so an exact one above c - 2^-12, so x > lo + h (c - 2^-12); a point of cell c < dim - 1 likewise has
// x < lo + h (c + 1 + 2^-12).  The two expressions below give away NWK_CELL_SLACK instead, 3/4 of which (0.7e-3 h) is left for their own
// two roundings: those are below 2^-52 of the largest coordinate M on the axis, and on an axis with any extent at all the grid's cell is
// at least 1/1024 of that extent (the starting cell size sees to it), which is at least 2^-24 M: 2^-52 M <= 2^-18 h.  The last factor
// pays for the rounding of the difference.
NWK_HD double nwq_axis_gap(double q, double lo, double hi, double h, int dim, int c)
{
    const double left = c == 0 ? lo : lo + h * ((double)c - NWK_CELL_SLACK);
    const double right = c == dim - 1 ? hi : lo + h * ((double)(c + 1) + NWK_CELL_SLACK);
    const double g = q < left ? left - q : (q > right ? q - right : 0.0);
    return g * (1.0 - 1e-9);
}

// The grid as the walk needs it: the box's corners and the cell size as doubles (exactly the floats the cloud was binned with)
struct nwq_grid {
    double lo[3], hi[3];
    double h;
    int dims[3];
};

// The walk of one query (x, y, z): visit(pts[p]) for every cloud point of every cell that can hold a point within r_max of the query,
// r_max2 = r_max * r_max being the last edge.  The cells are the box of nwq_axis_cells' three ranges -- the query may lie anywhere, inside
// the grid or far outside it: the box is clamped, no ring and no out-of-box term is used -- minus the cells whose gaps put every one of
// their points beyond r_max: whole rows (y, z) by gy^2 + gz^2, then cells from both ends of a row by gx^2 + gy^2 + gz^2.  Such a sum,
// rounded down by the factor, is a lower bound of the exact squared distance to any point of the cell, and the float64 d2 (three
// roundings of 2^-53) of such a point is above r_max2: it lies in no bin.  What is left of a row is adjacent in cell order, so it is one
// run of points.  *cells = the cells read.  Which points are visited depends on the cell size; which of them are counted does not.
template <class Visit>
NWK_HD void nwq_walk(const nwq_pt *pts, const int *cstart, const nwq_grid &g, double x, double y, double z, double r_max, double r_max2, Visit &visit,
                     long long *cells)
{
    int x0, x1, y0, y1, z0, z1;
    nwq_axis_cells(x, r_max, g.lo[0], g.h, g.dims[0], &x0, &x1);
    nwq_axis_cells(y, r_max, g.lo[1], g.h, g.dims[1], &y0, &y1);
    nwq_axis_cells(z, r_max, g.lo[2], g.h, g.dims[2], &z0, &z1);
    long long read = 0;
    for (int cz = z0; cz <= z1; ++cz) {
        const double gz = nwq_axis_gap(z, g.lo[2], g.hi[2], g.h, g.dims[2], cz);
        for (int cy = y0; cy <= y1; ++cy) {
            const double gy = nwq_axis_gap(y, g.lo[1], g.hi[1], g.h, g.dims[1], cy);
            const double gyz = gy * gy + gz * gz;
            if (gyz * (1.0 - 1e-9) > r_max2) continue;
            int a = x0, b = x1;
            while (a <= b) {
                const double gx = nwq_axis_gap(x, g.lo[0], g.hi[0], g.h, g.dims[0], a);
                if (!((gx * gx + gyz) * (1.0 - 1e-9) > r_max2)) break;
                ++a;
            }
            while (b > a) {
                const double gx = nwq_axis_gap(x, g.lo[0], g.hi[0], g.h, g.dims[0], b);
                if (!((gx * gx + gyz) * (1.0 - 1e-9) > r_max2)) break;
                --b;
            }
            if (a > b) continue;
            const long long row = ((long long)cz * g.dims[1] + cy) * g.dims[0];
            const int first = cstart[row + a], end = cstart[row + b + 1];
            read += b - a + 1;
            for (int p = first; p < end; ++p) visit(pts[p]);
        }
    }
    *cells = read;
}
