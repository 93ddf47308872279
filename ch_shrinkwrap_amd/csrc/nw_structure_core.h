// The definition of the local-shape query (include/nw_structure.h), shared by the kernels of nw_structure.hip and by whoever compiles this
// header for the CPU (tests/test_structure_core_cpu.py builds a shim from it with g++ -ffp-contract=off):
//   - what a valid radius is, the neighbourhood N(q) = { j : d2(p_j, q) <= r * r }, inclusive;
//   - the quantisation of a neighbour's offset from the query into an integer of at most 19 bits and a sign, with its proof;
//   - the ten integer moments of a neighbourhood and why none can overflow;
//   - the covariance, the cyclic Jacobi iteration, the order and the signs of the eigenvectors, the flags: one fixed float64 procedure;
//   - the cell size a grid starts from;
//   - the walk of one query over the cloud's cell grid: a clamped box of cells, cells skipped by their distance, with its proof.
// The squared distance and NWK_CELL_SLACK are nw_neighbours_core.h's: included, not copied.  PYME is not in the reference tree and upstream
// has no such module: the definition is this project's own, and this file is where it is written down.
// Nothing may be contracted into a fused multiply-add: compile with -ffp-contract=off.  No HIP header is needed: without a HIP compiler
// NWK_HD is plain `inline`.
#pragma once
#include "nw_neighbours_core.h"

#define NWF_MAX_N (1ll << 26)
#define NWF_MAX_R 1099511627776.0   // 2^40
#define NWF_Q_BITS 18
#define NWF_Q_ONE 262144.0          // 2^18
// Sweeps of the cyclic Jacobi iteration, a constant: no convergence test, so every query runs the same instructions.  Seen on the
// restatement (tests/local_shape_ref.py, 12 505 neighbourhoods of noisy shells, sheets, tubules, blobs, lattices, a plane and a line): the
// largest off-diagonal element relative to the largest diagonal one was 0.31 after 1 sweep, 4.4e-2 after 2, 4.3e-6 after 3, 7.3e-23
// after 4, 5.9e-94 after 5 and exactly 0 after 6.  Four are already far below an ulp (1.1e-16); five leave one sweep in hand.  A rotation
// whose a_pq is exactly 0 is skipped, so a sweep over a diagonal matrix changes nothing.
#define NWF_SWEEPS 5
// The cell size a grid starts from, as a share of the radius.  A first choice that nobody has measured: taken over from the pair counts'
// starting cell, whose walk this one repeats.  A smaller cell hugs the ball more closely and reads more cells, a larger one reads fewer
// cells and tests more points that are too far.
#define NWF_CELL_OF_R 0.5

// flags[q]: which case applied
#define NWF_FLAG_VALID 1            // n >= 3 and lambda_0 > 0
#define NWF_FLAG_EMPTY 2            // n = 0: eigenvalues NaN, vectors zero
#define NWF_FLAG_FEW 4              // 1 <= n < 3
#define NWF_FLAG_POINT 8            // n >= 3 and lambda_0 <= 0: all neighbours in one place (as far as the quantisation sees)
#define NWF_FLAG_TURNED 16          // the viewpoint turned the normal against the largest-component rule

// a cloud point in cell order: its coordinates and its index in the caller's array (the cloud grid's, nw_bq_core.h)
typedef bq::PtF32 nwf_pt;

// Whether r is a radius: finite, 0 < r <= 2^40, and *r2 = r * r (float64, computed here once) finite and above 0.  A nan fails the first
// comparison.
NWK_HD bool nwf_radius(double r, double *r2)
{
    if (!(r > 0.0 && r <= NWF_MAX_R)) return false;
    *r2 = r * r;
    return *r2 > 0.0 && *r2 <= NWF_MAX_R * NWF_MAX_R;
}

// R = the smallest power of two >= r, r a radius as above (so a normal double: r * r > 0).  frexp gives r = f * 2^e with 1/2 <= f < 1.
NWK_HD double nwf_pow2_above(double r)
{
    int e = 0;
    const double f = frexp(r, &e);
    return f == 0.5 ? r : ldexp(1.0, e);
}

// The scale of the quantisation, s = 2^18 / R, and the size of one step, 1 / s = R / 2^18: both powers of two, both exact.
NWK_HD void nwf_scale(double r, double *s, double *step)
{
    const double R = nwf_pow2_above(r);
    *s = NWF_Q_ONE / R;
    *step = R / NWF_Q_ONE;
}

// u = rint(e * s) for one axis of a neighbour, e = (double)p - q exactly as nwk_dist2 forms it (one rounding).  s is a power of two, so the
// product is exact (it cannot overflow, and where it is so small that it loses bits it rounds to 0 all the same); rint rounds to the nearest
// integer, ties to even, in the default rounding mode.
// Proof that a neighbour's |u| <= 2^18.  d2 = fl(fl(fl(ex^2) + fl(ey^2)) + fl(ez^2)) <= r2 and every rounding is within 2^-53 relative,
// so ex^2 <= ex^2 + ey^2 + ez^2 <= r2 (1 + 2^-53)^3 < r2 (1 + 2^-51): the roundings of d2 give away at most that factor.
// r2 = fl(r * r) <= r^2 (1 + 2^-53), so |ex| < r (1 + 2^-51) <= R (1 + 2^-51) and |ex * s| < 2^18 + 2^-33, whose nearest integer is at
// most 2^18 in magnitude.  u fits an int with 12 bits to spare.
NWK_HD int nwf_quantise(double e, double s) { return (int)rint(e * s); }

// The ten moments of one neighbourhood.  |u_a u_b| <= 2^36; with at most NWF_MAX_N = 2^26 cloud points |S2| <= 2^62 and |S1| <= 2^44: no
// sum can overflow an int64, whatever the order of the terms (nwf_set_cloud refuses more points).  Integer sums depend neither on the
// order of the cloud, nor on the cell size, nor on the launch.
#define NWF_MOMENTS 10
struct nwf_sums {
    long long n;
    long long sx, sy, sz;                                     // S1 = sum u
    long long xx, xy, xz, yy, yz, zz;                         // S2 = sum u_a u_b
};

NWK_HD void nwf_sums_init(nwf_sums *m) { m->n = m->sx = m->sy = m->sz = m->xx = m->xy = m->xz = m->yy = m->yz = m->zz = 0; }

// One cloud point against the query (x, y, z): the inclusive test, and the neighbour's terms.  The products are of int operands widened
// once: a 32 x 32 -> 64 multiply-add each, not a 64-bit multiply.
NWK_HD void nwf_visit(nwf_sums *m, float px, float py, float pz, double x, double y, double z, double r2, double s)
{
    if (!(nwk_dist2(px, py, pz, x, y, z) <= r2)) return;
    const int ux = nwf_quantise((double)px - x, s), uy = nwf_quantise((double)py - y, s), uz = nwf_quantise((double)pz - z, s);
    m->n += 1;
    m->sx += ux; m->sy += uy; m->sz += uz;
    m->xx += (long long)ux * ux; m->xy += (long long)ux * uy; m->xz += (long long)ux * uz;
    m->yy += (long long)uy * uy; m->yz += (long long)uy * uz; m->zz += (long long)uz * uz;
}

// ---- covariance and eigenvectors: one fixed float64 procedure ------------------------------------------------------------------------

// One Jacobi rotation in the plane (p, q) of the symmetric matrix A and of the vectors V (columns): a_pq becomes 0.  `arp`, `arq` are the
// two elements that couple the third index r to p and q; v?p, v?q are columns p and q of V.  Skipped when a_pq == 0.
//   theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) (sgn(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c
// (a theta so large that its square overflows gives t = 0, c = 1, s = 0: nothing is a nan).  Then, element by element and in this order,
//   a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq),
//   (v_kp, v_kq) = (c v_kp - s v_kq, s v_kp + c v_kq) for k = 0, 1, 2.
NWK_HD void nwf_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p, double &v0q, double &v1p, double &v1q, double &v2p,
                       double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double sgn = theta >= 0.0 ? 1.0 : -1.0;
    const double t = sgn / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double tapq = t * apq;
    app = app - tapq;
    aqq = aqq + tapq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    const double p0 = c * v0p - s * v0q, q0 = s * v0p + c * v0q;
    v0p = p0; v0q = q0;
    const double p1 = c * v1p - s * v1q, q1 = s * v1p + c * v1q;
    v1p = p1; v1q = q1;
    const double p2 = c * v2p - s * v2q, q2 = s * v2p + c * v2q;
    v2p = p2; v2q = q2;
}

// swaps (lambda, vector) a and b if lambda_b > lambda_a: strictly, so equal eigenvalues keep their positions
NWK_HD void nwf_order(double &la, double &lb, double &a0, double &a1, double &a2, double &b0, double &b1, double &b2)
{
    if (!(lb > la)) return;
    double w;
    w = la; la = lb; lb = w;
    w = a0; a0 = b0; b0 = w;
    w = a1; a1 = b1; b1 = w;
    w = a2; a2 = b2; b2 = w;
}

// flips a vector so that its component of largest magnitude is positive; on a tie the first such component counts
NWK_HD void nwf_sign(double &v0, double &v1, double &v2)
{
    double big = v0;
    if (fabs(v1) > fabs(big)) big = v1;
    if (fabs(v2) > fabs(big)) big = v2;
    if (big < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
}

// From the ten moments of a neighbourhood to its shape.
//   m_a = (double)S1_a / n,  C_ab = (double)S2_ab / n - m_a m_b                 (every conversion, quotient and product rounded once)
// The coordinates are relative to the query, so |u| <= 2^18 and the cancellation in C costs a few ulp of 2^36 -- not of the cloud's squared
// distance from the origin, which at 10^6 nm would leave no digits at all.  C is in units of step^2 = (R / 2^18)^2.
// Then NWF_SWEEPS sweeps of rotations in the order (0,1), (0,2), (1,2), V starting as the identity; the eigenvalues are the diagonal, the
// eigenvectors the columns of V.  They are put in descending order by three exchanges (0,1), (1,2), (0,1), each strict: on a tie the
// earlier position stays in front.  The eigenvalues are then scaled, (lambda * step) * step, a power of two each time, and reported as
// computed: the small ones of a flat or thin neighbourhood may be a few ulp below zero.
// vec[0..3) = the axis (of lambda_0), vec[3..6) = mid, vec[6..9) = the normal (of lambda_2), each by nwf_sign's rule.  With a viewpoint,
// w = viewpoint - query in float64, the normal is then turned if (n_0 w_0 + n_1 w_1) + n_2 w_2 < 0, so that it faces the viewpoint.
// n = 0: eigenvalues NaN, vectors zero.  Otherwise whatever the procedure gives (n = 1: C = 0 exactly, eigenvalues 0, V the identity).
// Returns the flags.
NWK_HD unsigned char nwf_shape(const nwf_sums &m, double step, bool has_view, double wx, double wy, double wz, double *lam, double *vec)
{
    if (m.n == 0) {
        lam[0] = lam[1] = lam[2] = (double)NAN;
        vec[0] = vec[1] = vec[2] = vec[3] = vec[4] = vec[5] = vec[6] = vec[7] = vec[8] = 0.0;
        return NWF_FLAG_EMPTY;
    }
    const double dn = (double)m.n;
    const double mx = (double)m.sx / dn, my = (double)m.sy / dn, mz = (double)m.sz / dn;
    double a00 = (double)m.xx / dn - mx * mx, a01 = (double)m.xy / dn - mx * my, a02 = (double)m.xz / dn - mx * mz;
    double a11 = (double)m.yy / dn - my * my, a12 = (double)m.yz / dn - my * mz, a22 = (double)m.zz / dn - mz * mz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;     // v[row][column]
    for (int sweep = 0; sweep < NWF_SWEEPS; ++sweep) {
        nwf_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);        // (0,1); the third index is 2
        nwf_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);        // (0,2); the third index is 1
        nwf_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);        // (1,2); the third index is 0
    }
    double l0 = a00, l1 = a11, l2 = a22;
    nwf_order(l0, l1, v00, v10, v20, v01, v11, v21);
    nwf_order(l1, l2, v01, v11, v21, v02, v12, v22);
    nwf_order(l0, l1, v00, v10, v20, v01, v11, v21);
    l0 = (l0 * step) * step; l1 = (l1 * step) * step; l2 = (l2 * step) * step;
    nwf_sign(v00, v10, v20);
    nwf_sign(v01, v11, v21);
    nwf_sign(v02, v12, v22);
    unsigned char flag = 0;
    if (has_view && (v02 * wx + v12 * wy) + v22 * wz < 0.0) {
        v02 = -v02; v12 = -v12; v22 = -v22;
        flag |= NWF_FLAG_TURNED;
    }
    lam[0] = l0; lam[1] = l1; lam[2] = l2;
    vec[0] = v00; vec[1] = v10; vec[2] = v20;
    vec[3] = v01; vec[4] = v11; vec[5] = v21;
    vec[6] = v02; vec[7] = v12; vec[8] = v22;
    if (m.n < 3) flag |= NWF_FLAG_FEW;
    else if (l0 > 0.0) flag |= NWF_FLAG_VALID;
    else flag |= NWF_FLAG_POINT;
    return flag;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------

// The cells along one axis that can hold a cloud point within r of the query coordinate q: [*c0, *c1], never empty.
// Proof.  Let x be the coordinate of a cloud point with |x - q| <= r (in exact arithmetic; otherwise the point is further than r from
// the query and is no neighbour).  Rounding is monotone and x is a double, so fl(q - r) <= x, fl(fl(q - r) - lo) <= fl(x - lo) and
// a = fl(fl(fl(q - r) - lo) / h) <= fl(fl(x - lo) / h) = t64, the point's cell coordinate in float64 arithmetic.  The point's cell index
// is the float32 expression floorf((x - lo) / h) clamped to [0, dim - 1]; by nw_neighbours_core.h's bound its cell coordinate is off by
// less than 2^-12 of a cell from the exact one on a grid of at most 1025 cells an axis, and t64 by far less, so the index is at least
// floor(a - NWK_CELL_SLACK) clamped, which is *c0; the same with the signs turned gives *c1.  The clamp is the cloud's own clamp and
// monotone as well: a query far outside the box walks the slab of cells at the box's face.  Nothing can overflow: |q| is a float, r is at
// most 2^40, the quotient is clamped as a double before it becomes an int.
NWK_HD void nwf_axis_cells(double q, double r, double lo, double h, int dim, int *c0, int *c1)
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
NWK_HD double nwf_axis_gap(double q, double lo, double hi, double h, int dim, int c)
{
    const double left = c == 0 ? lo : lo + h * ((double)c - NWK_CELL_SLACK);
    const double right = c == dim - 1 ? hi : lo + h * ((double)(c + 1) + NWK_CELL_SLACK);
    const double g = q < left ? left - q : (q > right ? q - right : 0.0);
    return g * (1.0 - 1e-9);
}

// The grid as the walk needs it: the box's corners and the cell size as doubles (exactly the floats the cloud was binned with)
struct nwf_grid {
    double lo[3], hi[3];
    double h;
    int dims[3];
};

// The walk of one query (x, y, z): visit(pts[p]) for every cloud point of every cell that can hold a point within r of the query,
// r2 = r * r.  The cells are the box of nwf_axis_cells' three ranges -- the query may lie anywhere, inside the grid or far outside it: the
// box is clamped, no ring and no out-of-box term is used -- minus the cells whose gaps put every one of their points beyond r: whole rows
// (y, z) by gy^2 + gz^2, then cells from both ends of a row by gx^2 + gy^2 + gz^2.  Such a sum, rounded down by the factor, is a lower
// bound of the exact squared distance to any point of the cell, and the float64 d2 (three roundings of 2^-53) of such a point is above
// r2: it is no neighbour.  What is left of a row is adjacent in cell order, so it is one run of points.  *cells = the cells read.
// Which points are visited depends on the cell size; which of them are neighbours does not.
template <class Visit>
NWK_HD void nwf_walk(const nwf_pt *pts, const int *cstart, const nwf_grid &g, double x, double y, double z, double r, double r2, Visit &visit,
                     int *cells)
{
    int x0, x1, y0, y1, z0, z1;
    nwf_axis_cells(x, r, g.lo[0], g.h, g.dims[0], &x0, &x1);
    nwf_axis_cells(y, r, g.lo[1], g.h, g.dims[1], &y0, &y1);
    nwf_axis_cells(z, r, g.lo[2], g.h, g.dims[2], &z0, &z1);
    int read = 0;                                             // (at most 2^26 cells)
    for (int cz = z0; cz <= z1; ++cz) {
        const double gz = nwf_axis_gap(z, g.lo[2], g.hi[2], g.h, g.dims[2], cz);
        for (int cy = y0; cy <= y1; ++cy) {
            const double gy = nwf_axis_gap(y, g.lo[1], g.hi[1], g.h, g.dims[1], cy);
            const double gyz = gy * gy + gz * gz;
            if (gyz * (1.0 - 1e-9) > r2) continue;
            int a = x0, b = x1;
            while (a <= b) {
                const double gx = nwf_axis_gap(x, g.lo[0], g.hi[0], g.h, g.dims[0], a);
                if (!((gx * gx + gyz) * (1.0 - 1e-9) > r2)) break;
                ++a;
            }
            while (b > a) {
                const double gx = nwf_axis_gap(x, g.lo[0], g.hi[0], g.h, g.dims[0], b);
                if (!((gx * gx + gyz) * (1.0 - 1e-9) > r2)) break;
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
