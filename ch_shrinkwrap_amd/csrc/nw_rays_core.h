// The arithmetic of ray casting against a triangle mesh (include/nw_rays.h: nwc_cast), shared by the kernels of nw_rays.hip and by
// whoever compiles this header for the CPU (tests/test_rays_core_cpu.py builds a shim from it with g++ -ffp-contract=off).
// tests/mesh_rays_ref.py restates the definition in NumPy, operation for operation, over all faces with no grid.
//
// Everything is float64 on the float32 vertex positions widened to double, in nw_intersections_core.h's order of operations (its
// nwx_v3, nwx_sub / dot / cross / load / normal / face_centroid are used, not copied); nothing may be contracted into an fma: compile
// with -ffp-contract=off.
//
// A ray is an origin o, a direction d of any finite length and two optional ids, skip_vertex and skip_face (-1 for none).  L = sqrt(d.d); a
// ray with !(L > 0) hits nothing (the zero vector, and any d so short that d.d is zero in float64: below about 1e-162).  The ray HITS face f (corners a, b, c; n = (b - a) x (c - a); centroid c_f and rho_f from
// nwx_face_centroid, rho_f enlarged by 1 + NWC_RHO_SLACK) iff all of these hold:
//   - the face is not flat: n.n > 0;
//   - the face is not skipped: none of its three vertex IDS is skip_vertex and f != skip_face (positions are never compared);
//   - the edge test passes, inclusively: with ea = a - o, eb = b - o, ec = c - o and w0 = (ea x eb).d, w1 = (eb x ec).d,
//     w2 = (ec x ea).d, all three are >= 0 or all three are <= 0, and not all three are zero.  The cross and dot products are exactly
//     antisymmetric in float arithmetic: the two faces of a shared edge see w and -w, so with the inclusive rule no ray leaks through
//     an edge or a vertex of a closed mesh (with a strict rule it does: rays through opposite vertices of a lattice cube miss);
//   - the parameter is in range: den = n.d != 0, t = (n.ea) / den, t > 0 and t <= t_max;
//   - the hit point lies in the face's ball: x = o + t d per axis, |x - c_f|^2 <= rho_f^2.  In exact arithmetic this is implied; in
//     rounded arithmetic a grazing ray's t can put x anywhere, and it is this clause that lets a search by centroids be exact.
// Per ray: t of the nearest hit (+inf if none), its face (equal t goes to the smallest face id; -1 if none), an info word whose bit 0
// is den > 0 at that hit (the ray leaves through the face's back: what an inward ray inside an outward-oriented surface does), and on
// request the NUMBER OF FACES HIT.  A ray that meets an edge or a vertex in rounded arithmetic (some w == 0) counts every face of the
// fan, so the count is a function of the input, compared exactly -- and the number of crossings of the surface only off such rays.
//
// THE WALK (nwc_walk) finds the same answer through a cell grid over the face centroids (cell size h, cells [lo, hi], the largest
// rho_f = rho_max).  With E = NWC_REL_SLACK (max |o_k| + max |lo_k|, |hi_k|), an absolute allowance seven orders above the rounding of
// any coordinate here, and pad = rho_max + NWC_CELL_SLACK h + E:
//   - a direction of any finite length: the walk never uses d or L themselves (d.d leaves double's normal range beyond |d| = 1e154 and
//     below 1e-154: L would be inf or carry no digits).  It follows the same line along u = d / dm, dm = the largest |d_k|: every
//     |u_k| <= 1 and one is 1, Lu = sqrt(u.u) lies in [1, sqrt 3], and a parameter t of the definition stands at tau = t dm along u, at
//     arc length tau Lu.  Each u_k is rounded once, which moves a point of the line by 1e-16 of its distance from o: far inside E.  A
//     tau that overflows is +inf and only ever stands on the safe side of a comparison; one that underflows is off by 5e-324;
//   - clip: every hit point lies within rho_max of a centroid, so inside the box [lo - pad, hi + pad]; a slab test per axis (an axis
//     with u_k == 0 is an inside test, not a division) gives [tau0, tau1] within [0, t_max dm]; empty means no hit.  The axis with
//     |u_k| = 1 bounds tau1 - tau0 by the box's extent, so the number of pieces is bounded by the grid, whatever the direction;
//   - pieces: the arc length [tau0 Lu - pad - E, tau1 Lu + pad + E] is cut into pieces of length h.  Piece j with midpoint m_j visits
//     the cells that overlap the box m_j +- (h / 2 + rho_max + E) (+ NWC_CELL_SLACK cells), row by row; a centroid c_g read there is
//     examined only if its arc coordinate s_g = ((c_g - o).u) / Lu has floor((s_g - start) / h) == j -- one piece at most, so every
//     face is examined at most once -- and passed over if it lies farther than rho_g (1 + NWC_RHO_SLACK) + E from the line;
//   - why nothing is lost: a hit point x of face g is on the line and within rho_g of c_g, so c_g is within rho_g of the line, s_g is
//     within rho_g of t dm Lu, which is inside the arc range, and c_g is within h / 2 along the line and rho_g across it of m_j, inside
//     the box of its piece;
//   - stopping (first-hit mode only): before piece j, once t_best dm Lu + pad + E < the piece's start: every face examined later
//     has s_g >= that start and t dm Lu >= s_g - rho_g, strictly beyond the best.
// One oversize face raises rho_max: every piece's box then covers the grid and every ray reads every centroid once per piece -- slow,
// never inexact.  There is no DDA and no list of oversize faces.
// No HIP header is needed: without a HIP compiler NWX_HD is plain `inline`.
#pragma once
#include "nw_intersections_core.h"

#define NWC_RHO_SLACK BQ_FACE_RHO_SLACK    // relative enlargement of rho_f (nw_bq_core.h: 1e-9)
#define NWC_CELL_SLACK 1e-6       // of a cell, added to every box in cell units (the intersection unit's NWX_CELL_SLACK)
#define NWC_REL_SLACK 1e-9        // of the largest coordinate, an absolute allowance for the rounding of points along a ray
#define NWC_INFO_EXITS 1          // bit 0 of the info word: den > 0 at the nearest hit

// o, d, L = sqrt(d.d): the definition's; dm = the largest |d_k|, u = d / dm, Lu = sqrt(u.u): the walk's (not numbers if d is zero)
struct nwc_ray { nwx_v3 o, d, u; double L, dm, Lu, t_max; int skip_vertex, skip_face; };

NWX_HD nwc_ray nwc_make_ray(const double *o, const double *d, int skip_vertex, int skip_face, double t_max)
{
    nwc_ray r;
    r.o = nwx_v3{o[0], o[1], o[2]};
    r.d = nwx_v3{d[0], d[1], d[2]};
    r.L = sqrt(nwx_dot(r.d, r.d));
    r.dm = fmax(fmax(fabs(d[0]), fabs(d[1])), fabs(d[2]));
    r.u = nwx_v3{d[0] / r.dm, d[1] / r.dm, d[2] / r.dm};
    r.Lu = sqrt(nwx_dot(r.u, r.u));
    r.t_max = t_max;
    r.skip_vertex = skip_vertex;
    r.skip_face = skip_face;
    return r;
}

// whether the ray hits face f = T, whose centroid is c and whose enlarged radius is rho; *t and *exits are written on a hit
NWX_HD bool nwc_ray_face(const nwc_ray &r, int f, const nwx_tri &T, const nwx_v3 &c, double rho, double *t, bool *exits)
{
    const nwx_v3 n = nwx_normal(T);
    if (!(nwx_dot(n, n) > 0.0)) return false;
    if (T.i0 == r.skip_vertex || T.i1 == r.skip_vertex || T.i2 == r.skip_vertex || f == r.skip_face) return false;
    const nwx_v3 ea = nwx_sub(T.a, r.o), eb = nwx_sub(T.b, r.o), ec = nwx_sub(T.c, r.o);
    const double w0 = nwx_dot(nwx_cross(ea, eb), r.d), w1 = nwx_dot(nwx_cross(eb, ec), r.d), w2 = nwx_dot(nwx_cross(ec, ea), r.d);
    const bool pos = w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0, neg = w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0;
    if (!(pos || neg) || (w0 == 0.0 && w1 == 0.0 && w2 == 0.0)) return false;
    const double den = nwx_dot(n, r.d);
    if (!(den != 0.0)) return false;
    const double tt = nwx_dot(n, ea) / den;
    if (!(tt > 0.0 && tt <= r.t_max)) return false;
    const nwx_v3 x = nwx_v3{r.o.x + tt * r.d.x, r.o.y + tt * r.d.y, r.o.z + tt * r.d.z};
    const nwx_v3 e = nwx_sub(x, c);
    if (!(nwx_dot(e, e) <= rho * rho)) return false;
    *t = tt;
    *exits = den > 0.0;
    return true;
}

// what a ray has found so far
struct nwc_best { double t; int face, info, hits; };

NWX_HD nwc_best nwc_nothing()
{
    nwc_best b;
    b.t = INFINITY; b.face = -1; b.info = 0; b.hits = 0;
    return b;
}

// a hit of face f at t: the nearest wins, equal t goes to the smaller face id
NWX_HD void nwc_take(nwc_best &b, double t, int f, bool exits)
{
    ++b.hits;
    if (t < b.t || (t == b.t && f < b.face)) { b.t = t; b.face = f; b.info = exits ? NWC_INFO_EXITS : 0; }
}

// the definition, face by face
NWX_HD nwc_best nwc_cast_all_faces(const float *pos, const int32_t *faces, int nf, const nwc_ray &r)
{
    nwc_best b = nwc_nothing();
    if (!(r.L > 0.0)) return b;
    for (int f = 0; f < nf; ++f) {
        const nwx_tri T = nwx_load(pos, faces, f);
        nwx_v3 c;
        const double rho = nwx_face_centroid(T, &c) * (1.0 + NWC_RHO_SLACK);
        double t;
        bool exits;
        if (nwc_ray_face(r, f, T, c, rho, &t, &exits)) nwc_take(b, t, f, exits);
    }
    return b;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------------
struct nwc_point { double x, y, z; long long i; };             // a centroid in cell order with its face id (bq::PtF64's layout)

struct nwc_mesh {
    const float *pos;
    const int32_t *faces;
    int nf;
    const nwc_point *pts;
    const int *cstart;                                        // cell (x, y, z) = (z d1 + y) d0 + x holds pts[cstart[cell] .. cstart[cell + 1])
    const double *rho;                                        // per face, enlarged
    double rho_max, lo0, lo1, lo2, hi0, hi1, hi2, h;
    int d0, d1, d2;
};

struct nwc_walk_stats { long long pieces, read, tested; };

// the cells [c0, c1] along one axis that a box of half-width w cells around the coordinate x can overlap
NWX_HD void nwc_cell_range(double x, double lo, double h, int dim, double w, int &c0, int &c1)
{
    const double t = (x - lo) / h;
    c0 = (int)fmin(fmax(floor(t - w - NWC_CELL_SLACK), 0.0), (double)(dim - 1));
    c1 = (int)fmin(fmax(floor(t + w + NWC_CELL_SLACK), 0.0), (double)(dim - 1));
}

// one axis of the clip: [t0, t1] cut to where o + t d lies in [lo, hi] -> false if the axis alone excludes the ray
NWX_HD bool nwc_slab(double o, double d, double lo, double hi, double &t0, double &t1)
{
    if (d == 0.0) return o >= lo && o <= hi;
    const double ta = (lo - o) / d, tb = (hi - o) / d;
    t0 = fmax(t0, fmin(ta, tb));
    t1 = fmin(t1, fmax(ta, tb));
    return true;
}

template <bool COUNT>
NWX_HD nwc_best nwc_walk(const nwc_mesh &m, const nwc_ray &r, nwc_walk_stats *st)
{
    nwc_best b = nwc_nothing();
    st->pieces = st->read = st->tested = 0;
    if (!(r.L > 0.0)) return b;
    const double omax = fmax(fmax(fabs(r.o.x), fabs(r.o.y)), fabs(r.o.z));
    const double gmax = fmax(fmax(fmax(fabs(m.lo0), fabs(m.hi0)), fmax(fabs(m.lo1), fabs(m.hi1))), fmax(fabs(m.lo2), fabs(m.hi2)));
    const double E = NWC_REL_SLACK * (omax + gmax);
    const double pad = (m.rho_max + NWC_CELL_SLACK * m.h) + E;
    double t0 = 0.0, t1 = r.t_max * r.dm;                         // (parameters along u from here on: tau = t dm)
    if (!nwc_slab(r.o.x, r.u.x, m.lo0 - pad, m.hi0 + pad, t0, t1)) return b;
    if (!nwc_slab(r.o.y, r.u.y, m.lo1 - pad, m.hi1 + pad, t0, t1)) return b;
    if (!nwc_slab(r.o.z, r.u.z, m.lo2 - pad, m.hi2 + pad, t0, t1)) return b;
    if (!(t0 <= t1)) return b;
    // (t1 is finite: the axis with |u_k| == 1 bounds it by the box)
    const double start = (t0 * r.Lu - pad) - E, stop = (t1 * r.Lu + pad) + E;
    const double np_ = ceil((stop - start) / m.h);
    if (!(np_ == np_)) return b;                                  // (cannot happen with finite arguments; never a walk of unknown length)
    const long long n_pieces = np_ < 1.0 ? 1 : (np_ < 1073741824.0 ? (long long)np_ : 1073741824ll);
    const double w = ((0.5 * m.h + m.rho_max) + E) / m.h;
    for (long long j = 0; j < n_pieces; ++j) {
        const double s_lo = start + (double)j * m.h;
        if (!COUNT && b.face >= 0 && ((b.t * r.dm) * r.Lu + pad) + E < s_lo) break;
        ++st->pieces;
        const double u = (s_lo + 0.5 * m.h) / r.Lu;
        int x0, x1, y0, y1, z0, z1;
        nwc_cell_range(r.o.x + u * r.u.x, m.lo0, m.h, m.d0, w, x0, x1);
        nwc_cell_range(r.o.y + u * r.u.y, m.lo1, m.h, m.d1, w, y0, y1);
        nwc_cell_range(r.o.z + u * r.u.z, m.lo2, m.h, m.d2, w, z0, z1);
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * m.d1 + y) * m.d0;
                const int s = m.cstart[row + x0], e = m.cstart[row + x1 + 1];
                for (int p = s; p < e; ++p) {
                    const nwc_point q = m.pts[p];
                    const int g = (int)q.i;
                    if (g < 0 || g >= m.nf) continue;             // (cannot happen: the grid's points are numbered by face)
                    ++st->read;
                    const nwx_v3 c = nwx_v3{q.x, q.y, q.z};
                    const double sg = nwx_dot(nwx_sub(c, r.o), r.u) / r.Lu;
                    if (!(floor((sg - start) / m.h) == (double)j)) continue;      // another piece's, or nobody's
                    const double ug = sg / r.Lu;
                    const nwx_v3 off = nwx_sub(c, nwx_v3{r.o.x + ug * r.u.x, r.o.y + ug * r.u.y, r.o.z + ug * r.u.z});
                    const double rho = m.rho[g], reach = rho * (1.0 + NWC_RHO_SLACK) + E;
                    if (nwx_dot(off, off) > reach * reach) continue;              // the face's ball does not touch the line
                    ++st->tested;
                    double t;
                    bool exits;
                    if (nwc_ray_face(r, g, nwx_load(m.pos, m.faces, g), c, rho, &t, &exits)) nwc_take(b, t, g, exits);
                }
            }
        }
    }
    return b;
}
