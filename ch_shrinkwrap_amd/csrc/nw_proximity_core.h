// The arithmetic of the mesh-to-mesh distance (include/nw_proximity.h: nwm_query), shared by the kernels of nw_proximity.hip and by
// whoever compiles this header for the CPU (tests/test_proximity_core_cpu.py builds a shim from it with g++ -ffp-contract=off).
// tests/mesh_proximity_ref.py restates it in NumPy, operation for operation and by brute force over all pairs of faces.  The
// point-triangle distance and the face centroid are nw_distance_core.h's, the segment-face test and the vectors
// nw_intersections_core.h's: included, not copied.
//
// Everything is float64 on the float32 vertex positions widened to double, in nw_distance_core.h's written order of operations (a dot
// product is (u0 v0 + u1 v1) + u2 v2, a cross product rounds each product and subtracts, a point p + t d is taken per axis as
// p_k + t * d_k); nothing may be contracted into an fma: compile with -ffp-contract=off.  PYME is not in the reference tree and upstream
// has no such module: the definition is this project's own.
//
// nwm_tri_tri(A, B): the squared distance of triangle A (a face of the querying mesh) from triangle B (a face of the mesh in the
// context), a kind code and one closest point on each.
//   1. Piercing, only if both faces have n.n > 0 (n = (b - a) x (c - a)).  Six tests in this order: nwx_seg_tri(A_k, A_k+1; B) for
//      k = 0, 1, 2, then nwx_seg_tri(B_k, B_k+1; A) for k = 0, 1, 2.  At the first that holds: d2 = +0.0, kind 0, and both closest
//      points are the piercing point p + t (q - p), t = (n.(a - p)) / (n.(q - p)), with p -> q the segment, n the pierced face's normal
//      and a its corner 0.
//   2. Otherwise the candidates in this order, a later one replacing the best only when it is strictly nearer:
//      kinds 1-3      nwd_point_triangle(A_k, B), k = 0, 1, 2: the closest points are A_k and the one the function returns;
//      kinds 4-6      nwd_point_triangle(B_k, A), k = 0, 1, 2: the closest points are the one the function returns and B_k;
//      kinds 7+3i+j   edge i of A (A_i -> A_i+1) against edge j of B (B_j -> B_j+1), interior against interior only: with u, v the
//                     edge vectors, p, q their starts and w = p - q: a = u.u, b = u.v, c = v.v, d = u.w, e = v.w, den = a c - b b; the
//                     candidate exists only if den > 0 and s = (b e - c d) / den, t = (a e - b d) / den both lie strictly inside
//                     (0, 1); its points are p + s u and q + t v, its value |(p + s u) - (q + t v)|^2.
//      Every boundary case of a segment pair is an end of one segment against the other segment, and the six point-triangle candidates
//      cover those.  Every candidate is the distance of two points of the two triangles, so rounding can only overstate the distance,
//      by its own size.  A near-parallel pair whose den is rounding noise gives a valid, not minimal candidate; the end-point candidates
//      carry the minimum there.  A flat face is skipped by the piercing tests, and nwd_point_triangle makes it its three segments.
//      (So a flat face that passes through the other face's interior is as far away as its corners and edges are, not at 0.)
//
// Per face f of A with a band d_cap (a positive double, +inf allowed): the minimum of nwm_tri_tri(f, g) over all faces g of B, the
// smallest g among equal d2 whatever the visiting order.  The face is in band iff sqrt(d2) <= d_cap (nwm_in_band):
//   in band      distance = sqrt(d2), partner = g, the kind and the two closest points;
//   out of band  distance = +inf, partner = -1, kind = -1, closest points NaN.
// Nothing depends on the cell size, the launch geometry or the order of B's faces beyond the tie rule.  The function is not promised
// to be symmetric bit for bit in its two arguments (the edge-edge roles swap): A against B and B against A are two calls.  A mesh
// against itself is out of scope: every face would find itself at 0.
//
// The walk (nwm_walk).  Every face has a centroid c and rho, the largest distance from c to a corner (nwd_face_centroid), a hair
// enlarged; rho_max is the largest rho of B.  Face f of A walks rings of B's centroid grid around the cell of c_f (of its projection
// onto the grid's box, if it lies outside).  A centroid in ring r lies at least lbd = (r - 1) h from the projection along one axis, so
// its face is at least sqrt(lbd^2 + out^2) - rho_f - rho_max from face f; the walk ends when that is strictly more than
// min(best, d_cap), so a face at exactly d_cap and all equally near faces are seen.  A far face stops after
// ceil((d_cap + rho_f + rho_max) / h) + 1 rings with nothing found.  A candidate g is passed over without the exact test when
// |c_f - c_g| (1 - slack) - rho_g - rho_f > min(best, d_cap) (nwm_beyond compares with the best in squares, a hair shrunk).  The slack (NWM_CORE_SLACK, used as NWX_SLACK is) is relative, 1e-9: the
// bounds are float64 expressions of a handful of operations, whose rounding is some 1e-15 of their value, so a bound weakened by 1e-9
// of itself can never pass over a face that exact arithmetic would keep, and 1e-9 of a distance changes no count that matters.
// The walk keeps only (d2, g): the pair test is some 1500 float64 operations and the record must stay small; the kind and the closest
// points come from evaluating the winning pair once more (the pair function is pure: the same bits).
// One face much larger than the rest, in either mesh, raises rho_f or rho_max and makes walks long, never inexact.
// No HIP header is needed.
#pragma once
#include "nw_distance_core.h"
#include "nw_intersections_core.h"

// The stages of the pair test are loops over k (or over the 3 x 3 edge pairs) with the corners of step k picked by selects.  On the
// device the loops are kept as loops (unrolled, the compiler runs the stages side by side: 370 VGPRs against 168); for the CPU the
// macro is empty and the compiler is free to unroll, so the CPU tests run another loop shape than the device.  The operations and
// their order are the same in both, and without contraction that is all the bits depend on; tests/test_hip_proximity.py asks the
// device itself for them.
#if defined(__HIPCC__)
#define NWM_KEEP_LOOP _Pragma("unroll 1")
#else
#define NWM_KEEP_LOOP
#endif
#define NWM_CORE_SLACK BQ_FACE_RHO_SLACK      // (nw_bq_core.h: 1e-9) relative slack of every bound: far above the rounding of a float64 distance, far below what matters

// the centroid grid as the walk reads it (the layout of the query units' shared grid in double) and a sorted centroid with its face id
struct nwm_grid {
    double lo[3], hi[3];
    double h;
    int dims[3];
};
struct nwm_pt { double x, y, z; long long i; };

struct nwm_best {
    double d2;                // the best squared distance
    int face;
};

// The candidate cell size of a band d_cap (bq::face_cell takes it from there): max(2 m, min((d_cap + rho_max) / 2, 16 m)) with m the
// mean rho of B.  2 m is a face or two per occupied cell of a surface; half of d_cap + rho_max ends a far face's walk after three or
// four rings; 16 m is where a walk without a band was fastest when it was measured (profiles/proximity.txt: its rings cost more than
// the centroids a larger cell makes it read), and it keeps a wide band from turning the grid into a few cells that hold every centroid.
inline double nwm_band_cell(double rho_mean, double rho_max, double d_cap)
{
    return std::max(2.0 * rho_mean, std::min((d_cap + rho_max) / 2.0, 16.0 * rho_mean));
}

NWD_HD bool nwm_in_band(double u, double d_cap) { return u <= d_cap; }

// whether a lower bound x of a distance is strictly beyond min(sqrt(d2), d_cap).  Against the best it is compared in squares, a hair
// shrunk, so that the walk carries d2 alone and no square root of it: x^2 (1 - slack) > d2 implies x > sqrt(d2) with room to spare
NWD_HD bool nwm_beyond(double x, double d2, double d_cap) { return x > d_cap || (x > 0.0 && (x * x) * (1.0 - NWM_CORE_SLACK) > d2); }

// u or v, component by component (a conditional between two structs may be compiled as a choice between their addresses, and a
// corner picked through an address goes to scratch on the device)
NWD_HD nwx_v3 nwm_pick(bool c, const nwx_v3 &u, const nwx_v3 &v) { return nwx_v3{c ? u.x : v.x, c ? u.y : v.y, c ? u.z : v.z}; }

// corner k (k = 0 .. 3, corner 3 being corner 0 again) of a face, by selects
NWD_HD nwx_v3 nwm_corner_of(const nwx_tri &t, int k) { return nwm_pick(k == 1, t.b, nwm_pick(k == 2, t.c, t.a)); }

// the edges k -> k+1 of S, k = 0, 1, 2, against the face T with normal n: whether one pierces it, and at the first that does the
// piercing point p + t (q - p), t = (n.(T_0 - p)) / (n.(q - p))
NWD_HD bool nwm_pierce(const nwx_tri &S, const nwx_tri &T, const nwx_v3 &n, nwx_v3 &at)
{
    NWM_KEEP_LOOP
    for (int k = 0; k < 3; ++k) {
        const nwx_v3 p = nwm_corner_of(S, k), q = nwm_corner_of(S, k + 1);
        if (nwx_seg_tri(p, q, T, n)) {
            const nwx_v3 d = nwx_sub(q, p);
            const double t = nwx_dot(n, nwx_sub(T.a, p)) / nwx_dot(n, d);
            at = nwx_v3{p.x + t * d.x, p.y + t * d.y, p.z + t * d.z};
            return true;
        }
    }
    return false;
}

// candidate kinds 1-3 (point_of_a) and 4-6: a corner p of one triangle against the other triangle t0 t1 t2
NWD_HD void nwm_corner(const nwx_v3 &p, const float *t0, const float *t1, const float *t2, bool point_of_a, int kind, double &best, int &bk,
                       nwx_v3 &ca, nwx_v3 &cb)
{
    const double q[3] = {p.x, p.y, p.z};
    double c[3];
    int feature;
    const double d2 = nwd_point_triangle(q, t0, t1, t2, c, &feature);
    if (d2 < best) {
        best = d2; bk = kind;
        const nwx_v3 on = nwx_v3{c[0], c[1], c[2]};
        ca = nwm_pick(point_of_a, p, on);
        cb = nwm_pick(point_of_a, on, p);
    }
}

// candidate kinds 7..15: the interiors of the segments p -> p1 (of A) and q -> q1 (of B)
NWD_HD void nwm_edge_edge(const nwx_v3 &p, const nwx_v3 &p1, const nwx_v3 &q, const nwx_v3 &q1, int kind, double &best, int &bk, nwx_v3 &ca, nwx_v3 &cb)
{
    const nwx_v3 u = nwx_sub(p1, p), v = nwx_sub(q1, q), w = nwx_sub(p, q);
    const double a = nwx_dot(u, u), b = nwx_dot(u, v), c = nwx_dot(v, v), d = nwx_dot(u, w), e = nwx_dot(v, w);
    const double den = a * c - b * b;
    if (!(den > 0.0)) return;
    const double s = (b * e - c * d) / den, t = (a * e - b * d) / den;
    if (!(s > 0.0 && s < 1.0 && t > 0.0 && t < 1.0)) return;
    const nwx_v3 x = nwx_v3{p.x + s * u.x, p.y + s * u.y, p.z + s * u.z}, y = nwx_v3{q.x + t * v.x, q.y + t * v.y, q.z + t * v.z};
    const nwx_v3 r = nwx_sub(x, y);
    const double d2 = nwx_dot(r, r);
    if (d2 < best) { best = d2; bk = kind; ca = x; cb = y; }
}

// the squared distance of the triangle a0 a1 a2 from the triangle b0 b1 b2 (float32 corners); *kind_out = 0..15, ca / cb = one closest
// point on each
NWD_HD double nwm_tri_tri(const float *a0, const float *a1, const float *a2, const float *b0, const float *b1, const float *b2, int *kind_out,
                          double *ca_out, double *cb_out)
{
    nwx_tri A, B;
    A.i0 = A.i1 = A.i2 = B.i0 = B.i1 = B.i2 = 0;                  // (the vertex ids play no part between two meshes)
    A.a = nwx_widen(a0); A.b = nwx_widen(a1); A.c = nwx_widen(a2);
    B.a = nwx_widen(b0); B.b = nwx_widen(b1); B.c = nwx_widen(b2);
    const nwx_v3 nA = nwx_normal(A), nB = nwx_normal(B);
    double best = INFINITY;
    int kind = 1;
    nwx_v3 ca = A.a, cb = B.a;
    bool pierced = false;
    // The tests and the candidates run one after the other in loops that stay loops on the device (NWM_KEEP_LOOP): unrolled, the
    // compiler runs them side by side and the pair test alone outgrows the register file.  The corners of step k are picked with
    // selects, never from an array indexed at run time.
    if (nwx_dot(nA, nA) > 0.0 && nwx_dot(nB, nB) > 0.0) {
        pierced = nwm_pierce(A, B, nB, ca);
        if (!pierced) pierced = nwm_pierce(B, A, nA, ca);
        if (pierced) { cb = ca; best = 0.0; kind = 0; }
    }
    if (!pierced) {
        NWM_KEEP_LOOP
        for (int k = 0; k < 3; ++k)
            nwm_corner(nwm_corner_of(A, k), b0, b1, b2, true, 1 + k, best, kind, ca, cb);
        NWM_KEEP_LOOP
        for (int k = 0; k < 3; ++k)
            nwm_corner(nwm_corner_of(B, k), a0, a1, a2, false, 4 + k, best, kind, ca, cb);
        NWM_KEEP_LOOP
        for (int ij = 0; ij < 9; ++ij) {
            const int i = ij / 3, j = ij - 3 * i;
            nwm_edge_edge(nwm_corner_of(A, i), nwm_corner_of(A, i + 1), nwm_corner_of(B, j), nwm_corner_of(B, j + 1), 7 + ij, best, kind, ca, cb);
        }
    }
    *kind_out = kind;
    ca_out[0] = ca.x; ca_out[1] = ca.y; ca_out[2] = ca.z;
    cb_out[0] = cb.x; cb_out[1] = cb.y; cb_out[2] = cb.z;
    return best;
}

// cell index along one axis: the expression the grid was binned with
NWD_HD int nwm_cell_1d(double x, double lo, double h, int dim)
{
    const double t = floor((x - lo) / h);
    return (int)fmin(fmax(t, 0.0), (double)(dim - 1));
}

// the faces of B whose centroids lie in cells [c0, c1] of one row against the face a0 a1 a2 of A (centroid cf, radius rho_f)
NWD_HD void nwm_scan_cells(const nwm_pt *pts, const int *cstart, int c0, int c1, const double *cf, double rho_f, const float *a0, const float *a1,
                           const float *a2, const float *bpos, const int32_t *bfaces, const double *rho, int nf, double d_cap, nwm_best &b,
                           int &n_centroids, int &n_tests)
{
    const int s = cstart[c0], e = cstart[c1 + 1];
    n_centroids += e - s;
    NWM_KEEP_LOOP
    for (int p = s; p < e; ++p) {
        const nwm_pt r = pts[p];
        const int g = (int)r.i;
        if (g < 0 || g >= nf) continue;                           // (cannot happen: the grid's points are numbered by face)
        const double ex = r.x - cf[0], ey = r.y - cf[1], ez = r.z - cf[2];
        const double cd = sqrt((ex * ex + ey * ey) + ez * ez);
        if (nwm_beyond((cd * (1.0 - NWM_CORE_SLACK) - rho[g]) - rho_f, b.d2, d_cap)) continue;     // the whole face is farther than the best and the band
        const int ia = bfaces[3 * (int64_t)g], ib = bfaces[3 * (int64_t)g + 1], ic = bfaces[3 * (int64_t)g + 2];
        double ca[3], cb[3];
        int kind;
        const double d2 = nwm_tri_tri(a0, a1, a2, bpos + 3 * (int64_t)ia, bpos + 3 * (int64_t)ib, bpos + 3 * (int64_t)ic, &kind, ca, cb);
        ++n_tests;
        if (d2 < b.d2 || (d2 == b.d2 && g < b.face)) { b.d2 = d2; b.face = g; }
    }
}

// The capped walk of one face of A -> the number of rings walked; b.face = INT32_MAX if no face was examined.  rho[g] must cover face g
// of B from its centroid, rho_max every rho[g], and rho_f the face a0 a1 a2 from cf.
NWD_HD int nwm_walk(const double *cf, double rho_f, const float *a0, const float *a1, const float *a2, const float *bpos, const int32_t *bfaces, int nf,
                    const nwm_pt *pts, const int *cstart, const double *rho, double rho_max, const nwm_grid &g, double d_cap, nwm_best &b,
                    int &n_centroids, int &n_tests)
{
    // the centroid's projection onto the box of B's centroids: every centroid c has |c - q|^2 >= |c - q'|^2 + |q - q'|^2
    const double px = fmin(fmax(cf[0], g.lo[0]), g.hi[0]), py = fmin(fmax(cf[1], g.lo[1]), g.hi[1]), pz = fmin(fmax(cf[2], g.lo[2]), g.hi[2]);
    const double out2 = (((cf[0] - px) * (cf[0] - px) + (cf[1] - py) * (cf[1] - py)) + (cf[2] - pz) * (cf[2] - pz)) * (1.0 - NWM_CORE_SLACK);
    const int cx = nwm_cell_1d(px, g.lo[0], g.h, g.dims[0]), cy = nwm_cell_1d(py, g.lo[1], g.h, g.dims[1]), cz = nwm_cell_1d(pz, g.lo[2], g.h, g.dims[2]);
    const int mx = cx > g.dims[0] - 1 - cx ? cx : g.dims[0] - 1 - cx, my = cy > g.dims[1] - 1 - cy ? cy : g.dims[1] - 1 - cy;
    const int mz = cz > g.dims[2] - 1 - cz ? cz : g.dims[2] - 1 - cz;
    const int rmax = mx > my ? (mx > mz ? mx : mz) : (my > mz ? my : mz);
    b.d2 = INFINITY; b.face = INT32_MAX;
    int r = 0;
    for (; r <= rmax; ++r) {
        // a centroid in a cell of ring r lies at least (r - 1) h from the projection along one axis; its face reaches at most rho_max
        // towards face f, which reaches at most rho_f towards it.  The walk ends when that exceeds the best distance or the band --
        // strictly, so that equally near faces and a face at exactly d_cap are all seen
        const double lbd = (double)(r > 1 ? r - 1 : 0) * g.h * (1.0 - NWM_CORE_SLACK);
        if (nwm_beyond((sqrt(lbd * lbd + out2) * (1.0 - NWM_CORE_SLACK) - rho_f) - rho_max, b.d2, d_cap)) break;
        const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < g.dims[2] - 1 ? cz + r : g.dims[2] - 1;
        const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < g.dims[1] - 1 ? cy + r : g.dims[1] - 1;
        const int xa = cx - r > 0 ? cx - r : 0, xb = cx + r < g.dims[0] - 1 ? cx + r : g.dims[0] - 1;
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * g.dims[1] + y) * g.dims[0];
                // a row of the ring's shell is one run of cells; any other row meets the ring in its two end cells.  One call site
                // for both: the pair test is large, and it is compiled once
                const bool shell = z - cz == r || cz - z == r || y - cy == r || cy - y == r;
                NWM_KEEP_LOOP
                for (int part = 0; part < (shell ? 1 : 2); ++part) {
                    const int x = part ? cx + r : cx - r;
                    if (!shell && (x < 0 || x >= g.dims[0])) continue;
                    nwm_scan_cells(pts, cstart, row + (shell ? xa : x), row + (shell ? xb : x), cf, rho_f, a0, a1, a2, bpos, bfaces, rho, nf, d_cap, b,
                                   n_centroids, n_tests);
                }
            }
        }
    }
    return r;
}

// What a face's walk leaves behind: the partner, or -1 out of band (or if no face was examined)
NWD_HD int nwm_partner(const nwm_best &b, double d_cap) { return (b.face == INT32_MAX || !nwm_in_band(sqrt(b.d2), d_cap)) ? -1 : b.face; }

// The second evaluation of the winning pair: distance, kind and closest points of an in-band face, the out-of-band values otherwise.
// -> the pair's d2 (NaN out of band): the same bits as the walk's, as the pair function is pure
NWD_HD double nwm_finish(const float *a0, const float *a1, const float *a2, const float *bpos, const int32_t *bfaces, int partner, double *distance,
                         int *kind, double *ca, double *cb)
{
    if (partner < 0) {
        *distance = INFINITY; *kind = -1;
        ca[0] = ca[1] = ca[2] = cb[0] = cb[1] = cb[2] = NAN;
        return NAN;
    }
    const int ia = bfaces[3 * (int64_t)partner], ib = bfaces[3 * (int64_t)partner + 1], ic = bfaces[3 * (int64_t)partner + 2];
    const double d2 = nwm_tri_tri(a0, a1, a2, bpos + 3 * (int64_t)ia, bpos + 3 * (int64_t)ib, bpos + 3 * (int64_t)ic, kind, ca, cb);
    *distance = sqrt(d2);
    return d2;
}
