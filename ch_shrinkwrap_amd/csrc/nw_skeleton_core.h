// The definition of the level-set skeleton of a mesh (include/nw_skeleton.h), shared by the kernels of nw_skeleton.hip and by whoever
// compiles this header for the CPU (tests/test_skeleton_core_cpu.py builds a shim from it with g++ -ffp-contract=off):
//   - the band of a vertex and the pieces of a face, and the index of a piece;
//   - the band range two faces share across an edge;
//   - the crossing point of a level on an edge and the contour segment of a piece;
//   - the quantisation of positions and lengths into integers, with the proof that no node sum overflows.
// Upstream's SkeletonizeMembrane (mean-curvature flow with Voronoi poles) is not mirrored: this definition is the project's own.
// All arithmetic is float64 on the float32 positions and the float64 field.  Nothing may be contracted into an fma: compile with
// -ffp-contract=off.  No HIP header is needed: without a HIP compiler NWA_HD is plain `inline`.
//
// WHAT THIS IS.  A level-set diagram (a Reeb graph over bands) of ONE scalar field D on the mesh.  The surface is cut into the bands
// {k w <= D < (k + 1) w}; every connected piece of a band is a node; pieces of neighbouring bands that touch are joined by an arc.
// WHAT THIS IS NOT.  It is not a medial axis and not upstream's curve skeleton.  It depends on the field, and so on the source the field
// was grown from.  A sheet becomes a chain of nodes.  A LOOP NARROWER THAN A BAND VANISHES: where the band is wider than a hole, the
// pieces either side of the hole are one node.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NWA_HD __host__ __device__ __forceinline__
#else
#define NWA_HD inline
#endif

#define NWA_MAX_N (1ll << 30)        // vertices
#define NWA_MAX_FACES (1ll << 29)    // 3 * faces half-edges are indexed by an int
#define NWA_MAX_BAND (1ll << 30)     // the largest band index
#define NWA_MAX_PIECES (1ll << 28)   // pieces of one call
#define NWA_DEAD (-1)                // the band of a dead vertex
#define NWA_COORD_BITS 20            // a quantised coordinate lies in [0, 2^20]
#define NWA_LEN_SHIFT 10             // a quantised length counts quanta / 2^10
// the columns of a node's row of sums (uint64 each)
#define NWA_S_PIECES 0               // pieces
#define NWA_S_CENTROID 1             // 1, 2, 3: the sum over the pieces of (c0 + c1 + c2), the face's three quantised corners, per axis
#define NWA_S_SEGMENTS 4             // pieces that have a contour segment
#define NWA_S_LENGTH 5               // the sum of the quantised segment lengths l
#define NWA_S_MOMENT_LO 6            // 6, 7, 8: the sum of the low 32 bits of l * (a + b), a and b the segment's quantised ends, per axis
#define NWA_S_MOMENT_HI 9            // 9, 10, 11: the sum of the bits above them
#define NWA_S_COLUMNS 12

// half-edge h = 3 f + k runs from faces[f][k] to faces[f][(k + 1) % 3]
NWA_HD long long nwa_next(long long h) { return h - h % 3 + (h + 1) % 3; }

// ---- bands -------------------------------------------------------------------------------------------------------------------------------
// b(v) = floor(D[v] / w) in IEEE float64, as an integer.  +inf and every D < 0 (-inf too) are dead: NWA_DEAD.  *bad is set for a nan and
// for a band beyond NWA_MAX_BAND (then the result is NWA_DEAD as well, and the call is refused).  The quotient is compared as a double
// before it is converted: w may be so small that it is +inf.
NWA_HD int nwa_band(double D, double w, bool *bad)
{
    if (D != D) { *bad = true; return NWA_DEAD; }
    if (D < 0.0 || D == INFINITY) return NWA_DEAD;
    const double q = floor(D / w);
    if (!(q <= (double)NWA_MAX_BAND)) { *bad = true; return NWA_DEAD; }
    return (int)q;
}

// w > 0, finite
NWA_HD bool nwa_width_ok(double w) { return w > 0.0 && w < INFINITY; }

// A face's bands: lo = min b, hi = max b over its corners; a face with a dead corner is dead and has no piece (span 0).  Its pieces are
// (f, k) for lo <= k <= hi, stored band ascending: piece (f, k) has the index piece_start[f] + (k - lo), piece_start being the exclusive
// scan of the spans.
struct nwa_face_bands { int lo, hi, span; };

NWA_HD nwa_face_bands nwa_face(int b0, int b1, int b2)
{
    nwa_face_bands r;
    if (b0 < 0 || b1 < 0 || b2 < 0) { r.lo = r.hi = NWA_DEAD; r.span = 0; return r; }
    r.lo = b0 < b1 ? (b0 < b2 ? b0 : b2) : (b1 < b2 ? b1 : b2);
    r.hi = b0 > b1 ? (b0 > b2 ? b0 : b2) : (b1 > b2 ? b1 : b2);
    r.span = r.hi - r.lo + 1;
    return r;
}

// The bands in which the live faces f and g are joined across their common edge {u, v}: min(b(u), b(v)) .. max(b(u), b(v)) INCLUSIVE.
// Inside a triangle the region of one band is convex (a triangle cut by two parallel lines of the linear interpolant), so one piece per
// (face, band) is right; the region of band k touches the edge {u, v} exactly when k lies between the ends' bands, both included: the
// field runs through every value between D[u] and D[v] along the edge.  Both faces hold u and v, so both have a piece in each of these
// bands.  The fan of faces round a vertex is joined through the edges that hold the vertex.  This is right for any w, also far below the
// edge length, where most pieces hold no vertex at all; a definition on the vertices' bands alone breaks a tube apart there.
NWA_HD void nwa_edge_range(int bu, int bv, int *k0, int *k1)
{
    *k0 = bu < bv ? bu : bv;
    *k1 = bu < bv ? bv : bu;
}

// the face of piece p: the last f with piece_start[f] <= p (dead faces have span 0 and are never the last)
NWA_HD int nwa_piece_face(const int *piece_start, int nf, int p)
{
    int a = 0, b = nf;                                            // piece_start[a] <= p < piece_start[b]
    while (b - a > 1) {
        const int m = a + (b - a) / 2;
        if (piece_start[m] <= p) a = m; else b = m;
    }
    return a;
}

// ---- the contour of a piece --------------------------------------------------------------------------------------------------------------
// The level of band k is L = (k + 1/2) w; a corner is below when D < L.  For k <= 2^30 a corner below has a band <= k and a corner that is
// not below a band >= k, also after rounding: D < fl((k + 1/2) w) gives fl(D / w) < k + 1, and D >= fl((k + 1/2) w) gives fl(D / w) > k
// (three roundings of 2^-53 each against a margin of 1 / (2 k + 1) >= 2^-32).  So a face crossed by the level of band k has a piece there.
NWA_HD double nwa_level(int k, double w) { return ((double)k + 0.5) * w; }

// The crossing point on the edge whose below end is pu (field Du < L) and whose other end is pv (Dv >= L): pu + t (pv - pu) with
// t = (L - Du) / (Dv - Du).  ALWAYS from the below end: the two faces of an edge then compute the same bits.  0 < t <= 1: the rounded
// differences keep their order.
NWA_HD void nwa_crossing(const float *pu, const float *pv, double Du, double Dv, double L, double *x)
{
    const double t = (L - Du) / (Dv - Du);
    x[0] = (double)pu[0] + t * ((double)pv[0] - (double)pu[0]);
    x[1] = (double)pu[1] + t * ((double)pv[1] - (double)pu[1]);
    x[2] = (double)pu[2] + t * ((double)pv[2] - (double)pu[2]);
}

// ---- quantisation ------------------------------------------------------------------------------------------------------------------------
// Positions are taken relative to the bounding box's lower corner `low` (the smallest float32 coordinate per axis, as a double) and
// counted in quanta q, a power of two: with E the largest of the box's three extents (float64 differences of float32 numbers) and
// E = m 2^x, 1/2 <= m < 1 (frexp), q = 2^(x - 20); E = 0 gives q = 1.  Then E / q < 2^20, and 2^-168 <= q <= 2^109: dividing by q is exact.
//     c(x) = floor((x - low) / q + 1/2), clamped to [0, 2^20]                        (a coordinate)
//     l(a, b) = floor(sqrt((double)|a - b|^2) * 2^10 + 1/2), a and b quantised points  (a length, in units of q / 2^10)
// |a - b|^2 <= 3 * 2^40 is an exact integer and an exact double, and sqrt is correctly rounded, so l is a function of a and b alone.
//
// Proof that no sum of a node overflows an unsigned 64-bit word, for at most P <= 2^28 pieces in one call (a node has at most P):
//     pieces, segments                 <= 2^28
//     centroid: c0 + c1 + c2           <= 3 * 2^20 < 2^22 per piece                          sum < 2^50
//     length: l                        <= sqrt(3) 2^20 2^10 + 1 < 2^31 per piece             sum < 2^59
//     moment: l (a + b)                < 2^31 * 2^21 = 2^52 per piece: its sum can pass 2^64, so it is added in two limbs,
//                                      the low 32 bits (< 2^32 per piece, sum < 2^60) and the bits above (< 2^20 per piece, sum < 2^48)
// Every term is an integer >= 0, integer addition commutes, so the sums do not depend on the order of the atomics.
//
// What it costs.  q <= E 2^-19 (E >= 2^(x - 1)).  A quantised point is within q / 2 per axis of the point; a node's position is a mean of
// such points with non-negative weights (the contour centroid: segment midpoints weighted by l; else the mean of the face centroids), so
// it lies within q / 2 <= E 2^-20 per axis of the same mean of the unquantised points.  A weight l 2^-10 q differs from the length of
// the unquantised segment by at most (sqrt(3) + 2^-11) q, and the perimeter of a node of n segments by at most n times that.
NWA_HD double nwa_quantum(double extent)
{
    if (!(extent > 0.0)) return 1.0;
    int x;
    (void)frexp(extent, &x);
    return ldexp(1.0, x - NWA_COORD_BITS);
}

NWA_HD long long nwa_coord(double x, double low, double q)
{
    const double c = floor((x - low) / q + 0.5);
    const double top = (double)(1ll << NWA_COORD_BITS);
    return (long long)(c < 0.0 ? 0.0 : c > top ? top : c);
}

NWA_HD unsigned long long nwa_length(const long long *a, const long long *b)
{
    const long long dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const long long d2 = dx * dx + dy * dy + dz * dz;
    return (unsigned long long)floor(sqrt((double)d2) * (double)(1 << NWA_LEN_SHIFT) + 0.5);
}

// What piece (f, k) adds to its node's row.  D, pos: the field and the float32 positions; v[3]: the face's corners; low[3], q: the
// quantisation.  add[NWA_S_COLUMNS] gets the terms; returns whether the piece has a contour segment (columns 4 .. 11 are zero if not).
// The corners are picked with selects, never from an array indexed at run time.
NWA_HD bool nwa_piece_terms(const float *pos, const double *D, const int *v, int k, double w, const double *low, double q, unsigned long long *add)
{
    const float *p0 = pos + 3 * (long long)v[0], *p1 = pos + 3 * (long long)v[1], *p2 = pos + 3 * (long long)v[2];
    const double D0 = D[v[0]], D1 = D[v[1]], D2 = D[v[2]];
    add[NWA_S_PIECES] = 1;
    for (int c = 0; c < 3; ++c)
        add[NWA_S_CENTROID + c] = (unsigned long long)(nwa_coord((double)p0[c], low[c], q) + nwa_coord((double)p1[c], low[c], q) + nwa_coord((double)p2[c], low[c], q));
    for (int c = NWA_S_SEGMENTS; c < NWA_S_COLUMNS; ++c) add[c] = 0;
    const double L = nwa_level(k, w);
    const bool s0 = D0 < L, s1 = D1 < L, s2 = D2 < L;
    if (s0 == s1 && s1 == s2) return false;
    // the corner that is alone on its side: the two crossed edges are the ones that hold it
    const bool alone0 = s0 != s1 && s0 != s2, alone1 = s1 != s0 && s1 != s2;
    const float *pa = alone0 ? p0 : alone1 ? p1 : p2;             // the lone corner, then the other two
    const float *pb = alone0 ? p1 : alone1 ? p2 : p0;
    const float *pc = alone0 ? p2 : alone1 ? p0 : p1;
    const double Da = alone0 ? D0 : alone1 ? D1 : D2, Db = alone0 ? D1 : alone1 ? D2 : D0, Dc = alone0 ? D2 : alone1 ? D0 : D1;
    const bool a_below = alone0 ? s0 : alone1 ? s1 : s2;
    double x[3], y[3];
    if (a_below) { nwa_crossing(pa, pb, Da, Db, L, x); nwa_crossing(pa, pc, Da, Dc, L, y); }
    else         { nwa_crossing(pb, pa, Db, Da, L, x); nwa_crossing(pc, pa, Dc, Da, L, y); }
    long long a[3], b[3];
    for (int c = 0; c < 3; ++c) { a[c] = nwa_coord(x[c], low[c], q); b[c] = nwa_coord(y[c], low[c], q); }
    const unsigned long long l = nwa_length(a, b);
    add[NWA_S_SEGMENTS] = 1;
    add[NWA_S_LENGTH] = l;
    for (int c = 0; c < 3; ++c) {
        const unsigned long long P = l * (unsigned long long)(a[c] + b[c]);
        add[NWA_S_MOMENT_LO + c] = P & 0xffffffffull;
        add[NWA_S_MOMENT_HI + c] = P >> 32;
    }
    return true;
}

// an arc's key: the smaller node above the larger
NWA_HD unsigned long long nwa_arc_key(int n0, int n1)
{
    const unsigned long long a = (unsigned long long)(n0 < n1 ? n0 : n1), b = (unsigned long long)(n0 < n1 ? n1 : n0);
    return (a << 32) | b;
}

// ---- arguments ---------------------------------------------------------------------------------------------------------------------------
// twin[0 .. 3 nf): -1 on a border or the half-edge that runs the other way along the same edge, mutually.  A non-manifold edge has no
// such table.
NWA_HD bool nwa_twins_ok(const int *faces, const int *twin, long long nf)
{
    for (long long h = 0; h < 3 * nf; ++h) {
        const long long t = twin[h];
        if (t == -1) continue;
        if (t < 0 || t >= 3 * nf || t == h || twin[t] != h) return false;
        if (faces[t] != faces[nwa_next(h)] || faces[nwa_next(t)] != faces[h]) return false;
    }
    return true;
}

// a field on the host: no nan, no band beyond NWA_MAX_BAND
NWA_HD bool nwa_field_ok(const double *D, long long nv, double w)
{
    bool bad = false;
    for (long long v = 0; v < nv; ++v) (void)nwa_band(D[v], w, &bad);
    return !bad;
}

// the bounding box's lower corner and the quantum of nv >= 1 finite float32 positions; false: a position is not finite
NWA_HD bool nwa_box(const float *pos, long long nv, double *low, double *q)
{
    double hi[3];
    for (int c = 0; c < 3; ++c) { low[c] = INFINITY; hi[c] = -INFINITY; }
    for (long long i = 0; i < 3 * nv; ++i) {
        const double x = (double)pos[i];
        if (!(x - x == 0.0)) return false;
        if (x < low[i % 3]) low[i % 3] = x;
        if (x > hi[i % 3]) hi[i % 3] = x;
    }
    double e = 0.0;
    for (int c = 0; c < 3; ++c)
        if (hi[c] - low[c] > e) e = hi[c] - low[c];
    *q = nwa_quantum(e);
    return true;
}
