// The arithmetic of the self-intersection check (include/nw_intersections.h: nwx_find), shared by the kernels of nw_intersections.hip and
// by whoever compiles this header for the CPU (tests/test_intersections_core_cpu.py builds a shim from it with g++ -ffp-contract=off).
// tests/mesh_intersections_ref.py restates it in NumPy, operation for operation.
//
// Everything is float64 on the float32 vertex positions widened to double, and the order of operations is part of the definition
// (nw_distance_core.h's):
//   - a difference u - v is taken per axis; a dot product is (u0 v0 + u1 v1) + u2 v2; a cross product rounds each product and subtracts:
//     (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0);
//   - nothing may be contracted into an fma: compile with -ffp-contract=off.
//
// What is reported are PROPER CROSSINGS: the interior of an edge of one face passes through the interior of the other face.  Touching
// (a corner or an edge of one face lying on the other), coplanar overlap and faces that share an edge are not crossings.
//
// Flat faces.  For a face a b c (the corners faces[f][0..2]): n = (b - a) x (c - a), nn = n.n.  A face with !(nn > 0) is flat (a repeated
// vertex id makes n exactly zero); it neither crosses nor is crossed.
//
// seg_tri(p, q; a, b, c) is true when both hold:
//   - sp = n.(p - a) and sq = n.(q - a) have strictly opposite signs: (sp > 0 and sq < 0) or (sp < 0 and sq > 0);
//   - with d = q - p, the three values ((a - p) x (b - p)).d, ((b - p) x (c - p)).d, ((c - p) x (a - p)).d are all > 0 or all < 0.
//
// A pair of faces is always evaluated as A = the smaller face id, B = the larger, so the answer is one bit per unordered pair whichever
// thread computes it.  s = the number of corner pairs (one corner of A, one of B) with equal VERTEX IDS (positions are never compared):
//   s = 0   plane rejection first: n_A.(B_k - A_0), k = 0..2, must contain a value > 0 and a value < 0, and so must n_B.(A_k - B_0)
//           (in exact arithmetic the six tests imply it; in rounded arithmetic it keeps a face that touches the other's plane from one
//           side out of the tests whose triple products are then rounding noise).  Then the OR of six tests: A's edges k -> k+1 against
//           B (k = 0, 1, 2), then B's edges k -> k+1 against A.
//   s = 1   the edge of A opposite its shared corner k (corners k+1 -> k+2) against B, OR the edge of B opposite its shared corner
//           against A.  No plane rejection.  The corners are picked with selects, never from an array indexed at run time.
//   s >= 2  the pair is not examined (faces that share an edge, or a face with a repeated vertex: the remesher's fold test owns those).
//
// The centroid of a face and rho, the largest distance from it to a corner, are nw_bq_core.h's: ((a + b) + c) / 3 per axis, then
// the square root of the largest of the three squared distances.  Two faces can only meet if |c_f - c_g| <= rho_f + rho_g.
// No HIP header is needed: without a HIP compiler NWX_HD is plain `inline`.
#pragma once
#include <cmath>
#include <cstdint>

#include "nw_bq_core.h"

#if defined(__HIPCC__)
#define NWX_HD __host__ __device__ __forceinline__
#else
#define NWX_HD inline
#endif

struct nwx_v3 { double x, y, z; };
struct nwx_tri { int i0, i1, i2; nwx_v3 a, b, c; };           // the three vertex ids and the three corners of a face

NWX_HD nwx_v3 nwx_sub(const nwx_v3 &u, const nwx_v3 &v) { return nwx_v3{u.x - v.x, u.y - v.y, u.z - v.z}; }
NWX_HD double nwx_dot(const nwx_v3 &u, const nwx_v3 &v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
NWX_HD nwx_v3 nwx_cross(const nwx_v3 &u, const nwx_v3 &v) { return nwx_v3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
NWX_HD nwx_v3 nwx_widen(const float *p) { return nwx_v3{(double)p[0], (double)p[1], (double)p[2]}; }

NWX_HD nwx_tri nwx_load(const float *pos, const int32_t *faces, int64_t f)
{
    nwx_tri t;
    t.i0 = faces[3 * f]; t.i1 = faces[3 * f + 1]; t.i2 = faces[3 * f + 2];
    t.a = nwx_widen(pos + 3 * (int64_t)t.i0); t.b = nwx_widen(pos + 3 * (int64_t)t.i1); t.c = nwx_widen(pos + 3 * (int64_t)t.i2);
    return t;
}

NWX_HD nwx_v3 nwx_normal(const nwx_tri &t) { return nwx_cross(nwx_sub(t.b, t.a), nwx_sub(t.c, t.a)); }

// whether x and y have strictly opposite signs
NWX_HD bool nwx_opposite(double x, double y) { return (x > 0.0 && y < 0.0) || (x < 0.0 && y > 0.0); }

// the segment p -> q against the face t with normal n = nwx_normal(t)
NWX_HD bool nwx_seg_tri(const nwx_v3 &p, const nwx_v3 &q, const nwx_tri &t, const nwx_v3 &n)
{
    const double sp = nwx_dot(n, nwx_sub(p, t.a)), sq = nwx_dot(n, nwx_sub(q, t.a));
    // (no early return and no || between the tests of a pair: on the device they run without a branch between them)
    const nwx_v3 d = nwx_sub(q, p), ea = nwx_sub(t.a, p), eb = nwx_sub(t.b, p), ec = nwx_sub(t.c, p);
    const double w0 = nwx_dot(nwx_cross(ea, eb), d), w1 = nwx_dot(nwx_cross(eb, ec), d), w2 = nwx_dot(nwx_cross(ec, ea), d);
    return nwx_opposite(sp, sq) && ((w0 > 0.0 && w1 > 0.0 && w2 > 0.0) || (w0 < 0.0 && w1 < 0.0 && w2 < 0.0));
}

// whether x, y, z contain a value > 0 and a value < 0
NWX_HD bool nwx_straddles(double x, double y, double z) { return (x > 0.0 || y > 0.0 || z > 0.0) && (x < 0.0 || y < 0.0 || z < 0.0); }

// the pair's bit; A must be the face with the smaller id
NWX_HD bool nwx_pair(const nwx_tri &A, const nwx_tri &B)
{
    const nwx_v3 nA = nwx_normal(A), nB = nwx_normal(B);
    if (!(nwx_dot(nA, nA) > 0.0) || !(nwx_dot(nB, nB) > 0.0)) return false;
    const bool a0 = A.i0 == B.i0 || A.i0 == B.i1 || A.i0 == B.i2, a1 = A.i1 == B.i0 || A.i1 == B.i1 || A.i1 == B.i2;
    const bool b0 = B.i0 == A.i0 || B.i0 == A.i1 || B.i0 == A.i2, b1 = B.i1 == A.i0 || B.i1 == A.i1 || B.i1 == A.i2;
    const int s = ((A.i0 == B.i0) + (A.i0 == B.i1) + (A.i0 == B.i2)) + ((A.i1 == B.i0) + (A.i1 == B.i1) + (A.i1 == B.i2)) +
                  ((A.i2 == B.i0) + (A.i2 == B.i1) + (A.i2 == B.i2));
    if (s >= 2) return false;
    if (s == 1) {
        // corner k of A is shared (the third if neither of the first two is): its opposite edge runs k+1 -> k+2
        const nwx_v3 pa = a0 ? A.b : a1 ? A.c : A.a, qa = a0 ? A.c : a1 ? A.a : A.b;
        const nwx_v3 pb = b0 ? B.b : b1 ? B.c : B.a, qb = b0 ? B.c : b1 ? B.a : B.b;
        return ((int)nwx_seg_tri(pa, qa, B, nB) | (int)nwx_seg_tri(pb, qb, A, nA)) != 0;
    }
    if (!nwx_straddles(nwx_dot(nA, nwx_sub(B.a, A.a)), nwx_dot(nA, nwx_sub(B.b, A.a)), nwx_dot(nA, nwx_sub(B.c, A.a)))) return false;
    if (!nwx_straddles(nwx_dot(nB, nwx_sub(A.a, B.a)), nwx_dot(nB, nwx_sub(A.b, B.a)), nwx_dot(nB, nwx_sub(A.c, B.a)))) return false;
    return ((int)nwx_seg_tri(A.a, A.b, B, nB) | (int)nwx_seg_tri(A.b, A.c, B, nB) | (int)nwx_seg_tri(A.c, A.a, B, nB) |
            (int)nwx_seg_tri(B.a, B.b, A, nA) | (int)nwx_seg_tri(B.b, B.c, A, nA) | (int)nwx_seg_tri(B.c, B.a, A, nA)) != 0;
}

// the centroid of a face in float64 and rho, the largest distance from it to a corner: the face grid's (nw_bq_core.h), on the corners
// that nwx_load has widened
NWX_HD double nwx_face_centroid(const nwx_tri &t, nwx_v3 *cen)
{
    const double a[3] = {t.a.x, t.a.y, t.a.z}, b[3] = {t.b.x, t.b.y, t.b.z}, c[3] = {t.c.x, t.c.y, t.c.z};
    double m[3];
    const double rho = bq::face_centroid(a, b, c, m);
    *cen = nwx_v3{m[0], m[1], m[2]};
    return rho;
}
