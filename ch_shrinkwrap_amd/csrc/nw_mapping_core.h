// The rules of mapping localizations onto a mesh (include/nw_mapping.h: nwl_map), shared by the kernels of nw_mapping.hip and by whoever
// compiles this header for the CPU (tests/test_mapping_core_cpu.py builds a shim from it with g++ -ffp-contract=off).
// tests/surface_mapping_ref.py restates the definition by brute force.  The banded closest-face walk is nw_volume_core.h's nwv_walk and
// the point-triangle arithmetic nw_distance_core.h's, included and not copied.
//
// Definition.  Everything is float64 on the float32 vertices, the order of operations is part of it, nothing may be contracted into
// an fma (compile with -ffp-contract=off).
//   1. Closest point, banded.  For a localization p and a band d_cap (finite, > 0, <= 2^40): nwv_walk(p, ..., d_cap, best) over the
//      mesh's centroid grid.  p is in band iff a face was found and nwv_in_band(best.d, d_cap) -- a face at exactly d_cap is in band.
//      The face is the smallest id among equally near faces; closest point and feature code are that face's, as nwd_query gives them.
//      Out of band: face -1, weights 0 0 0, distance +inf, closest point NaN, and nothing is accumulated.
//   2. Weights (nwl_weights): integers W[0..2] >= 0 with W0 + W1 + W2 = 2^20 exactly, from the closest point q and the feature:
//        vertex 4+k    W[k] = 2^20;
//        edge 1+k      (v_k -> v_k+1, d = v_k+1 - v_k) t = ((q - v_k).d) / (d.d) clamped to [0, 1]; W[(k+1)%3] = floor(t 2^20), W[k] the rest;
//        interior 0    n = (b-a) x (c-a); e0 = ((b-a) x (q-a)).n, e1 = ((c-b) x (q-b)).n, e2 = ((a-c) x (q-c)).n, each raised to 0 if
//                      negative; S = (e0 + e1) + e2; W_a = floor((e1 / S) 2^20), W_b = min(floor((e2 / S) 2^20), 2^20 - W_a), W_c the
//                      rest; if !(S > 0): W_a = 2^20.
//      A face of zero area never has feature 0 (nwd_point_triangle), so it needs no rule of its own.
//   3. Accumulators, all integers (added with integer atomics on the device, so the sums are a function of the input alone):
//        mass[v] (uint64) += W_k at the face's three corners; count[f] (int32) += 1;
//        per value column c <= NWL_MAX_COLUMNS with a power of two scale_c >= max |x_c|: q = (int64) rint(x / scale_c * 2^30) (both
//        scalings exact, ties to even; nwl_quantise); a non-finite x or |q| > 2^30 on an in-band localization is an error;
//        P = W_k q, |P| <= 2^50, is added in two limbs (nwl_limbs): sum_lo[v, c] += P & 0xFFFFFFFF (uint64), sum_hi[v, c] += P >> 32
//        (int64, arithmetic shift).  The column's sum is the exact integer sum_hi 2^32 + sum_lo.
//      Bound.  For at most 2^30 localizations in one set of accumulators no limb overflows: a vertex gains at most three limbs a
//      localization (a face may name it three times), so sum_lo < 3 2^30 2^32 < 2^64, |sum_hi| <= 3 2^30 2^18 < 2^63, mass <= 2^30 2^20.
//   4. Vertex areas (nwl_face_area): A_f = 0.5 sqrt(n.n); area3[v] (uint64) = the sum over the faces at v of floor(A_f 2^20); a face
//      with A_f >= 2^40 (or not finite) is refused.
//   5. Density is made from the integers by the caller: n[v] = mass / 2^20, area[v] = area3 / (3 2^20), density = 3 mass / area3,
//      mean_c[v] = (sum_hi 2^32 + sum_lo) / mass * scale_c / 2^30.
// No HIP header is needed.
#pragma once
#include "nw_volume_core.h"

#define NWL_W_SHIFT 20
#define NWL_W_ONE 1048576               // 2^20: the weights of one localization add up to it
#define NWL_Q_SHIFT 30
#define NWL_Q_ONE 1073741824.0          // 2^30: a value of +-scale
#define NWL_MAX_COLUMNS 8
#define NWL_MAX_AREA 1099511627776.0    // 2^40
#define NWL_Q_OK 0
#define NWL_Q_NONFINITE 1
#define NWL_Q_RANGE 2

// what one localization's walk leaves behind
struct nwl_hit {
    int face;                 // -1 out of band
    int32_t w[3];
    double d;                 // +inf out of band
    double c[3];              // NaN out of band
};

NWD_HD int32_t nwl_floor_w(double t) { return (int32_t)floor(t * (double)NWL_W_ONE); }       // t within [0, 1]

// one edge v -> w of the face, q on it -> the weight of w
NWD_HD int32_t nwl_edge_weight(const double *q, const float *v, const float *w)
{
    const double vx = v[0], vy = v[1], vz = v[2];
    const double dx = (double)w[0] - vx, dy = (double)w[1] - vy, dz = (double)w[2] - vz;
    const double dd = nwd_dot(dx, dy, dz, dx, dy, dz);
    double t = 0.0;
    if (dd > 0.0) t = nwd_dot(q[0] - vx, q[1] - vy, q[2] - vz, dx, dy, dz) / dd;
    if (!(t > 0.0)) t = 0.0;
    else if (t >= 1.0) t = 1.0;
    return nwl_floor_w(t);
}

// the weights of the corners a, b, c for the closest point q on feature `feature` (0..6) of the face.  W is written with constant
// indices only: nothing here asks for an array indexed at run time.
NWD_HD void nwl_weights(const double *q, const float *a, const float *b, const float *c, int feature, int32_t *W)
{
    int32_t wa = 0, wb = 0, wc = 0;
    if (feature == 4) wa = NWL_W_ONE;
    else if (feature == 5) wb = NWL_W_ONE;
    else if (feature == 6) wc = NWL_W_ONE;
    else if (feature == 1) { wb = nwl_edge_weight(q, a, b); wa = NWL_W_ONE - wb; }
    else if (feature == 2) { wc = nwl_edge_weight(q, b, c); wb = NWL_W_ONE - wc; }
    else if (feature == 3) { wa = nwl_edge_weight(q, c, a); wc = NWL_W_ONE - wa; }
    else {
        const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
        const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double wx = cx - bx, wy = cy - by, wz = cz - bz;            // edge 1: b -> c
        const double sx = ax - cx, sy = ay - cy, sz = az - cz;            // edge 2: c -> a
        double rx = q[0] - ax, ry = q[1] - ay, rz = q[2] - az;
        double e0 = nwd_dot(uy * rz - uz * ry, uz * rx - ux * rz, ux * ry - uy * rx, nx, ny, nz);
        rx = q[0] - bx; ry = q[1] - by; rz = q[2] - bz;
        double e1 = nwd_dot(wy * rz - wz * ry, wz * rx - wx * rz, wx * ry - wy * rx, nx, ny, nz);
        rx = q[0] - cx; ry = q[1] - cy; rz = q[2] - cz;
        double e2 = nwd_dot(sy * rz - sz * ry, sz * rx - sx * rz, sx * ry - sy * rx, nx, ny, nz);
        if (e0 < 0.0) e0 = 0.0;
        if (e1 < 0.0) e1 = 0.0;
        if (e2 < 0.0) e2 = 0.0;
        const double S = (e0 + e1) + e2;
        if (!(S > 0.0)) wa = NWL_W_ONE;
        else {
            wa = nwl_floor_w(e1 / S);
            wb = nwl_floor_w(e2 / S);
            if (wb > NWL_W_ONE - wa) wb = NWL_W_ONE - wa;
            wc = NWL_W_ONE - wa - wb;
        }
    }
    W[0] = wa; W[1] = wb; W[2] = wc;
}

// the walk's result as a localization's record
NWD_HD void nwl_hit_of(const nwv_best &b, double d_cap, const float *pos, const int32_t *faces, nwl_hit &h)
{
    if (b.face == INT32_MAX || !nwv_in_band(b.d, d_cap)) {
        h.face = -1; h.w[0] = h.w[1] = h.w[2] = 0; h.d = INFINITY; h.c[0] = h.c[1] = h.c[2] = NAN;
        return;
    }
    h.face = b.face; h.d = b.d; h.c[0] = b.c[0]; h.c[1] = b.c[1]; h.c[2] = b.c[2];
    const int64_t f = b.face;
    nwl_weights(b.c, pos + 3 * (int64_t)faces[3 * f], pos + 3 * (int64_t)faces[3 * f + 1], pos + 3 * (int64_t)faces[3 * f + 2], b.feature, h.w);
}

// One localization: the capped walk, the band rule and the weights -> the number of rings walked.  rho[f] must cover face f from its
// centroid and rho_max every rho[f].
NWD_HD int nwl_locate(const double *p, const float *pos, const int32_t *faces, int nf, const nwv_pt *pts, const int *cstart, const double *rho,
                      double rho_max, const nwv_grid &g, double d_cap, nwl_hit &h, int &n_centroids)
{
    nwv_best b;
    const int rings = nwv_walk(p, pos, faces, nf, pts, cstart, rho, rho_max, g, d_cap, b, n_centroids);
    nwl_hit_of(b, d_cap, pos, faces, h);
    return rings;
}

// a value as an integer in units of scale / 2^30; scale is a power of two, so both scalings are exact
NWD_HD int nwl_quantise(double x, double scale, int64_t *q)
{
    *q = 0;
    if (!(fabs(x) <= 1.79769313486231570815e308)) return NWL_Q_NONFINITE;
    const double r = rint(x / scale * NWL_Q_ONE);
    if (!(fabs(r) <= NWL_Q_ONE)) return NWL_Q_RANGE;
    *q = (int64_t)r;
    return NWL_Q_OK;
}

// P = hi 2^32 + lo with 0 <= lo < 2^32: the shift of a negative P is arithmetic
NWD_HD void nwl_limbs(int64_t P, uint64_t *lo, int64_t *hi)
{
    *lo = (uint64_t)P & 0xFFFFFFFFull;
    *hi = P >> 32;
}

// A_f = 0.5 sqrt(n.n) -> floor(A_f 2^20) and whether the face is within the limit
NWD_HD bool nwl_face_area(const float *a, const float *b, const float *c, uint64_t *area_q)
{
    const double ax = a[0], ay = a[1], az = a[2];
    const double ux = (double)b[0] - ax, uy = (double)b[1] - ay, uz = (double)b[2] - az;
    const double vx = (double)c[0] - ax, vy = (double)c[1] - ay, vz = (double)c[2] - az;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double A = 0.5 * sqrt(nwd_dot(nx, ny, nz, nx, ny, nz));
    if (!(A < NWL_MAX_AREA)) { *area_q = 0; return false; }
    *area_q = (uint64_t)floor(A * (double)NWL_W_ONE);
    return true;
}
