// The arithmetic of the point-to-mesh distance (include/nw_distance.h: nwd_query), shared by the kernels of nw_distance.hip and by
// whoever compiles this header for the CPU (tests/test_distance_core_cpu.py builds a shim from it with g++ -ffp-contract=off).
// tests/mesh_distance_ref.py restates it in NumPy, operation for operation.
//
// Everything is float64 on the float32 vertex positions widened to double, and the order of operations is part of the definition:
//   - a sum of three is (x + y) + z, a dot product (u0 v0 + u1 v1) + u2 v2, a cross product rounds each product and subtracts;
//   - nothing may be contracted into an fma: compile with -ffp-contract=off;
//   - division and square root are the correctly rounded ones.
//
// Point and triangle (a, b, c = the corners faces[f][0..2]); the candidates in this order, a later one replacing the best only when it
// is strictly nearer:
//   plane   n = (b - a) x (c - a), nn = n.n; only if nn > 0: t = ((p - a).n) / nn, q = p - t n, and the three edge functions
//           w_k = ((v_k+1 - v_k) x (q - v_k)).n must be >= 0; d2 = |p - q|^2; feature 0
//   edge k  (half-edge 3f+k, v_k -> v_k+1, k = 0, 1, 2): d = v_k+1 - v_k, dd = d.d, t = dd > 0 ? ((p - v_k).d) / dd : 0;
//           t <= 0: the closest point is v_k itself (feature 4 + k); t >= 1: v_k+1 itself (feature 4 + (k+1) % 3); else v_k + t d
//           (feature 1 + k); d2 = |p - closest|^2
// A face of zero area is its three segments.  A query at a vertex gets d2 = 0 exactly, because segment ends are the corners themselves.
//
// Pseudonormal of the closest feature (Baerentzen & Aanaes 2005), from unit face normals n / sqrt(nn); faces of zero area add nothing:
//   interior  the face's unit normal
//   edge k    the face's plus that of the face across twin[3f+k] (the face alone on a border, twin = -1)
//   vertex k  the sum over the fan around faces[f][k] of corner angle x unit normal, the angle atan2(|u x w|, u.w) of the two edges
//             leaving the corner.  The fan is walked from half-edge h0 = 3f+k by h -> twin[prev(h)] until it returns to h0; if it
//             meets a border first, it is then walked the other way from h0 by h -> next(twin[h]) until the other border.  At most
//             NWD_FAN_CAP faces are visited; a walk that is cut short sets NWD_FEATURE_CAPPED in the feature code.
// sign = -1 where (p - closest).N < 0, else +1: negative inside a closed mesh whose faces wind counter-clockwise seen from outside.
// No HIP header is needed: without a HIP compiler NWD_HD is plain `inline`.
#pragma once
#include <cmath>
#include <cstdint>

#include "nw_bq_core.h"

#if defined(__HIPCC__)
#define NWD_HD __host__ __device__ __forceinline__
#else
#define NWD_HD inline
#endif

#define NWD_FAN_CAP 256
#define NWD_FEATURE_MASK 7
#define NWD_FEATURE_CAPPED 8

NWD_HD double nwd_dot(double u0, double u1, double u2, double v0, double v1, double v2) { return (u0 * v0 + u1 * v1) + u2 * v2; }

// one clamped segment v -> w against the best so far; `fe`, `f0`, `f1`: the feature codes of its inside and of its two ends
NWD_HD void nwd_segment(double px, double py, double pz, double vx, double vy, double vz, double wx, double wy, double wz, int fe, int f0, int f1,
                        double &best, double &cx, double &cy, double &cz, int &feature)
{
    const double dx = wx - vx, dy = wy - vy, dz = wz - vz;
    const double dd = nwd_dot(dx, dy, dz, dx, dy, dz);
    double t = 0.0;
    if (dd > 0.0) t = nwd_dot(px - vx, py - vy, pz - vz, dx, dy, dz) / dd;
    double qx, qy, qz;
    int code;
    if (!(t > 0.0)) { qx = vx; qy = vy; qz = vz; code = f0; }
    else if (t >= 1.0) { qx = wx; qy = wy; qz = wz; code = f1; }
    else { qx = vx + t * dx; qy = vy + t * dy; qz = vz + t * dz; code = fe; }
    const double ex = px - qx, ey = py - qy, ez = pz - qz;
    const double d2 = nwd_dot(ex, ey, ez, ex, ey, ez);
    if (d2 < best) { best = d2; cx = qx; cy = qy; cz = qz; feature = code; }
}

// squared distance of p from the triangle a b c (float32 corners), its closest point and the feature code 0..6
NWD_HD double nwd_point_triangle(const double *p, const float *a, const float *b, const float *c, double *closest, int *feature_out)
{
    const double px = p[0], py = p[1], pz = p[2];
    const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2], cx = c[0], cy = c[1], cz = c[2];
    double best = INFINITY, qx = ax, qy = ay, qz = az;
    int feature = 4;
    const double ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double nn = nwd_dot(nx, ny, nz, nx, ny, nz);
    if (nn > 0.0) {
        const double t = nwd_dot(px - ax, py - ay, pz - az, nx, ny, nz) / nn;
        const double hx = px - t * nx, hy = py - t * ny, hz = pz - t * nz;
        // edge function k: ((v_k+1 - v_k) x (h - v_k)) . n
        const double wx = cx - bx, wy = cy - by, wz = cz - bz;            // edge 1: b -> c
        const double sx = ax - cx, sy = ay - cy, sz = az - cz;            // edge 2: c -> a
        double rx = hx - ax, ry = hy - ay, rz = hz - az;
        const double w0 = nwd_dot(uy * rz - uz * ry, uz * rx - ux * rz, ux * ry - uy * rx, nx, ny, nz);
        rx = hx - bx; ry = hy - by; rz = hz - bz;
        const double w1 = nwd_dot(wy * rz - wz * ry, wz * rx - wx * rz, wx * ry - wy * rx, nx, ny, nz);
        rx = hx - cx; ry = hy - cy; rz = hz - cz;
        const double w2 = nwd_dot(sy * rz - sz * ry, sz * rx - sx * rz, sx * ry - sy * rx, nx, ny, nz);
        if (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) {
            const double ex = px - hx, ey = py - hy, ez = pz - hz;
            best = nwd_dot(ex, ey, ez, ex, ey, ez);
            qx = hx; qy = hy; qz = hz;
            feature = 0;
        }
    }
    nwd_segment(px, py, pz, ax, ay, az, bx, by, bz, 1, 4, 5, best, qx, qy, qz, feature);
    nwd_segment(px, py, pz, bx, by, bz, cx, cy, cz, 2, 5, 6, best, qx, qy, qz, feature);
    nwd_segment(px, py, pz, cx, cy, cz, ax, ay, az, 3, 6, 4, best, qx, qy, qz, feature);
    closest[0] = qx; closest[1] = qy; closest[2] = qz;
    *feature_out = feature;
    return best;
}

// N += weight x the unit normal of face g, where the weight is 1 (corner < 0) or the angle at corner `corner` of the face
NWD_HD void nwd_add_face_normal(const float *pos, const int32_t *faces, int g, int corner, double *N)
{
    const int k = corner < 0 ? 0 : corner;
    const float *a = pos + 3 * (int64_t)faces[3 * (int64_t)g + k];
    const float *b = pos + 3 * (int64_t)faces[3 * (int64_t)g + (k + 1) % 3];
    const float *c = pos + 3 * (int64_t)faces[3 * (int64_t)g + (k + 2) % 3];
    const double ax = a[0], ay = a[1], az = a[2];
    const double ux = (double)b[0] - ax, uy = (double)b[1] - ay, uz = (double)b[2] - az;
    const double vx = (double)c[0] - ax, vy = (double)c[1] - ay, vz = (double)c[2] - az;
    // (the cross product of the two edges leaving any corner of a face is the face's normal, in exact arithmetic; the corner in use
    // is part of the definition)
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double nn = nwd_dot(nx, ny, nz, nx, ny, nz);
    if (!(nn > 0.0)) return;
    const double len = sqrt(nn);
    const double w = corner < 0 ? 1.0 : atan2(len, nwd_dot(ux, uy, uz, vx, vy, vz));
    N[0] = N[0] + w * (nx / len);
    N[1] = N[1] + w * (ny / len);
    N[2] = N[2] + w * (nz / len);
}

// the pseudonormal of feature `feature` (0..6) of face f -> N; returns 0, or NWD_FEATURE_CAPPED if the fan walk was cut short.
// twin[3F]: -1 on a border; every other entry in range and an involution (nwd_set_mesh checks it).
NWD_HD int nwd_pseudonormal(const float *pos, const int32_t *faces, const int32_t *twin, int f, int feature, double *N)
{
    N[0] = N[1] = N[2] = 0.0;
    if (feature == 0) {
        nwd_add_face_normal(pos, faces, f, -1, N);
        return 0;
    }
    if (feature <= 3) {
        nwd_add_face_normal(pos, faces, f, -1, N);
        const int t = twin[3 * (int64_t)f + (feature - 1)];
        if (t >= 0) nwd_add_face_normal(pos, faces, t / 3, -1, N);
        return 0;
    }
    const int h0 = 3 * f + (feature - 4);
    int h = h0, steps = 0;
    bool border = false;
    for (;;) {
        nwd_add_face_normal(pos, faces, h / 3, h % 3, N);
        ++steps;
        const int t = twin[3 * (h / 3) + (h % 3 + 2) % 3];         // across prev(h): the next outgoing half-edge of the vertex
        if (t < 0) { border = true; break; }
        if (t == h0) return 0;
        if (steps >= NWD_FAN_CAP) return NWD_FEATURE_CAPPED;
        h = t;
    }
    h = h0;
    while (border) {
        const int t = twin[h];
        if (t < 0) break;
        h = 3 * (t / 3) + (t % 3 + 1) % 3;                         // next(twin[h]): the outgoing half-edge on the other side
        if (h == h0) break;
        if (steps >= NWD_FAN_CAP) return NWD_FEATURE_CAPPED;
        nwd_add_face_normal(pos, faces, h / 3, h % 3, N);
        ++steps;
    }
    return 0;
}

// -1 where (p - closest) . N < 0, else +1
NWD_HD double nwd_sign(const double *p, const double *closest, const double *N)
{
    return nwd_dot(p[0] - closest[0], p[1] - closest[1], p[2] - closest[2], N[0], N[1], N[2]) < 0.0 ? -1.0 : 1.0;
}

// the centroid of a face in float64 and rho, the largest distance from it to a corner: the face grid's (nw_bq_core.h)
NWD_HD double nwd_face_centroid(const float *a, const float *b, const float *c, double *cen) { return bq::face_centroid(a, b, c, cen); }
