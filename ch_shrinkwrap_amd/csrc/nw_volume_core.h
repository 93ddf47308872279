// The rules of the banded signed-distance volume (include/nw_volume.h: nwv_volume), shared by the kernels of nw_volume.hip and by
// whoever compiles this header for the CPU (tests/test_volume_core_cpu.py builds a shim from it with g++ -ffp-contract=off).
// tests/mesh_volume_ref.py restates the definition by brute force.  The point-triangle distance, the pseudonormal and the sign are
// nw_distance_core.h's, included and not copied.
//
// Definition.  A mesh (float32 positions, int32 faces, the half-edge twin table), a lattice as nwi_density takes it -- node (i, j, k)
// lies at (double)lo[a] + ((double)index + 0.5) * (double)h along axis a, x fastest -- and a band d_cap, h <= d_cap <= 2^40.
// Per node:
//   u, face   the exact unsigned distance to the triangles and its face (nwd_point_triangle; ties go to the smallest face id);
//   in band   iff u <= d_cap (nwv_in_band);
//   in band:  sd = +-u, the sign that of the pseudonormal of the closest feature exactly as nwd_query gives it with NWD_SIGNED; a
//             distance of 0 is +0.0;
//   out of band: face = -1 and sd = +-d_cap, the sign that of the node's predecessor (nwv_predecessor): (i-1, j, k) if i > 0, else
//             (0, j-1, k) if j > 0, else (0, 0, k-1) if k > 0.  The seed (0, 0, 0) takes its sign from an exact evaluation with no cap:
//             the nearest face over all faces, then its pseudonormal.
//   field = (uint64) floor((d_cap - sd) * 2^20) (nwv_quantise), mask = sd < 0.
// Unsigned (no NWV_SIGNED): sd = min(u, d_cap), no sweep, no twin table.
//
// Why the predecessor rule is right for a closed embedded surface.  If two lattice neighbours P, Q lie on different sides, the segment
// between them crosses the surface at some X, so u(P) + u(Q) <= |P - X| + |X - Q| = h <= d_cap: both are in band and carry exact signs
// of their own.  Hence an out-of-band node lies on the same side as each of its lattice neighbours, its predecessor among them, and
// every node's predecessor path ends at the seed, whose sign is exact.  That is the reason d_cap < h is refused: with a thinner band a
// path can step over the surface without meeting an in-band node.  For an open or self-crossing mesh there are no sides: the result is
// defined by the same rules, and not meaningful (the in-band signs are as wrong there as nwd_query's).
//
// The capped walk (nwv_walk) is nwd_query's ring walk over the centroid grid with min(best, d_cap) in place of best in both bounds --
// the ring's sqrt(lbd^2 + out^2)(1 - slack) - rho_max and the face's |p - c_f|(1 - slack) - rho_f -- both compared strictly, so that a
// face at exactly d_cap is seen.  Every face within d_cap (or, if nearer, within the best) is examined, so (u, face) is exact whenever
// the node is in band; a node whose walk ends with best > d_cap is out of band.  A far node stops after ceil((d_cap + rho_max) / h_cell)
// + 1 rings.  Nothing may be contracted into an fma: compile with -ffp-contract=off.  No HIP header is needed.
#pragma once
#include "nw_distance_core.h"

#define NWV_FIELD_SHIFT 20
#define NWV_CORE_SLACK BQ_FACE_RHO_SLACK      // (nw_bq_core.h: 1e-9) relative slack of every bound: far above the rounding of a float64 distance, far below what matters

// the centroid grid as the walk reads it (the layout of the query units' shared grid in double) and a sorted centroid with its face id
struct nwv_grid {
    double lo[3], hi[3];
    double h;
    int dims[3];
};
struct nwv_pt { double x, y, z; long long i; };

struct nwv_best {
    double d2, d;             // the best squared distance and its square root
    double c[3];              // the closest point
    int face, feature;
};

// a node's coordinate along one axis
NWD_HD double nwv_node_coord(float lo, float h, int64_t index) { return (double)lo + ((double)index + 0.5) * (double)h; }

NWD_HD bool nwv_in_band(double u, double d_cap) { return u <= d_cap; }

// the linear index of the node whose sign an out-of-band node (i, j, k) takes; -1 for the seed (0, 0, 0).  It is always smaller than
// the node's own index, so one pass in index order resolves every node.
NWD_HD int64_t nwv_predecessor(int64_t i, int64_t j, int64_t k, int64_t nx, int64_t ny)
{
    if (i > 0) return (k * ny + j) * nx + (i - 1);
    if (j > 0) return (k * ny + (j - 1)) * nx;
    if (k > 0) return (k - 1) * ny * nx;
    return -1;
}

// The predecessor paths as three stages of lines, each of which only needs the stage before it: stage 0 is the z-line of (0, 0, .),
// stage 1 the y-lines of (0, ., k), stage 2 the x-rows.  Line L of a stage holds the nodes L * pitch + t * stride, t = 0 .. n-1; its
// node 0 is resolved by the stage before (the seed by its own evaluation), and the predecessor of node t > 0 is node t - 1.
NWD_HD void nwv_sweep_stage(int stage, int64_t nx, int64_t ny, int64_t nz, int64_t *n_lines, int64_t *pitch, int64_t *n, int64_t *stride)
{
    if (stage == 0) { *n_lines = 1; *pitch = 0; *n = nz; *stride = nx * ny; }
    else if (stage == 1) { *n_lines = nz; *pitch = nx * ny; *n = ny; *stride = nx; }
    else { *n_lines = ny * nz; *pitch = nx; *n = nx; *stride = 1; }
}

// the value of an out-of-band node from the resolved value of its predecessor (or, for the seed, from anything with the seed's sign)
NWD_HD double nwv_out_of_band(double d_cap, double sd_pred) { return sd_pred < 0.0 ? -d_cap : d_cap; }

// sd within [-d_cap, d_cap], d_cap <= 2^40
NWD_HD uint64_t nwv_quantise(double sd, double d_cap) { return (uint64_t)floor((d_cap - sd) * 1048576.0); }

// cell index along one axis: the expression the grid was binned with
NWD_HD int nwv_cell_1d(double x, double lo, double h, int dim)
{
    const double t = floor((x - lo) / h);
    return (int)fmin(fmax(t, 0.0), (double)(dim - 1));
}

// the faces whose centroids lie in cells [c0, c1] of one row against the node
NWD_HD void nwv_scan_cells(const nwv_pt *pts, const int *cstart, int c0, int c1, const double *q, const float *pos, const int32_t *faces,
                           const double *rho, int nf, double d_cap, nwv_best &b, int &n_centroids)
{
    const int s = cstart[c0], e = cstart[c1 + 1];
    n_centroids += e - s;
    for (int p = s; p < e; ++p) {
        const nwv_pt r = pts[p];
        const int f = (int)r.i;
        if (f < 0 || f >= nf) continue;                           // (cannot happen: the grid's points are numbered by face)
        const double ex = r.x - q[0], ey = r.y - q[1], ez = r.z - q[2];
        const double cd = sqrt((ex * ex + ey * ey) + ez * ez);
        if (cd * (1.0 - NWV_CORE_SLACK) - rho[f] > fmin(b.d, d_cap)) continue;      // the whole face is farther than the best and the band
        const int ia = faces[3 * (int64_t)f], ib = faces[3 * (int64_t)f + 1], ic = faces[3 * (int64_t)f + 2];
        double c[3];
        int feature;
        const double d2 = nwd_point_triangle(q, pos + 3 * (int64_t)ia, pos + 3 * (int64_t)ib, pos + 3 * (int64_t)ic, c, &feature);
        if (d2 < b.d2 || (d2 == b.d2 && f < b.face)) {
            b.d2 = d2; b.d = sqrt(d2); b.c[0] = c[0]; b.c[1] = c[1]; b.c[2] = c[2]; b.face = f; b.feature = feature;
        }
    }
}

// The capped walk of one node -> the number of rings walked; b.face = INT32_MAX if no face was examined.  rho[f] must cover face f
// from its centroid and rho_max every rho[f].
NWD_HD int nwv_walk(const double *q, const float *pos, const int32_t *faces, int nf, const nwv_pt *pts, const int *cstart, const double *rho,
                    double rho_max, const nwv_grid &g, double d_cap, nwv_best &b, int &n_centroids)
{
    // the node's projection onto the centroids' box: every centroid c has |c - q|^2 >= |c - q'|^2 + |q - q'|^2
    const double px = fmin(fmax(q[0], g.lo[0]), g.hi[0]), py = fmin(fmax(q[1], g.lo[1]), g.hi[1]), pz = fmin(fmax(q[2], g.lo[2]), g.hi[2]);
    const double out2 = (((q[0] - px) * (q[0] - px) + (q[1] - py) * (q[1] - py)) + (q[2] - pz) * (q[2] - pz)) * (1.0 - NWV_CORE_SLACK);
    const int cx = nwv_cell_1d(px, g.lo[0], g.h, g.dims[0]), cy = nwv_cell_1d(py, g.lo[1], g.h, g.dims[1]), cz = nwv_cell_1d(pz, g.lo[2], g.h, g.dims[2]);
    const int mx = cx > g.dims[0] - 1 - cx ? cx : g.dims[0] - 1 - cx, my = cy > g.dims[1] - 1 - cy ? cy : g.dims[1] - 1 - cy;
    const int mz = cz > g.dims[2] - 1 - cz ? cz : g.dims[2] - 1 - cz;
    const int rmax = mx > my ? (mx > mz ? mx : mz) : (my > mz ? my : mz);
    b.d2 = INFINITY; b.d = INFINITY; b.c[0] = b.c[1] = b.c[2] = 0.0; b.face = INT32_MAX; b.feature = 0;
    int r = 0;
    for (; r <= rmax; ++r) {
        // a centroid in a cell of ring r lies at least (r - 1) h from q' along one axis, and its face reaches at most rho_max towards
        // the node; the walk ends when that exceeds the best distance or the band -- strictly, so that equally near faces and a face
        // at exactly d_cap are all seen
        const double lbd = (double)(r > 1 ? r - 1 : 0) * g.h * (1.0 - NWV_CORE_SLACK);
        if (sqrt(lbd * lbd + out2) * (1.0 - NWV_CORE_SLACK) - rho_max > fmin(b.d, d_cap)) break;
        const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < g.dims[2] - 1 ? cz + r : g.dims[2] - 1;
        const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < g.dims[1] - 1 ? cy + r : g.dims[1] - 1;
        const int xa = cx - r > 0 ? cx - r : 0, xb = cx + r < g.dims[0] - 1 ? cx + r : g.dims[0] - 1;
        for (int z = z0; z <= z1; ++z) {
            for (int y = y0; y <= y1; ++y) {
                const int row = (z * g.dims[1] + y) * g.dims[0];
                if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
                    nwv_scan_cells(pts, cstart, row + xa, row + xb, q, pos, faces, rho, nf, d_cap, b, n_centroids);      // a row of the ring's shell
                } else {
                    if (cx - r >= 0) nwv_scan_cells(pts, cstart, row + cx - r, row + cx - r, q, pos, faces, rho, nf, d_cap, b, n_centroids);
                    if (cx + r < g.dims[0]) nwv_scan_cells(pts, cstart, row + cx + r, row + cx + r, q, pos, faces, rho, nf, d_cap, b, n_centroids);
                }
            }
        }
    }
    return r;
}

// What a node's walk leaves behind: *face_out = the face or -1, the return value sd before the sweep (an out-of-band node gets +d_cap,
// which the sweep may negate), *capped |= NWD_FEATURE_CAPPED if a fan walk was cut short.  twin may be NULL (unsigned).
NWD_HD double nwv_node_value(const double *q, const nwv_best &b, double d_cap, const float *pos, const int32_t *faces, const int32_t *twin,
                             int32_t *face_out, int *capped)
{
    if (b.face == INT32_MAX || !nwv_in_band(b.d, d_cap)) { *face_out = -1; return d_cap; }
    *face_out = b.face;
    double d = b.d;
    if (twin) {
        double N[3];
        *capped |= nwd_pseudonormal(pos, faces, twin, b.face, b.feature, N);
        if (b.d2 > 0.0 && nwd_sign(q, b.c, N) < 0.0) d = -d;
    }
    return d;
}
