// Hole-punch point queries on the device (MI355X, gfx950): include/nw_holepunch.h.
//
// Upstream's punch_holes (ch_shrinkwrap/_membrane_mesh.pyx:1163-1199) asks three questions of the localizations and of the candidate faces:
//   step 1  which faces have no localization within eps of their centroid      (:877-887, a cKDTree query per face)
//   step 2  which opposite candidate face is nearest "in mean-normal space"     (membrane_mesh_utils.c:1301-1376, a serial O(C^2) loop)
//   step 3  is the prism between a pair of faces empty of localizations         (:946-1016, query_ball_point + six half-plane tests)
// Here they are kernels over one cell grid of the localizations, built once per fit by the query units' shared counting sort
// (bq::bounds, bq::size_grid, bq::build_grid: nw_bq.h); the device buffer, the staging of host arrays and the context's scaffolding are
// the shared ones too.  What is this unit's own about the grid is its starting cell size and its limits (NWH_GRID_RULE).
//
//   k_hp_empty_faces  one thread per face: the rows of cells that overlap the eps-ball, first localization within eps ends the search
//                     (unless the nearest distance was asked for);
//   k_hp_pair         one row per candidate, the j > i streamed through LDS in tiles; a row's j range is cut into chunks that run in
//                     different workgroups and meet in a 64-bit atomicMin of (shift^2 bits, j): the lexicographic minimum, i.e. the
//                     first j with the smallest shift, which is what the serial loop's strict `<` keeps.  float32, no contraction
//                     (-ffp-contract=off), operation for operation as the C loop: the result is bit-identical;
//   k_hp_prism        one wave per pair: lanes walk the cells overlapping the two balls, a cell that lies beyond one of the six
//                     half-planes (or outside both balls) is passed over, the first witness ends the wave; float64.
//
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/nw_holepunch.h"
#include "nw_bq.h"

#define NWH_EXPORT extern "C" __attribute__((visibility("default")))
#define NWH_BLOCK 256
#define NWH_PAIR_CHUNK 4096         // j range of one k_hp_pair workgroup

typedef unsigned long long u64;

// ---- step 1: faces with no localization within eps of their centroid ---------------------------------------------------------------
__global__ __launch_bounds__(NWH_BLOCK) void k_hp_empty_faces(const float *__restrict__ pos, const int *__restrict__ faces, int nf, float eps,
                                                              const float4 *__restrict__ pts, const int *__restrict__ cstart, bq::Grid<float> g,
                                                              unsigned char *__restrict__ far, float *__restrict__ dist)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    // the float32 mean numpy takes over the three corners: ((p0 + p1) + p2) / 3
    const float cx = ((pos[3 * a] + pos[3 * b]) + pos[3 * c]) / 3.0f;
    const float cy = ((pos[3 * a + 1] + pos[3 * b + 1]) + pos[3 * c + 1]) / 3.0f;
    const float cz = ((pos[3 * a + 2] + pos[3 * b + 2]) + pos[3 * c + 2]) / 3.0f;
    const float eps2 = eps * eps;
    const float r = eps * (1.0f + 1e-5f) + 1e-4f;           // (cell range: a little wider than the ball, the test below is the exact one)
    const int x0 = bq::cell_1d(cx - r, g.lo[0], g.h, g.dims[0]), x1 = bq::cell_1d(cx + r, g.lo[0], g.h, g.dims[0]);
    const int y0 = bq::cell_1d(cy - r, g.lo[1], g.h, g.dims[1]), y1 = bq::cell_1d(cy + r, g.lo[1], g.h, g.dims[1]);
    const int z0 = bq::cell_1d(cz - r, g.lo[2], g.h, g.dims[2]), z1 = bq::cell_1d(cz + r, g.lo[2], g.h, g.dims[2]);
    const bool want_dist = dist != nullptr;
    float best = INFINITY;
    bool found = false;
    for (int z = z0; z <= z1 && !(found && !want_dist); ++z) {
        const float zl = g.lo[2] + z * g.h, zh = zl + g.h;
        const float dz = fmaxf(fmaxf(zl - cz, cz - zh), 0.0f);
        for (int y = y0; y <= y1; ++y) {
            const float yl = g.lo[1] + y * g.h, yh = yl + g.h;
            const float dy = fmaxf(fmaxf(yl - cy, cy - yh), 0.0f);
            // (a row of cells beyond the ball is passed over: the slack covers the rounding of the cell bounds; the outermost cells, which
            // hold what lies beyond the box, are never passed over)
            const bool outer = (z == 0 || z == g.dims[2] - 1 || y == 0 || y == g.dims[1] - 1);
            if (!outer && dy * dy + dz * dz > r * r + 1e-3f * g.h * g.h) continue;
            const int row = (z * g.dims[1] + y) * g.dims[0];
            const int s = cstart[row + x0], e = cstart[row + x1 + 1];
            for (int p = s; p < e; ++p) {
                const float4 q = pts[p];
                const float ex = q.x - cx, ey = q.y - cy, ez = q.z - cz;
                const float d2 = (ex * ex + ey * ey) + ez * ez;
                if (d2 <= eps2) {
                    found = true;
                    best = fminf(best, d2);
                    if (!want_dist) break;
                }
            }
            if (found && !want_dist) break;
        }
    }
    far[f] = found ? 0 : 1;
    if (want_dist) dist[f] = found ? fminf(sqrtf(best), eps) : eps;
}

// ---- step 2: pairing (membrane_mesh_utils.c:1301-1376), bit-identical float32 --------------------------------------------------------
// geometry of candidate k: centroid ((p0 + p1) + p2) * 0.33333334f (calculate_face_centroid: ffscalar_mult3f takes the double constant as
// a float argument) and the face normal
__global__ __launch_bounds__(NWH_BLOCK) void k_hp_cand_geom(const float *__restrict__ tri /* n x 9: p0 p1 p2 */, const float *__restrict__ nrm, int n,
                                                            float4 *__restrict__ cent, float4 *__restrict__ cnrm)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float *t = tri + 9 * (int64_t)k;
    const float third = 0.3333333333333333f;
    cent[k] = make_float4(((t[0] + t[3]) + t[6]) * third, ((t[1] + t[4]) + t[7]) * third, ((t[2] + t[5]) + t[8]) * third, 0.0f);
    cnrm[k] = make_float4(nrm[3 * (int64_t)k], nrm[3 * (int64_t)k + 1], nrm[3 * (int64_t)k + 2], 0.0f);
}

__device__ __forceinline__ float hp_dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    // ffdot3f: c = 0; c += a[i] * b[i] for i = 0, 1, 2 -- in this order, each product rounded
    float c = 0.0f;
    c += ax * bx;
    c += ay * by;
    c += az * bz;
    return c;
}

__global__ __launch_bounds__(NWH_BLOCK) void k_hp_pair(const float4 *__restrict__ cent, const float4 *__restrict__ cnrm, int n, u64 *__restrict__ key)
{
    __shared__ float4 s_c[NWH_BLOCK];
    __shared__ float4 s_n[NWH_BLOCK];
    const int row0 = blockIdx.x * NWH_BLOCK;
    const int j_begin = blockIdx.y * NWH_PAIR_CHUNK;
    const int j_end = min(n, j_begin + NWH_PAIR_CHUNK);
    if (j_end <= row0 + 1) return;                            // (every j of the chunk is <= every row of the workgroup: workgroup-uniform)
    const int i = row0 + threadIdx.x;
    const bool active = i < n;
    float4 ci = make_float4(0.f, 0.f, 0.f, 0.f), ni = ci;
    if (active) { ci = cent[i]; ni = cnrm[i]; }
    float best = 1e6f;                                        // min_shift = 1e6
    int best_j = -1;
    // (tiles before the row's first j are skipped by the whole workgroup: they are <= every row)
    for (int t0 = max(j_begin, row0 + 1) & ~(NWH_BLOCK - 1); t0 < j_end; t0 += NWH_BLOCK) {
        __syncthreads();
        const int jl = t0 + threadIdx.x;
        if (jl < j_end) { s_c[threadIdx.x] = cent[jl]; s_n[threadIdx.x] = cnrm[jl]; }
        __syncthreads();
        const int kmax = min(NWH_BLOCK, j_end - t0);
        if (!active) continue;
        for (int k = 0; k < kmax; ++k) {
            const int j = t0 + k;
            if (j <= i) continue;
            const float4 nj = s_n[k];
            const float nd = hp_dot3(ni.x, ni.y, ni.z, nj.x, nj.y, nj.z);
            // `if (nd > -0.6) continue;` compares the float in double: for a float, nd > -0.6 (double) <=> nd > -0.6f, as -0.6f < -0.6
            // and the next float up is > -0.6
            if (nd > -0.6f) continue;
            const float4 cj = s_c[k];
            const float hx = (ni.x + nj.x) * 0.5f, hy = (ni.y + nj.y) * 0.5f, hz = (ni.z + nj.z) * 0.5f;
            const float sx = ci.x - cj.x, sy = ci.y - cj.y, sz = ci.z - cj.z;
            const float ndi = hp_dot3(ni.x, ni.y, ni.z, sx, sy, sz);
            const float ndj = hp_dot3(nj.x, nj.y, nj.z, sx, sy, sz);
            if ((ndi < 0) && (ndj > 0)) continue;
            // fnorm3f: sqrt of the float sum, correctly rounded (sqrtf is lowered to the correctly rounded sequence on gfx950; __fsqrt_rn,
            // despite its name, to the bare v_sqrt_f32, which is not)
            const float snorm = sqrtf(hp_dot3(sx, sy, sz, sx, sy, sz));
            const float sdot = hp_dot3(hx, hy, hz, sx, sy, sz);
            const float m = sdot * snorm;                                           // (the |s| factor is the reference's: kept)
            const float px = sx - hx * m, py = sy - hy * m, pz = sz - hz * m;
            const float abs_shift = hp_dot3(px, py, pz, px, py, pz);
            if (abs_shift < best) { best = abs_shift; best_j = j; }                // j ascending within the row: the first j of a tie stays
        }
    }
    if (active && best_j >= 0)
        atomicMin(&key[i], ((u64)__float_as_uint(best) << 32) | (u64)(unsigned)best_j);     // (best >= 0: its bits order like the value)
}

__global__ __launch_bounds__(NWH_BLOCK) void k_hp_pair_final(const u64 *__restrict__ key, int n, int *__restrict__ pairs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    pairs[i] = (k == ~0ull) ? -1 : (int)(unsigned)(k & 0xffffffffull);
}

// ---- step 3: emptiness of the prism between two paired faces (float64, as upstream's numpy) ---------------------------------------
struct hp_d3 { double x, y, z; };
__device__ __forceinline__ hp_d3 hp_sub(hp_d3 a, hp_d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double hp_ddot(hp_d3 a, hp_d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ __forceinline__ void hp_halfplanes(const float *t, const float *nr, hp_d3 *hp, hp_d3 *anchor)
{
    // hp_k = n x e_k / |e_k| with e0 = p0 - p1 (anchor p1), e1 = p1 - p2 (anchor p2), e2 = p2 - p0 (anchor p0)  (:966-1009)
    const hp_d3 p[3] = {{t[0], t[1], t[2]}, {t[3], t[4], t[5]}, {t[6], t[7], t[8]}};
    const hp_d3 n = {nr[0], nr[1], nr[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const hp_d3 e = hp_sub(p[k], p[(k + 1) % 3]);
        const double l = sqrt(hp_ddot(e, e));
        hp[k] = {(n.y * e.z - n.z * e.y) / l, (n.z * e.x - n.x * e.z) / l, (n.x * e.y - n.y * e.x) / l};
        anchor[k] = p[(k + 1) % 3];
    }
}

// intersect [lo, hi] with the box of face t's column within `len` of its centre c (see k_hp_prism); no change if the face's geometry does
// not allow the bound (normal not a unit vector across the face's plane, a corner angle of almost nothing, non-finite values)
__device__ __forceinline__ void hp_column_box(const float *t, const float *nr, const double *c, double len, double eps, double slack, double *lo, double *hi)
{
    const hp_d3 p[3] = {{t[0], t[1], t[2]}, {t[3], t[4], t[5]}, {t[6], t[7], t[8]}};
    const hp_d3 n = {nr[0], nr[1], nr[2]};
    const hp_d3 cc = {c[0], c[1], c[2]};
    bool ok = fabs(hp_ddot(n, n) - 1.0) < 1e-3;
    double rho = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const hp_d3 u = hp_sub(p[(q + 1) % 3], p[q]), w = hp_sub(p[(q + 2) % 3], p[q]);
        const double lu = sqrt(hp_ddot(u, u)), lw = sqrt(hp_ddot(w, w));
        ok = ok && lu > 0.0 && lw > 0.0 && fabs(hp_ddot(n, u)) <= 1e-3 * lu;
        const double cosq = hp_ddot(u, w) / (lu * lw);
        const double s_half = sqrt(fmax(0.0, 0.5 * (1.0 - cosq)));
        ok = ok && s_half > 1e-3;
        const hp_d3 e = hp_sub(p[q], cc);
        rho = fmax(rho, sqrt(hp_ddot(e, e)) + eps / s_half);
    }
    if (!ok || !(rho < 1e30) || !(len < 1e30)) return;
    rho = rho * (1.0 + 1e-3) + slack;
    const double nd[3] = {n.x, n.y, n.z};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double ext = len * fabs(nd[d]) + rho * sqrt(fmax(0.0, 1.0 - nd[d] * nd[d])) + slack;
        lo[d] = fmax(lo[d], c[d] - ext);
        hi[d] = fmin(hi[d], c[d] + ext);
    }
}

__global__ __launch_bounds__(NWH_BLOCK) void k_hp_prism(const float *__restrict__ tri, const float *__restrict__ nrm, const int *__restrict__ pair_idx, int n,
                                                        double eps, const float4 *__restrict__ pts, const int *__restrict__ cstart, bq::Grid<float> g,
                                                        unsigned char *__restrict__ empty)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (NWH_BLOCK / 64) + (threadIdx.x >> 6);
    if (k >= n) return;                                       // (wave-uniform)
    const int j = pair_idx[k];
    const float *ti = tri + 9 * (int64_t)k, *tj = tri + 9 * (int64_t)j;
    // face centres as upstream: the float32 mean of the three corners, then float64
    const hp_d3 ci = {((ti[0] + ti[3]) + ti[6]) / 3.0f, ((ti[1] + ti[4]) + ti[7]) / 3.0f, ((ti[2] + ti[5]) + ti[8]) / 3.0f};
    const hp_d3 cj = {((tj[0] + tj[3]) + tj[6]) / 3.0f, ((tj[1] + tj[4]) + tj[7]) / 3.0f, ((tj[2] + tj[5]) + tj[8]) / 3.0f};
    hp_d3 hp[6], an[6];
    hp_halfplanes(ti, nrm + 3 * (int64_t)k, hp, an);
    hp_halfplanes(tj, nrm + 3 * (int64_t)j, hp + 3, an + 3);
    const hp_d3 dc = hp_sub(ci, cj);
    const double r = sqrt(hp_ddot(dc, dc)) + eps;
    const double r2 = r * r;
    const double slack = 1e-4 * (double)g.h + 1e-3;           // (cell bounds are float expressions: boxes are widened by this much)
    // cells to walk: the box of the two balls, cut down to the boxes of the two prisms' columns.  A witness lies below the three
    // half-planes of face i: its projection along n_i falls inside the triangle grown by eps, which lies within rho_i of c_i (rho = the
    // largest corner distance + eps / sin(half the corner's angle)); and it lies within r of c_i or c_j, so within |c_i - c_j| + r of c_i
    // along n_i.  A face whose normal is not a unit vector across its plane keeps the box of the balls.
    double box_lo[3], box_hi[3];
    {
        const double c0[3] = {ci.x, ci.y, ci.z}, c1[3] = {cj.x, cj.y, cj.z};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            box_lo[d] = fmin(c0[d], c1[d]) - r - slack;
            box_hi[d] = fmax(c0[d], c1[d]) + r + slack;
        }
        const double len = sqrt(hp_ddot(dc, dc)) + r;
        hp_column_box(ti, nrm + 3 * (int64_t)k, c0, len, eps, slack, box_lo, box_hi);
        hp_column_box(tj, nrm + 3 * (int64_t)j, c1, len, eps, slack, box_lo, box_hi);
    }
    int lo[3], hi[3];
    bool none = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        none |= !(box_lo[d] <= box_hi[d]);
        lo[d] = bq::cell_1d((float)box_lo[d], g.lo[d], g.h, g.dims[d]);
        hi[d] = bq::cell_1d((float)box_hi[d], g.lo[d], g.h, g.dims[d]);
    }
    if (none) {                                               // (the columns do not meet inside the balls: nothing can be a witness)
        if (lane == 0) empty[k] = 1;
        return;
    }
    const int nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
    const int64_t ncell = (int64_t)nx * ny * nz;
    bool found = false;
    for (int64_t base = 0; base < ncell; base += 64) {
        const int64_t t = base + lane;
        if (t < ncell && !found) {
            const int x = lo[0] + (int)(t % nx), y = lo[1] + (int)((t / nx) % ny), z = lo[2] + (int)(t / ((int64_t)nx * ny));
            const int ix[3] = {x, y, z};
            double bl[3], bh[3];
            bool outer = false;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                bl[d] = (double)(g.lo[d] + ix[d] * g.h) - slack;
                bh[d] = (double)(g.lo[d] + (ix[d] + 1) * g.h) + slack;
                outer |= (ix[d] == 0 || ix[d] == g.dims[d] - 1);
            }
            bool skip = false;
            if (!outer) {                                     // (the outermost cells hold what lies beyond the box: never passed over)
                // outside both balls?
                double d0 = 0.0, d1 = 0.0;
                const double c0[3] = {ci.x, ci.y, ci.z}, c1[3] = {cj.x, cj.y, cj.z};
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const double e0 = fmax(fmax(bl[d] - c0[d], c0[d] - bh[d]), 0.0), e1 = fmax(fmax(bl[d] - c1[d], c1[d] - bh[d]), 0.0);
                    d0 += e0 * e0; d1 += e1 * e1;
                }
                skip = d0 > r2 && d1 > r2;
                // beyond one of the six half-planes? (min over the box of hp . (x - p) >= eps; a NaN plane passes nothing over)
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const double mx = 0.5 * (bl[0] + bh[0]), my = 0.5 * (bl[1] + bh[1]), mz = 0.5 * (bl[2] + bh[2]);
                    const double lo_q = hp[q].x * (mx - an[q].x) + hp[q].y * (my - an[q].y) + hp[q].z * (mz - an[q].z)
                                      - 0.5 * (fabs(hp[q].x) * (bh[0] - bl[0]) + fabs(hp[q].y) * (bh[1] - bl[1]) + fabs(hp[q].z) * (bh[2] - bl[2]));
                    skip |= lo_q > eps + 1e-9;
                }
            }
            if (!skip) {
                const int cell = (z * g.dims[1] + y) * g.dims[0] + x;
                const int s = cstart[cell], e = cstart[cell + 1];
                for (int p = s; p < e; ++p) {
                    const float4 q = pts[p];
                    const hp_d3 xq = {q.x, q.y, q.z};
                    const hp_d3 u = hp_sub(xq, ci), v = hp_sub(xq, cj);
                    if (!(hp_ddot(u, u) <= r2 || hp_ddot(v, v) <= r2)) continue;
                    bool below = true;
#pragma unroll
                    for (int w = 0; w < 6; ++w) below = below && (hp_ddot(hp[w], hp_sub(xq, an[w])) < eps);
                    if (below) { found = true; break; }
                }
            }
        }
        if (__ballot(found) != 0ull) { found = true; break; }  // (a witness anywhere in the wave ends the pair)
    }
    if (lane == 0) empty[k] = found ? 0 : 1;
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwh_ctx : bq::Ctx {
    // the grid of the localizations (nwh_set_points)
    int n_points = 0;
    bq::Grid<float> grid{};
    DevBuf pts, cstart;
    // per call
    DevBuf a, b, c, d, e, f;
};

namespace {

#define NWH_HIP(call) BQ_HIP(call, NWH_ERR_NOMEM, NWH_ERR_HIP)

// at most max(4 n, 65536) cells, up to 2^30; at most 2048 an axis; 200 widening steps
const bq::GridRule NWH_GRID_RULE = {4, 1ll << 30, 2048, 200};

int check_cands(const int32_t *cands, int64_t nc, int64_t nf)
{
    if (!cands || nc < 1 || nc > (1ll << 30)) return NWH_ERR_BADARG;
    for (int64_t i = 0; i < nc; ++i)
        if (cands[i] < 0 || cands[i] >= nf) return NWH_ERR_BADARG;
    return NWH_OK;
}

// the candidates' corners (p0 p1 p2 = faces[f, 0..2]) and normals, gathered on the host: C is small next to the mesh
void gather(const float *pos, const int32_t *faces, const float *fn, const int32_t *cands, int64_t nc, std::vector<float> &tri, std::vector<float> &nrm)
{
    tri.resize(9 * nc);
    nrm.resize(3 * nc);
    for (int64_t k = 0; k < nc; ++k) {
        const int64_t f = cands[k];
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d) tri[9 * k + 3 * c + d] = pos[3 * (int64_t)faces[3 * f + c] + d];
        for (int d = 0; d < 3; ++d) nrm[3 * k + d] = fn[3 * f + d];
    }
}

}  // namespace

NWH_EXPORT int nwh_abi_version(void) { return NWH_ABI_VERSION; }

NWH_EXPORT int nwh_create(int device, nwh_ctx **out) { return bq::create(device, out, NWH_ERR_BADARG, NWH_ERR_HIP); }

NWH_EXPORT void nwh_destroy(nwh_ctx *ctx) { bq::destroy(ctx); }

NWH_EXPORT const char *nwh_last_error(nwh_ctx *ctx) { return bq::last_error(ctx); }

NWH_EXPORT int nwh_set_points(nwh_ctx *ctx, const float *xyz, int64_t n_points, float cell_size)
{
    if (!xyz || n_points < 1 || n_points > (1ll << 30) || !std::isfinite(cell_size)) return NWH_ERR_BADARG;
    if (!ctx) return NWH_ERR_BADARG;
    NWH_HIP(hipSetDevice(ctx->device));
    const int n = (int)n_points;
    ctx->n_points = 0;
    // a device pointer is read in place, a host one is copied first
    const float *src = xyz;
    if (!bq::on_device(xyz)) {
        NWH_HIP(bq::upload(ctx->stream, ctx->a, xyz, 3 * (int64_t)n));
        src = ctx->a.as<float>();
    }
    bq::Grid<float> g;
    bool finite[2];
    NWH_HIP(bq::bounds<float>(ctx->stream, ctx->b, src, n, nullptr, 0, &g, finite));
    if (!finite[0]) return fail(ctx, NWH_ERR_NONFINITE, "nwh_set_points: a localization is not finite");
    double ext[3];                                            // (float differences)
    float emax = 0.0f;
    for (int d = 0; d < 3; ++d) { const float e = g.hi[d] - g.lo[d]; ext[d] = e; emax = std::max(emax, e); }
    emax = std::max(emax, 1e-3f);
    // cell size: the caller's, or about one localization per cell of the box (the flattest axis counts as a thousandth of the widest);
    // then widened until the grid is within NWH_GRID_RULE
    double h = cell_size > 0 ? (double)cell_size
                             : std::cbrt(std::max(ext[0], 1e-3 * emax) * std::max(ext[1], 1e-3 * emax) * std::max(ext[2], 1e-3 * emax) / n);
    h = std::max(h, (double)emax / 2048.0);
    if (!bq::size_grid(NWH_GRID_RULE, n, ext, &h, g.dims)) return fail(ctx, NWH_ERR_BADARG, "nwh_set_points: no cell size keeps the grid within its cap");
    g.h = (float)h;
    int total = -1;
    NWH_HIP(bq::build_grid<float>(ctx->stream, src, n, g, ctx->c, ctx->d, ctx->e, ctx->cstart, ctx->pts, &total));
    if (total != n) return fail(ctx, NWH_ERR_HIP, "nwh_set_points: the cell counts do not add up to the localizations");
    ctx->grid = g;
    ctx->n_points = n;
    return NWH_OK;
}

NWH_EXPORT int nwh_empty_faces(nwh_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, float eps,
                               uint8_t *far, float *dist)
{
    if (!far || !(eps > 0.0f) || !std::isfinite(eps)) return NWH_ERR_BADARG;
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return NWH_ERR_BADARG;
    if (!ctx) return NWH_ERR_BADARG;
    if (ctx->n_points < 1) return fail(ctx, NWH_ERR_NOPOINTS, "nwh_empty_faces: nwh_set_points first");
    NWH_HIP(hipSetDevice(ctx->device));
    const int nf = (int)n_faces;
    NWH_HIP(bq::upload(ctx->stream, ctx->a, pos, 3 * n_vertices));
    NWH_HIP(bq::upload(ctx->stream, ctx->b, faces, 3 * n_faces));
    NWH_HIP(ctx->c.ensure((size_t)nf));
    if (dist) NWH_HIP(ctx->f.ensure(sizeof(float) * (size_t)nf));
    hipLaunchKernelGGL(k_hp_empty_faces, dim3(nblk(nf)), dim3(NWH_BLOCK), 0, ctx->stream, ctx->a.as<float>(), ctx->b.as<int>(), nf, eps,
                       ctx->pts.as<float4>(), ctx->cstart.as<int>(), ctx->grid, ctx->c.as<unsigned char>(), dist ? ctx->f.as<float>() : nullptr);
    NWH_HIP(hipGetLastError());
    NWH_HIP(hipMemcpyAsync(far, ctx->c.p, (size_t)nf, hipMemcpyDeviceToHost, ctx->stream));
    if (dist) NWH_HIP(hipMemcpyAsync(dist, ctx->f.p, sizeof(float) * (size_t)nf, hipMemcpyDeviceToHost, ctx->stream));
    NWH_HIP(hipStreamSynchronize(ctx->stream));
    return NWH_OK;
}

NWH_EXPORT int nwh_pair_faces(nwh_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const float *face_normals,
                              const int32_t *cands, int64_t n_cands, int32_t *pairs)
{
    if (!face_normals || !pairs) return NWH_ERR_BADARG;
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return NWH_ERR_BADARG;
    const int r = check_cands(cands, n_cands, n_faces);
    if (r != NWH_OK) return r;
    if (!ctx) return NWH_ERR_BADARG;
    NWH_HIP(hipSetDevice(ctx->device));
    const int nc = (int)n_cands;
    std::vector<float> tri, nrm;
    gather(pos, faces, face_normals, cands, nc, tri, nrm);
    NWH_HIP(bq::upload(ctx->stream, ctx->a, tri.data(), (int64_t)tri.size()));
    NWH_HIP(bq::upload(ctx->stream, ctx->b, nrm.data(), (int64_t)nrm.size()));
    NWH_HIP(ctx->c.ensure(sizeof(float4) * (size_t)nc));
    NWH_HIP(ctx->d.ensure(sizeof(float4) * (size_t)nc));
    NWH_HIP(ctx->e.ensure(sizeof(u64) * (size_t)nc));
    NWH_HIP(ctx->f.ensure(sizeof(int) * (size_t)nc));
    NWH_HIP(hipMemsetAsync(ctx->e.p, 0xff, sizeof(u64) * (size_t)nc, ctx->stream));
    hipLaunchKernelGGL(k_hp_cand_geom, dim3(nblk(nc)), dim3(NWH_BLOCK), 0, ctx->stream, ctx->a.as<float>(), ctx->b.as<float>(), nc, ctx->c.as<float4>(), ctx->d.as<float4>());
    const dim3 grid(nblk(nc), (unsigned)((nc + NWH_PAIR_CHUNK - 1) / NWH_PAIR_CHUNK));
    hipLaunchKernelGGL(k_hp_pair, grid, dim3(NWH_BLOCK), 0, ctx->stream, ctx->c.as<float4>(), ctx->d.as<float4>(), nc, ctx->e.as<u64>());
    hipLaunchKernelGGL(k_hp_pair_final, dim3(nblk(nc)), dim3(NWH_BLOCK), 0, ctx->stream, ctx->e.as<u64>(), nc, ctx->f.as<int>());
    NWH_HIP(hipGetLastError());
    NWH_HIP(hipMemcpyAsync(pairs, ctx->f.p, sizeof(int) * (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
    NWH_HIP(hipStreamSynchronize(ctx->stream));
    return NWH_OK;
}

NWH_EXPORT int nwh_prism_empty(nwh_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const float *face_normals,
                               const int32_t *cands, const int32_t *pair_idx, int64_t n, float eps, uint8_t *empty)
{
    if (!face_normals || !pair_idx || !empty || !(eps > 0.0f) || !std::isfinite(eps)) return NWH_ERR_BADARG;
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return NWH_ERR_BADARG;
    const int r = check_cands(cands, n, n_faces);
    if (r != NWH_OK) return r;
    for (int64_t k = 0; k < n; ++k)
        if (pair_idx[k] < 0 || pair_idx[k] >= n) return NWH_ERR_BADARG;
    if (!ctx) return NWH_ERR_BADARG;
    if (ctx->n_points < 1) return fail(ctx, NWH_ERR_NOPOINTS, "nwh_prism_empty: nwh_set_points first");
    NWH_HIP(hipSetDevice(ctx->device));
    const int nc = (int)n;
    std::vector<float> tri, nrm;
    gather(pos, faces, face_normals, cands, nc, tri, nrm);
    NWH_HIP(bq::upload(ctx->stream, ctx->a, tri.data(), (int64_t)tri.size()));
    NWH_HIP(bq::upload(ctx->stream, ctx->b, nrm.data(), (int64_t)nrm.size()));
    NWH_HIP(bq::upload(ctx->stream, ctx->c, pair_idx, n));
    NWH_HIP(ctx->f.ensure((size_t)nc));
    hipLaunchKernelGGL(k_hp_prism, dim3(nblk(nc, NWH_BLOCK / 64)), dim3(NWH_BLOCK), 0, ctx->stream, ctx->a.as<float>(), ctx->b.as<float>(), ctx->c.as<int>(), nc,
                       (double)eps, ctx->pts.as<float4>(), ctx->cstart.as<int>(), ctx->grid, ctx->f.as<unsigned char>());
    NWH_HIP(hipGetLastError());
    NWH_HIP(hipMemcpyAsync(empty, ctx->f.p, (size_t)nc, hipMemcpyDeviceToHost, ctx->stream));
    NWH_HIP(hipStreamSynchronize(ctx->stream));
    return NWH_OK;
}
