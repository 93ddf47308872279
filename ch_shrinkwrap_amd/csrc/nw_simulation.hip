// The SMLM cloud simulator on the device (MI355X, gfx950): include/nw_simulation.h.
//
// Upstream's evaluation recipe starts with PointcloudFromShape (recipe_modules/simulation.py:11-61): points on a CSG shape's surface
// (shape.py:57-86), a localization error per point and axis (util.py:37-47), clusters of repeated blinks and a uniform background
// (evaluation_utils.py:182-282), all NumPy on the host.  Here:
//
//   shape           sim_eval            the postfix program of nwg_op, one thread per point; the program is wave-uniform (read through scalar
//                                       loads, every branch of the interpreter uniform) and the value stack is eight named doubles that shift
//                                       on push and pop, so nothing is indexed dynamically and nothing goes to scratch
//                   k_sim_eval, k_sim_normals
//   surface lattice k_sim_cell_test     one thread per cell of a level: the program at the cell's centre against the level's bound
//                   (scan)              slots of the kept cells
//                   k_sim_cell_split    a kept cell's eight children, in Morton order: the list stays sorted by Morton code
//                   k_sim_leaf_test     one thread per candidate node: inside the cube, the shell test, the thinning draw
//                   (scan)              output slots
//                   k_sim_leaf_emit     key and lattice position of every detected node: ascending key by construction
//                   k_sim_project       Newton steps onto the zero level set
//   model           k_sim_loc_error, k_sim_displace, k_sim_background     one thread per point, three axes
//   clusters        k_sim_copy_hist     radix select of the sz-th smallest copy key, a byte per pass; the keys are recomputed, never stored
//                   k_sim_copy_equal, (scan), k_sim_copy_keep, (scan), k_sim_copy_emit
//
// The scan, the host loop and the bin rule of the radix select, the device buffer with its staging, the finiteness check of a host array
// and the context's scaffolding are the query units' shared ones (nw_bq.h).
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <climits>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/nw_simulation.h"
#include "nw_bq.h"

#define NWG_EXPORT extern "C" __attribute__((visibility("default")))
#define NWG_BLOCK 256
#define NWG_BIAS (1 << (NWG_COORD_BITS - 1))
#define NWG_MAX_START_CELLS (1 << 24)            // the start cells are listed by the host

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- Philox4x32-10 and the maps of the header's comment -------------------------------------------------------------------------------
__device__ __forceinline__ uint4 sim_philox(u64 item, u32 stream, u32 draw, u64 seed)
{
    u32 c0 = (u32)item, c1 = (u32)(item >> 32), c2 = stream, c3 = draw;
    u32 k0 = (u32)seed, k1 = (u32)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u32 hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

__device__ __forceinline__ double sim_unit(u32 hi, u32 lo)
{
    return ((double)((((u64)hi << 32) | lo) >> 11) + 0.5) * 0x1p-53;
}

__device__ __forceinline__ double sim_uniform(u64 item, u32 stream, u32 draw, u64 seed)
{
    const uint4 w = sim_philox(item, stream, draw, seed);
    return sim_unit(w.x, w.y);
}

__device__ __forceinline__ double sim_normal(u64 item, u32 stream, u32 draw, u64 seed)
{
    const uint4 w = sim_philox(item, stream, draw, seed);
    return sqrt(-2.0 * log(sim_unit(w.x, w.y))) * cospi(2.0 * sim_unit(w.z, w.w));
}

__device__ __forceinline__ u64 sim_key64(u64 item, u32 stream, u64 seed)
{
    const uint4 w = sim_philox(item, stream, 0u, seed);
    return ((u64)w.x << 32) | w.y;
}

// photons and sigma of one item and axis (util.py:39-43)
__device__ __forceinline__ double sim_sigma(u64 item, u32 stream, u32 axis, u64 seed, double psf, double mean, double bg, double *photons)
{
    const double l = bg + mean * (-log(sim_uniform(item, stream, axis, seed)));
    if (photons) *photons = l;
    return (psf / 2.355) / sqrt(l);
}

// ---- the shape ------------------------------------------------------------------------------------------------------------------------
// The program at (px, py, pz).  `prog` and `nops` are the same for the whole launch: every load from prog has a wave-uniform address and
// every branch below is wave-uniform.  The stack is s0 (top) .. s7.
__device__ __forceinline__ double sim_eval(const nwg_op *__restrict__ prog, int nops, double px, double py, double pz)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0, s6 = 0.0, s7 = 0.0;
    double qx = px, qy = py, qz = pz;
    for (int o = 0; o < nops; ++o) {
        const nwg_op *__restrict__ op = prog + o;
        const int code = op->code;
        if (code == NWG_OP_FRAME) {
            const double ex = px - op->a[9], ey = py - op->a[10], ez = pz - op->a[11];
            qx = (op->a[0] * ex + op->a[1] * ey) + op->a[2] * ez;
            qy = (op->a[3] * ex + op->a[4] * ey) + op->a[5] * ez;
            qz = (op->a[6] * ex + op->a[7] * ey) + op->a[8] * ez;
            continue;
        }
        if (code >= NWG_OP_UNION) {
            const double d0 = s1, d1 = s0, k = op->a[0];
            double res, h;
            if (code == NWG_OP_UNION) {                                   // shape.py:372-376
                res = fmin(d0, d1);
                h = fmax(k - fabs(d0 - d1), 0.0);
                if (k > 0.0) res = res - h * h * 0.25 / k;
            } else if (code == NWG_OP_DIFFERENCE) {                       // shape.py:406-410
                res = fmax(-d0, d1);
                h = fmax(k - fabs(-d0 - d1), 0.0);
                if (k > 0.0) res = res + h * h * 0.25 / k;
            } else {                                                      // shape.py:440-444
                res = fmax(d0, d1);
                h = fmax(k - fabs(d0 - d1), 0.0);
                if (k > 0.0) res = res + h * h * 0.25 / k;
            }
            s0 = res; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
            continue;
        }
        double v;
        if (code == NWG_OP_SPHERE) {                                      // sdf.py:46
            v = sqrt((qx * qx + qy * qy) + qz * qz) - op->a[0];
        } else if (code == NWG_OP_TORUS) {                                // sdf.py:57-58
            const double t = sqrt(qx * qx + qz * qz) - op->a[0];
            v = sqrt(t * t + qy * qy) - op->a[1];
        } else if (code == NWG_OP_CAPSULE) {                              // sdf.py:74-77
            const double ax = op->a[0], ay = op->a[1], az = op->a[2];
            const double bx = op->a[3] - ax, by = op->a[4] - ay, bz = op->a[5] - az;
            const double ux = qx - ax, uy = qy - ay, uz = qz - az;
            const double h = fmin(fmax(((ux * bx + uy * by) + uz * bz) / ((bx * bx + by * by) + bz * bz), 0.0), 1.0);
            const double dx = ux - bx * h, dy = uy - by * h, dz = uz - bz * h;
            v = sqrt((dx * dx + dy * dy) + dz * dz) - op->a[6];
        } else {                                                          // sdf.py:268-269 and :290-292
            const double wz = op->a[2], r = op->a[3];
            const double x = fabs(qx) - op->a[0], y = fabs(qy) - op->a[1], z = fabs(qz) - wz;
            const double m = fmax(x, fmax(y, z));
            if (code == NWG_OP_ROUND_BOX) {
                const double x0 = fmax(x, 0.0), y0 = fmax(y, 0.0), z0 = fmax(z, 0.0);
                v = sqrt((x0 * x0 + y0 * y0) + z0 * z0) + fmin(m, 0.0) - r;
            } else {
                const double e = fmax(x, y) + r, f = z + wz;
                v = fmin(sqrt(e * e + f * f) - r, m);
            }
        }
        s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
    }
    return s0;
}

// sdf.grad_sdf (sdf.py:22-30) at delta = 0.1
__device__ __forceinline__ void sim_grad(const nwg_op *__restrict__ prog, int nops, double x, double y, double z, double *g)
{
    const double d2 = 0.1 / 2.0;
    g[0] = (sim_eval(prog, nops, x + d2, y, z) - sim_eval(prog, nops, x - d2, y, z)) / 0.1;
    g[1] = (sim_eval(prog, nops, x, y + d2, z) - sim_eval(prog, nops, x, y - d2, z)) / 0.1;
    g[2] = (sim_eval(prog, nops, x, y, z + d2) - sim_eval(prog, nops, x, y, z - d2)) / 0.1;
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_eval(const nwg_op *__restrict__ prog, int nops, const double *__restrict__ xyz, int n,
                                                        double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = sim_eval(prog, nops, xyz[3 * (int64_t)i], xyz[3 * (int64_t)i + 1], xyz[3 * (int64_t)i + 2]);
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_normals(const nwg_op *__restrict__ prog, int nops, const double *__restrict__ xyz, int n,
                                                           double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double g[3];
    sim_grad(prog, nops, xyz[3 * (int64_t)i], xyz[3 * (int64_t)i + 1], xyz[3 * (int64_t)i + 2], g);
    const double norm = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);          // sdf.py:34-35
    out[3 * (int64_t)i] = g[0] / norm;
    out[3 * (int64_t)i + 1] = g[1] / norm;
    out[3 * (int64_t)i + 2] = g[2] / norm;
}

// ---- the surface lattice --------------------------------------------------------------------------------------------------------------
struct sim_geom {
    double centre[3];
    double dx;
    int imin, imax;                // the cube in biased node coordinates, both ends included, the same on every axis
};

__device__ __forceinline__ u64 sim_spread(u32 v)            // 21 bits -> every third bit
{
    u64 x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_cell_test(const nwg_op *__restrict__ prog, int nops, const int *__restrict__ cells, int n, int level,
                                                             sim_geom g, double bound, int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int side = 1 << level;
    const double mid = (double)(side - 1) * 0.5;
    double c[3];
    bool in_cube = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int lo = cells[3 * (int64_t)i + d] << level;
        in_cube = in_cube && lo <= g.imax && lo + side - 1 >= g.imin;
        c[d] = g.centre[d] + ((double)(lo - NWG_BIAS) + mid) * g.dx;
    }
    flag[i] = (in_cube && fabs(sim_eval(prog, nops, c[0], c[1], c[2])) <= bound) ? 1 : 0;
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_cell_split(const int *__restrict__ cells, int n, const int *__restrict__ flag, const int *__restrict__ slot,
                                                              int n_kept, int *__restrict__ children)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int o = slot[i];
    if (o < 0 || o >= n_kept) return;                         // (cannot happen: slot is the scan of flag)
    const int x = cells[3 * (int64_t)i] << 1, y = cells[3 * (int64_t)i + 1] << 1, z = cells[3 * (int64_t)i + 2] << 1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int *c = children + 3 * (8 * (int64_t)o + k);
        c[0] = x + (k & 1);
        c[1] = y + ((k >> 1) & 1);
        c[2] = z + (k >> 2);
    }
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_leaf_test(const nwg_op *__restrict__ prog, int nops, const int *__restrict__ nodes, int n, sim_geom g,
                                                             double p, u64 seed, int *__restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = nodes[3 * (int64_t)i], y = nodes[3 * (int64_t)i + 1], z = nodes[3 * (int64_t)i + 2];
    int keep = 0;
    if (min(x, min(y, z)) >= g.imin && max(x, max(y, z)) <= g.imax) {
        const double d = sim_eval(prog, nops, g.centre[0] + (double)(x - NWG_BIAS) * g.dx, g.centre[1] + (double)(y - NWG_BIAS) * g.dx,
                                  g.centre[2] + (double)(z - NWG_BIAS) * g.dx);
        const double half = 0.5 * g.dx;
        if (d >= -half && d < half) {
            const u64 key = sim_spread((u32)x) | (sim_spread((u32)y) << 1) | (sim_spread((u32)z) << 2);
            keep = sim_uniform(key, NWG_STREAM_THIN, 0u, seed) < p ? 1 : 0;
        }
    }
    flag[i] = keep;
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_leaf_emit(const int *__restrict__ nodes, int n, const int *__restrict__ flag, const int *__restrict__ slot,
                                                             int n_out, sim_geom g, u64 *__restrict__ keys, double *__restrict__ xyz)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int o = slot[i];
    if (o < 0 || o >= n_out) return;                          // (cannot happen: slot is the scan of flag, and n_out was checked against the capacity)
    const int x = nodes[3 * (int64_t)i], y = nodes[3 * (int64_t)i + 1], z = nodes[3 * (int64_t)i + 2];
    keys[o] = sim_spread((u32)x) | (sim_spread((u32)y) << 1) | (sim_spread((u32)z) << 2);
    xyz[3 * (int64_t)o] = g.centre[0] + (double)(x - NWG_BIAS) * g.dx;
    xyz[3 * (int64_t)o + 1] = g.centre[1] + (double)(y - NWG_BIAS) * g.dx;
    xyz[3 * (int64_t)o + 2] = g.centre[2] + (double)(z - NWG_BIAS) * g.dx;
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_project(const nwg_op *__restrict__ prog, int nops, double *__restrict__ xyz, int n, int steps)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x = xyz[3 * (int64_t)i], y = xyz[3 * (int64_t)i + 1], z = xyz[3 * (int64_t)i + 2];
    for (int s = 0; s < steps; ++s) {
        double g[3];
        const double d = sim_eval(prog, nops, x, y, z);
        sim_grad(prog, nops, x, y, z, g);
        const double g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        if (!(g2 > 0.0)) break;                               // (a flat spot of the field: the point stays)
        const double t = d / g2;
        x = x - t * g[0];
        y = y - t * g[1];
        z = z - t * g[2];
    }
    xyz[3 * (int64_t)i] = x;
    xyz[3 * (int64_t)i + 1] = y;
    xyz[3 * (int64_t)i + 2] = z;
}

// ---- the localization model -----------------------------------------------------------------------------------------------------------
struct sim_model {
    int exponential;
    double psf[3], mean, bg;
};

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_loc_error(int n, u64 seed, u32 stream, sim_model m, double *__restrict__ sigma, double *__restrict__ photons)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double l = 0.0;
        sigma[3 * (int64_t)i + a] = m.exponential ? sim_sigma((u64)i, stream, (u32)a, seed, m.psf[a], m.mean, m.bg, &l) : 10.0;
        if (photons) photons[3 * (int64_t)i + a] = l;
    }
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_displace(const double *__restrict__ xyz, const double *__restrict__ sigma, int n, u64 seed, u32 stream,
                                                            double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out[3 * (int64_t)i + a] = xyz[3 * (int64_t)i + a] + sigma[3 * (int64_t)i + a] * sim_normal((u64)i, stream, (u32)a, seed);
}

struct sim_box {
    double lo[3], hi[3];
};

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_background(int n, u64 seed, u32 stream, sim_box b, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        out[3 * (int64_t)i + a] = sim_uniform((u64)i, stream, (u32)a, seed) * (b.hi[a] - b.lo[a]) + b.lo[a];
}

// ---- clusters -------------------------------------------------------------------------------------------------------------------------
// one byte of the radix select: the histogram of byte (key >> shift) over the copies whose key agrees with `prefix` above that byte
__global__ __launch_bounds__(NWG_BLOCK) void k_sim_copy_hist(int n_copies, u64 seed, u32 stream, u64 prefix, int shift, u32 *__restrict__ hist)
{
    __shared__ u32 s_h[256];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n_copies; j += gridDim.x * blockDim.x) {
        const int b = bq::radix_bin(sim_key64((u64)j, stream, seed), prefix, shift);
        if (b >= 0) atomicAdd(&s_h[b], 1u);
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_copy_equal(int n_copies, u64 seed, u32 stream, u64 threshold, int *__restrict__ equal)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_copies) return;
    equal[j] = sim_key64((u64)j, stream, seed) == threshold ? 1 : 0;
}

// kept: a key below the threshold, or one of the first n_equal (by index) that equal it
__global__ __launch_bounds__(NWG_BLOCK) void k_sim_copy_keep(int n_copies, u64 seed, u32 stream, u64 threshold, const int *__restrict__ equal_rank, int n_equal,
                                                             int *__restrict__ keep)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_copies) return;
    const u64 key = sim_key64((u64)j, stream, seed);
    keep[j] = (key < threshold || (key == threshold && equal_rank[j] < n_equal)) ? 1 : 0;
}

__global__ __launch_bounds__(NWG_BLOCK) void k_sim_copy_emit(const double *__restrict__ xyz, const double *__restrict__ sigma, int n, int n_copies,
                                                             const int *__restrict__ keep, const int *__restrict__ slot, int sz, u64 seed, u32 stream_displace,
                                                             u32 stream_photons, sim_model m, double *__restrict__ xyz_out, double *__restrict__ sigma_out,
                                                             long long *__restrict__ copy_out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_copies || !keep[j]) return;
    const int o = slot[j];
    if (o < 0 || o >= sz) return;                             // (cannot happen: the host checked that the slots add up to sz)
    const int i = j % n;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        xyz_out[3 * (int64_t)o + a] = xyz[3 * (int64_t)i + a] + sigma[3 * (int64_t)i + a] * sim_normal((u64)j, stream_displace, (u32)a, seed);
        sigma_out[3 * (int64_t)o + a] = m.exponential ? sim_sigma((u64)j, stream_photons, (u32)a, seed, m.psf[a], m.mean, m.bg, nullptr) : 10.0;
    }
    copy_out[o] = j;
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwg_ctx : bq::Ctx {
    int n_ops = 0;
    DevBuf prog;
    // the points of the last nwg_sample_surface
    int64_t n_points = 0;
    DevBuf keys, points;
    // work
    DevBuf cells0, cells1, flag, slot, in0, in1, out0, out1, out2, hist;
    DevBuf scan_tmp;
};

namespace {

#define NWG_HIP(call) BQ_HIP(call, NWG_ERR_NOMEM, NWG_ERR_HIP)

bool count_ok(int64_t n) { return n >= 1 && n <= (1ll << 30); }

// the arguments every op reads, and whether its k / radii are in range
int check_program(const nwg_op *ops, int n_ops, std::string *why)
{
    static const int n_args[] = {12, 1, 2, 7, 4, 4, 1, 1, 1};
    int depth = 0;
    for (int o = 0; o < n_ops; ++o) {
        const int code = ops[o].code;
        if (code < NWG_OP_FRAME || code > NWG_OP_INTERSECTION || ops[o].reserved != 0) { *why = "op " + std::to_string(o) + ": unknown code"; return NWG_ERR_BADARG; }
        for (int k = 0; k < n_args[code]; ++k)
            if (!std::isfinite(ops[o].a[k])) { *why = "op " + std::to_string(o) + ": a non-finite argument"; return NWG_ERR_BADARG; }
        if (code == NWG_OP_FRAME) continue;
        if (code == NWG_OP_CAPSULE) {                          // sdf.capsule divides by |b - a|^2: 0 / 0 at every point of a capsule without length
            const double bx = ops[o].a[3] - ops[o].a[0], by = ops[o].a[4] - ops[o].a[1], bz = ops[o].a[5] - ops[o].a[2];
            if (!((bx * bx + by * by) + bz * bz > 0.0)) { *why = "op " + std::to_string(o) + ": a capsule whose ends coincide"; return NWG_ERR_BADARG; }
        }
        if (code >= NWG_OP_UNION) {
            if (ops[o].a[0] < 0.0) { *why = "op " + std::to_string(o) + ": negative k"; return NWG_ERR_BADARG; }
            if (depth < 2) { *why = "op " + std::to_string(o) + ": a combinator with fewer than two values on the stack"; return NWG_ERR_BADARG; }
            --depth;
        } else if (++depth > NWG_STACK_DEPTH) {
            *why = "op " + std::to_string(o) + ": the stack is deeper than NWG_STACK_DEPTH";
            return NWG_ERR_BADARG;
        }
    }
    if (depth != 1) { *why = "the program leaves " + std::to_string(depth) + " values"; return NWG_ERR_BADARG; }
    return NWG_OK;
}

bool model_ok(int model, const double *psf, double mean, double bg)
{
    if (model == NWG_MODEL_CONSTANT) return true;
    if (model != NWG_MODEL_EXPONENTIAL || !psf) return false;
    for (int a = 0; a < 3; ++a)
        if (!(psf[a] > 0.0) || !std::isfinite(psf[a])) return false;
    return mean > 0.0 && std::isfinite(mean) && bg >= 0.0 && std::isfinite(bg) && (bg > 0.0 || mean > 0.0);
}

sim_model make_model(int model, const double *psf, double mean, double bg)
{
    sim_model m;
    m.exponential = model == NWG_MODEL_EXPONENTIAL;
    for (int a = 0; a < 3; ++a) m.psf[a] = m.exponential ? psf[a] : 0.0;
    m.mean = mean;
    m.bg = bg;
    return m;
}

// the cells of [lo, hi]^3 inside the aligned cube of side 2^bits at (x, y, z), appended in ascending Morton code of their coordinates:
// an octree descent (x is the lowest bit of a code's triple) that skips every octant outside the range
void morton_cells(int x, int y, int z, int bits, int lo, int hi, std::vector<int> &out)
{
    const int side = 1 << bits;
    if (x > hi || y > hi || z > hi || x + side - 1 < lo || y + side - 1 < lo || z + side - 1 < lo) return;
    if (bits == 0) {
        out.push_back(x);
        out.push_back(y);
        out.push_back(z);
        return;
    }
    const int h = side >> 1;
    for (int k = 0; k < 8; ++k) morton_cells(x + (k & 1) * h, y + ((k >> 1) & 1) * h, z + (k >> 2) * h, bits - 1, lo, hi, out);
}

}  // namespace

NWG_EXPORT int nwg_abi_version(void) { return NWG_ABI_VERSION; }

NWG_EXPORT int nwg_create(int device, nwg_ctx **out) { return bq::create(device, out, NWG_ERR_BADARG, NWG_ERR_HIP); }

NWG_EXPORT void nwg_destroy(nwg_ctx *ctx) { bq::destroy(ctx); }

NWG_EXPORT const char *nwg_last_error(nwg_ctx *ctx) { return bq::last_error(ctx); }

NWG_EXPORT int nwg_set_program(nwg_ctx *ctx, const nwg_op *ops, int n_ops)
{
    if (!ops || n_ops < 1 || n_ops > NWG_MAX_OPS) return NWG_ERR_BADARG;
    std::string why;
    if (check_program(ops, n_ops, &why) != NWG_OK) return fail(ctx, NWG_ERR_BADARG, "nwg_set_program: " + why);
    if (!ctx) return NWG_ERR_BADARG;
    ctx->n_ops = 0;
    NWG_HIP(hipSetDevice(ctx->device));
    NWG_HIP(bq::upload(ctx->stream, ctx->prog, ops, n_ops));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    ctx->n_ops = n_ops;
    return NWG_OK;
}

NWG_EXPORT int nwg_eval(nwg_ctx *ctx, const double *xyz, int64_t n, double *d_out)
{
    if (!xyz || !d_out || !count_ok(n)) return NWG_ERR_BADARG;
    if (!ctx) return NWG_ERR_BADARG;
    if (!ctx->n_ops) return fail(ctx, NWG_ERR_NOPROGRAM, "nwg_eval: no program is set");
    if (!bq::all_finite(xyz, 3 * n)) return fail(ctx, NWG_ERR_NONFINITE, "nwg_eval: a coordinate is not finite");
    NWG_HIP(hipSetDevice(ctx->device));
    NWG_HIP(bq::upload(ctx->stream, ctx->in0, xyz, 3 * n));
    NWG_HIP(ctx->out0.ensure(sizeof(double) * (size_t)n));
    hipLaunchKernelGGL(k_sim_eval, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, ctx->prog.as<nwg_op>(), ctx->n_ops, ctx->in0.as<double>(), (int)n,
                       ctx->out0.as<double>());
    NWG_HIP(hipGetLastError());
    NWG_HIP(hipMemcpyAsync(d_out, ctx->out0.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    return NWG_OK;
}

NWG_EXPORT int nwg_normals(nwg_ctx *ctx, const double *xyz, int64_t n, double *normals_out)
{
    if (!xyz || !normals_out || !count_ok(n)) return NWG_ERR_BADARG;
    if (!ctx) return NWG_ERR_BADARG;
    if (!ctx->n_ops) return fail(ctx, NWG_ERR_NOPROGRAM, "nwg_normals: no program is set");
    if (!bq::all_finite(xyz, 3 * n)) return fail(ctx, NWG_ERR_NONFINITE, "nwg_normals: a coordinate is not finite");
    NWG_HIP(hipSetDevice(ctx->device));
    NWG_HIP(bq::upload(ctx->stream, ctx->in0, xyz, 3 * n));
    NWG_HIP(ctx->out0.ensure(sizeof(double) * 3 * (size_t)n));
    hipLaunchKernelGGL(k_sim_normals, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, ctx->prog.as<nwg_op>(), ctx->n_ops, ctx->in0.as<double>(), (int)n,
                       ctx->out0.as<double>());
    NWG_HIP(hipGetLastError());
    NWG_HIP(hipMemcpyAsync(normals_out, ctx->out0.p, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    return NWG_OK;
}

NWG_EXPORT int nwg_sample_surface(nwg_ctx *ctx, const double *centre, double r_max, double dx, double p, uint64_t seed, double lipschitz,
                                  int start_level, int project, int64_t max_points, int64_t *n_out)
{
    if (!centre || !n_out || !(dx > 0.0) || !std::isfinite(dx) || !(r_max > 0.0) || !std::isfinite(r_max) || !(p >= 0.0) || !std::isfinite(p)) return NWG_ERR_BADARG;
    if (!(lipschitz >= 1.0) || !std::isfinite(lipschitz) || project < 0 || project > 64 || max_points < 1 || max_points > (1ll << 30)) return NWG_ERR_BADARG;
    if (start_level < -1 || start_level >= NWG_COORD_BITS || !bq::all_finite(centre, 3)) return NWG_ERR_BADARG;
    const double half_nodes = std::floor(r_max / dx);
    if (!(half_nodes <= (double)(NWG_BIAS - 1))) return NWG_ERR_BADARG;          // the node coordinates would not fit NWG_COORD_BITS
    if (!ctx) return NWG_ERR_BADARG;
    *n_out = 0;
    ctx->n_points = 0;
    if (!ctx->n_ops) return fail(ctx, NWG_ERR_NOPROGRAM, "nwg_sample_surface: no program is set");
    sim_geom g;
    for (int d = 0; d < 3; ++d) g.centre[d] = centre[d];
    g.dx = dx;
    g.imin = NWG_BIAS - (int)half_nodes;
    g.imax = NWG_BIAS + (int)half_nodes;
    int level = start_level;
    if (level < 0)
        for (level = 0; (g.imax >> level) - (g.imin >> level) + 1 > 8; ++level) {}
    // the start cells, in Morton order
    const int c0 = g.imin >> level, c1 = g.imax >> level;
    const int64_t per_axis = (int64_t)c1 - c0 + 1;
    if (per_axis * per_axis * per_axis > NWG_MAX_START_CELLS) return fail(ctx, NWG_ERR_BADARG, "nwg_sample_surface: start_level gives more than 2^24 start cells");
    std::vector<int> start;
    start.reserve((size_t)(3 * per_axis * per_axis * per_axis));
    int bits = 0;
    while ((c0 >> bits) != (c1 >> bits)) ++bits;
    const int base = (c0 >> bits) << bits;
    morton_cells(base, base, base, bits, c0, c1, start);
    NWG_HIP(hipSetDevice(ctx->device));
    int n = (int)(start.size() / 3);
    NWG_HIP(bq::upload(ctx->stream, ctx->cells0, start.data(), (int64_t)start.size()));
    NWG_HIP(hipStreamSynchronize(ctx->stream));               // (`start` leaves scope below)
    DevBuf *cur = &ctx->cells0, *nxt = &ctx->cells1;
    const nwg_op *prog = ctx->prog.as<nwg_op>();
    for (; level > 0; --level) {
        // |sdf| at the centre of a cell that holds a fluorophore is at most lipschitz x the half-diagonal + dx / 2
        const double bound = lipschitz * (0.8660254037844386 * dx * (double)(1 << level)) + 0.5 * dx;
        NWG_HIP(ctx->flag.ensure(sizeof(int) * (size_t)n));
        NWG_HIP(ctx->slot.ensure(sizeof(int) * ((size_t)n + 1)));
        hipLaunchKernelGGL(k_sim_cell_test, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, prog, ctx->n_ops, cur->as<int>(), n, level, g, bound, ctx->flag.as<int>());
        NWG_HIP(hipGetLastError());
        int kept = -1;
        NWG_HIP(bq::scan_total(ctx->stream, ctx->flag.as<int>(), n, ctx->slot.as<int>(), ctx->scan_tmp, &kept));
        if (kept < 0 || kept > n) return fail(ctx, NWG_ERR_HIP, "nwg_sample_surface: the cell slots do not add up");
        if (kept == 0) return NWG_OK;
        if (8ll * kept > NWG_MAX_CELLS) return fail(ctx, NWG_ERR_TOOMANY, "nwg_sample_surface: " + std::to_string(8ll * kept) + " cells at level " + std::to_string(level - 1));
        NWG_HIP(nxt->ensure(sizeof(int) * 3 * 8 * (size_t)kept));
        hipLaunchKernelGGL(k_sim_cell_split, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, cur->as<int>(), n, ctx->flag.as<int>(), ctx->slot.as<int>(), kept,
                           nxt->as<int>());
        NWG_HIP(hipGetLastError());
        std::swap(cur, nxt);
        n = 8 * kept;
    }
    // the candidate nodes
    NWG_HIP(ctx->flag.ensure(sizeof(int) * (size_t)n));
    NWG_HIP(ctx->slot.ensure(sizeof(int) * ((size_t)n + 1)));
    hipLaunchKernelGGL(k_sim_leaf_test, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, prog, ctx->n_ops, cur->as<int>(), n, g, p, (u64)seed, ctx->flag.as<int>());
    NWG_HIP(hipGetLastError());
    int found = -1;
    NWG_HIP(bq::scan_total(ctx->stream, ctx->flag.as<int>(), n, ctx->slot.as<int>(), ctx->scan_tmp, &found));
    if (found < 0 || found > n) return fail(ctx, NWG_ERR_HIP, "nwg_sample_surface: the output slots do not add up");
    if (found == 0) return NWG_OK;
    if (found > max_points) return fail(ctx, NWG_ERR_CAPACITY, "nwg_sample_surface: " + std::to_string(found) + " detected nodes, max_points is " + std::to_string(max_points));
    NWG_HIP(ctx->keys.ensure(sizeof(u64) * (size_t)found));
    NWG_HIP(ctx->points.ensure(sizeof(double) * 3 * (size_t)found));
    hipLaunchKernelGGL(k_sim_leaf_emit, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, cur->as<int>(), n, ctx->flag.as<int>(), ctx->slot.as<int>(), found, g,
                       ctx->keys.as<u64>(), ctx->points.as<double>());
    if (project > 0)
        hipLaunchKernelGGL(k_sim_project, dim3(nblk(found)), dim3(NWG_BLOCK), 0, ctx->stream, prog, ctx->n_ops, ctx->points.as<double>(), found, project);
    NWG_HIP(hipGetLastError());
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    ctx->n_points = found;
    *n_out = found;
    return NWG_OK;
}

NWG_EXPORT int nwg_get_points(nwg_ctx *ctx, uint64_t *keys_out, double *xyz_out)
{
    if (!ctx) return NWG_ERR_BADARG;
    if (ctx->n_points < 1) return fail(ctx, NWG_ERR_NOPOINTS, "nwg_get_points: the context holds no points");
    NWG_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->n_points;
    if (keys_out) NWG_HIP(hipMemcpyAsync(keys_out, ctx->keys.p, sizeof(u64) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (xyz_out) NWG_HIP(hipMemcpyAsync(xyz_out, ctx->points.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    return NWG_OK;
}

NWG_EXPORT int nwg_loc_error(nwg_ctx *ctx, int64_t n, uint64_t seed, uint32_t stream, int model, const double *psf_width, double mean_photon_count,
                             double bg_photon_count, double *sigma_out, double *photons_out)
{
    if (!sigma_out || !count_ok(n) || !model_ok(model, psf_width, mean_photon_count, bg_photon_count)) return NWG_ERR_BADARG;
    if (!ctx) return NWG_ERR_BADARG;
    NWG_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * 3 * (size_t)n;
    NWG_HIP(ctx->out0.ensure(bytes));
    if (photons_out) NWG_HIP(ctx->out1.ensure(bytes));
    hipLaunchKernelGGL(k_sim_loc_error, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, (int)n, (u64)seed, stream,
                       make_model(model, psf_width, mean_photon_count, bg_photon_count), ctx->out0.as<double>(), photons_out ? ctx->out1.as<double>() : nullptr);
    NWG_HIP(hipGetLastError());
    NWG_HIP(hipMemcpyAsync(sigma_out, ctx->out0.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (photons_out) NWG_HIP(hipMemcpyAsync(photons_out, ctx->out1.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    return NWG_OK;
}

NWG_EXPORT int nwg_displace(nwg_ctx *ctx, const double *xyz, const double *sigma, int64_t n, uint64_t seed, uint32_t stream, double *out)
{
    if (!xyz || !sigma || !out || !count_ok(n)) return NWG_ERR_BADARG;
    if (!ctx) return NWG_ERR_BADARG;
    if (!bq::all_finite(xyz, 3 * n) || !bq::all_finite(sigma, 3 * n)) return fail(ctx, NWG_ERR_NONFINITE, "nwg_displace: a coordinate or a sigma is not finite");
    NWG_HIP(hipSetDevice(ctx->device));
    const size_t bytes = sizeof(double) * 3 * (size_t)n;
    NWG_HIP(bq::upload(ctx->stream, ctx->in0, xyz, 3 * n));
    NWG_HIP(bq::upload(ctx->stream, ctx->in1, sigma, 3 * n));
    NWG_HIP(ctx->out0.ensure(bytes));
    hipLaunchKernelGGL(k_sim_displace, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, ctx->in0.as<double>(), ctx->in1.as<double>(), (int)n, (u64)seed, stream,
                       ctx->out0.as<double>());
    NWG_HIP(hipGetLastError());
    NWG_HIP(hipMemcpyAsync(out, ctx->out0.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    return NWG_OK;
}

NWG_EXPORT int nwg_smlmify(nwg_ctx *ctx, const double *xyz, const double *sigma, int64_t n, int64_t sz, uint64_t seed, uint32_t stream_displace,
                           uint32_t stream_key, uint32_t stream_photons, int model, const double *psf_width, double mean_photon_count,
                           double bg_photon_count, double *xyz_out, double *sigma_out, int64_t *copy_out)
{
    if (!xyz || !sigma || !xyz_out || !sigma_out || n < 1 || n > (1ll << 30) / NWG_COPIES || sz < 1 || sz > NWG_COPIES * n) return NWG_ERR_BADARG;
    if (!model_ok(model, psf_width, mean_photon_count, bg_photon_count)) return NWG_ERR_BADARG;
    if (!ctx) return NWG_ERR_BADARG;
    if (!bq::all_finite(xyz, 3 * n) || !bq::all_finite(sigma, 3 * n)) return fail(ctx, NWG_ERR_NONFINITE, "nwg_smlmify: a coordinate or a sigma is not finite");
    NWG_HIP(hipSetDevice(ctx->device));
    const int nc = (int)(NWG_COPIES * n);
    NWG_HIP(bq::upload(ctx->stream, ctx->in0, xyz, 3 * n));
    NWG_HIP(bq::upload(ctx->stream, ctx->in1, sigma, 3 * n));
    // the sz-th smallest key; `rank` is what is left of its 0-based rank among the copies that hold the same key
    NWG_HIP(ctx->hist.ensure(sizeof(u32) * 256));
    uint64_t threshold = 0;
    int64_t rank = -1;
    const auto pass = [&](uint64_t prefix, int shift, unsigned *hist) {
        hipLaunchKernelGGL(k_sim_copy_hist, dim3(std::min(nblk(nc), 2048)), dim3(NWG_BLOCK), 0, ctx->stream, nc, (u64)seed, stream_key, (u64)prefix, shift, hist);
    };
    NWG_HIP(bq::select_u64(ctx->stream, ctx->hist.as<u32>(), 56, pass, [&](int64_t) { return sz - 1; }, &threshold, &rank));
    if (rank < 0) return fail(ctx, NWG_ERR_HIP, "nwg_smlmify: the key histogram does not reach the rank");
    const int n_equal = (int)rank + 1;                        // of the copies whose key equals the threshold, the first n_equal are kept
    NWG_HIP(ctx->flag.ensure(sizeof(int) * (size_t)nc));
    NWG_HIP(ctx->slot.ensure(sizeof(int) * ((size_t)nc + 1)));
    NWG_HIP(ctx->cells0.ensure(sizeof(int) * ((size_t)nc + 1)));                   // (the rank among equal keys; free between two lattices)
    hipLaunchKernelGGL(k_sim_copy_equal, dim3(nblk(nc)), dim3(NWG_BLOCK), 0, ctx->stream, nc, (u64)seed, stream_key, (u64)threshold, ctx->flag.as<int>());
    NWG_HIP(hipGetLastError());
    NWG_HIP(bq::scan_exclusive(ctx->stream, ctx->flag.as<int>(), nc, ctx->cells0.as<int>(), ctx->scan_tmp));
    hipLaunchKernelGGL(k_sim_copy_keep, dim3(nblk(nc)), dim3(NWG_BLOCK), 0, ctx->stream, nc, (u64)seed, stream_key, (u64)threshold, ctx->cells0.as<int>(), n_equal,
                       ctx->flag.as<int>());
    NWG_HIP(hipGetLastError());
    int total = -1;
    NWG_HIP(bq::scan_total(ctx->stream, ctx->flag.as<int>(), nc, ctx->slot.as<int>(), ctx->scan_tmp, &total));
    if (total != sz) return fail(ctx, NWG_ERR_HIP, "nwg_smlmify: the selection kept " + std::to_string(total) + " copies, not " + std::to_string(sz));
    const size_t bytes = sizeof(double) * 3 * (size_t)sz;
    NWG_HIP(ctx->out0.ensure(bytes));
    NWG_HIP(ctx->out1.ensure(bytes));
    NWG_HIP(ctx->out2.ensure(sizeof(long long) * (size_t)sz));
    hipLaunchKernelGGL(k_sim_copy_emit, dim3(nblk(nc)), dim3(NWG_BLOCK), 0, ctx->stream, ctx->in0.as<double>(), ctx->in1.as<double>(), (int)n, nc,
                       ctx->flag.as<int>(), ctx->slot.as<int>(), (int)sz, (u64)seed, stream_displace, stream_photons,
                       make_model(model, psf_width, mean_photon_count, bg_photon_count), ctx->out0.as<double>(), ctx->out1.as<double>(), ctx->out2.as<long long>());
    NWG_HIP(hipGetLastError());
    NWG_HIP(hipMemcpyAsync(xyz_out, ctx->out0.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipMemcpyAsync(sigma_out, ctx->out1.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (copy_out) NWG_HIP(hipMemcpyAsync(copy_out, ctx->out2.p, sizeof(long long) * (size_t)sz, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    return NWG_OK;
}

NWG_EXPORT int nwg_background(nwg_ctx *ctx, const double *lo, const double *hi, int64_t n, uint64_t seed, uint32_t stream, double *xyz_out)
{
    if (!lo || !hi || !xyz_out || !count_ok(n) || !bq::all_finite(lo, 3) || !bq::all_finite(hi, 3)) return NWG_ERR_BADARG;
    if (!ctx) return NWG_ERR_BADARG;
    NWG_HIP(hipSetDevice(ctx->device));
    sim_box b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = lo[a]; b.hi[a] = hi[a]; }
    const size_t bytes = sizeof(double) * 3 * (size_t)n;
    NWG_HIP(ctx->out0.ensure(bytes));
    hipLaunchKernelGGL(k_sim_background, dim3(nblk(n)), dim3(NWG_BLOCK), 0, ctx->stream, (int)n, (u64)seed, stream, b, ctx->out0.as<double>());
    NWG_HIP(hipGetLastError());
    NWG_HIP(hipMemcpyAsync(xyz_out, ctx->out0.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    NWG_HIP(hipStreamSynchronize(ctx->stream));
    return NWG_OK;
}
