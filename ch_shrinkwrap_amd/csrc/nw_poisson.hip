// The screened Poisson grid solver on the device (MI355X, gfx950): include/nw_poisson.h.
//
//   k_sp_prepare     one lane per sample: finiteness, the normal's quantised components (nwo_normal), the count of samples in use
//   k_sp_mark        one lane per sample: a byte at its home node of a level;  k_sp_count: the bytes that are set (the occupancy)
//   k_sp_splat       one lane per sample: its eight nodes' weights into W and V[3], 64-bit integer atomic adds whose results are not
//                    read (terms that are zero are not sent: the sums are the same).  Exact, whatever the order of arrival
//   k_sp_splat_lds   the same for levels 2 and 3, summed in LDS first: a word of the level takes 64 global adds at most, not one a sample
//   k_sp_splat_lds4  the same for level 4, whose four planes take 128 KB of LDS
//   k_sp_system      one lane per node: rhs and diag from W and V (nwo_system_node)
//   k_sp_prolong     one lane per node of the finer level: 0.75 / 0.25 along x, y, z from the eight coarse nodes around it
//   k_sp_relax       one colour of a sweep, one lane per PAIR of x-neighbours: of the nodes (2 p, j, k) and (2 p + 1, j, k) exactly one has
//                    the colour, so a wave's 64 lanes update 64 nodes of a run of 128 and touch one contiguous kilobyte of each of chi, rhs
//                    and diag.  Half of every rhs and diag line is the other colour's: the sweep reads those two arrays twice a sweep
//                    where a colour-split layout would read them once.  Nobody has measured that against the split layout's cost
//                    (two more arrays, or a system kernel that writes them split)
//   k_sp_residual    one lane per node: |rhs - (diag chi - S)|, the workgroup's largest into one 64-bit integer atomic maximum (the bits of
//                    a non-negative double order as the double does)
//   k_sp_absmax      the largest |chi|, the same way
//   k_sp_field       one lane per node: F, and the workgroup's sums of W, W Fl and W Fh into three 64-bit integer atomic adds
//
// The definition with its proofs is csrc/nw_poisson_core.h, which the tests also compile for the CPU.  There are no float atomics anywhere,
// every offset is 64 bits wide, all stores are vector stores, and no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).  The
// relaxation of levels 2 to 4 is a few launches over at most 4096 nodes: launch-bound, and left so.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cmath>
#include <string>
#include <algorithm>

#include "../../include/nw_poisson.h"
#include "nw_bq.h"
#include "nw_poisson_core.h"

#define NWO_EXPORT extern "C" __attribute__((visibility("default")))
#define NWO_BLOCK 256
#define NWO_WAVES (NWO_BLOCK / 64)
#define NWO_LDS_LEVEL 4               // the levels summed in LDS first: 2 and 3 by k_sp_splat_lds, 4 by k_sp_splat_lds4
#define NWO_LDS_GROUPS 64             // its workgroups at most
#define NWO_BAD_NONFINITE 1
#define NWO_BAD_LENGTH 2

typedef unsigned long long u64;

struct nwo_box { float lo[3]; double hl; int level; };

// the workgroup's sum / maximum of one 64-bit value a lane -> valid in thread 0
__device__ __forceinline__ u64 sp_block_sum(u64 v, u64 *s_w)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NWO_WAVES; ++w) t += s_w[w];
    __syncthreads();
    return t;
}

__device__ __forceinline__ u64 sp_block_max(u64 v, u64 *s_w)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NWO_WAVES; ++w) t = s_w[w] > t ? s_w[w] : t;
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_prepare(const float *__restrict__ xyz, const float *__restrict__ normals, int n, int use_lengths,
                                                          short4 *__restrict__ nq, int *__restrict__ bad, u64 *__restrict__ n_used)
{
    __shared__ u64 s_w[NWO_WAVES];
    const int i = blockIdx.x * NWO_BLOCK + threadIdx.x;
    u64 used = 0;
    if (i < n) {
        const float *p = xyz + 3 * (int64_t)i, *m = normals + 3 * (int64_t)i;
        const float nx = m[0], ny = m[1], nz = m[2];
        short4 out = make_short4(0, 0, 0, 0);
        if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(nx) && isfinite(ny) && isfinite(nz))) {
            atomicOr(bad, NWO_BAD_NONFINITE);
        } else {
            int q[3];
            const int rc = nwo_normal(nx, ny, nz, use_lengths, q);
            if (rc < 0) atomicOr(bad, NWO_BAD_LENGTH);
            if (rc == 1) { out = make_short4((short)q[0], (short)q[1], (short)q[2], 1); used = 1; }
        }
        nq[i] = out;
    }
    const u64 t = sp_block_sum(used, s_w);
    if (threadIdx.x == 0 && t) atomicAdd(n_used, t);
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_mark(const float *__restrict__ xyz, const short4 *__restrict__ nq, int n, nwo_box B,
                                                       unsigned char *__restrict__ mark)
{
    const int i = blockIdx.x * NWO_BLOCK + threadIdx.x;
    if (i >= n || !nq[i].w) return;
    const float *p = xyz + 3 * (int64_t)i;
    const int nl = 1 << B.level;
    mark[nwo_lin(B.level, nwo_home(p[0], B.lo[0], B.hl, nl), nwo_home(p[1], B.lo[1], B.hl, nl), nwo_home(p[2], B.lo[2], B.hl, nl))] = 1;
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_count(const unsigned char *__restrict__ mark, int64_t nodes, u64 *__restrict__ count)
{
    __shared__ u64 s_w[NWO_WAVES];
    u64 c = 0;
    for (int64_t i = (int64_t)blockIdx.x * NWO_BLOCK + threadIdx.x; i < nodes; i += (int64_t)gridDim.x * NWO_BLOCK) c += mark[i] ? 1 : 0;
    const u64 t = sp_block_sum(c, s_w);
    if (threadIdx.x == 0 && t) atomicAdd(count, t);
}

// one sample's eight nodes: w into W and w nq_a into V_a through `add(offset, term)`; terms that are zero are not sent (the sums are the same)
template <class Add>
__device__ __forceinline__ void sp_splat_sample(const float *__restrict__ p, const short4 q, const nwo_box &B, Add add)
{
    const int nl = 1 << B.level;
    const int64_t plane = (int64_t)1 << (3 * B.level);
    int xa, xb, xq, ya, yb, yq, za, zb, zq;
    nwo_axis(p[0], B.lo[0], B.hl, nl, &xa, &xb, &xq);
    nwo_axis(p[1], B.lo[1], B.hl, nl, &ya, &yb, &yq);
    nwo_axis(p[2], B.lo[2], B.hl, nl, &za, &zb, &zq);
    const int one = 1 << NWO_WEIGHT_BITS;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int ix = (c & 1) ? xb : xa, iy = (c & 2) ? yb : ya, iz = (c & 4) ? zb : za;
        const long long w = (long long)((c & 1) ? xq : one - xq) * ((c & 2) ? yq : one - yq) * ((c & 4) ? zq : one - zq);
        if (w == 0) continue;
        const int64_t at = nwo_lin(B.level, ix, iy, iz);
        add(at, (u64)w);
        if (q.x) add(at + plane, (u64)(w * q.x));                      // (two's complement: the unsigned add is the signed one)
        if (q.y) add(at + 2 * plane, (u64)(w * q.y));
        if (q.z) add(at + 3 * plane, (u64)(w * q.z));
    }
}

struct sp_add_global {
    u64 *acc;
    __device__ __forceinline__ void operator()(int64_t at, u64 v) const { atomicAdd(acc + at, v); }
};

struct sp_add_lds {
    u64 *acc;
    __device__ __forceinline__ void operator()(int64_t at, u64 v) const { atomicAdd(acc + (int)at, v); }
};

// acc: W, then the three planes of V, 2^(3 level) int64 each
__global__ __launch_bounds__(NWO_BLOCK) void k_sp_splat(const float *__restrict__ xyz, const short4 *__restrict__ nq, int n, nwo_box B, u64 *__restrict__ acc)
{
    const int i = blockIdx.x * NWO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const short4 q = nq[i];
    if (!q.w) return;
    sp_add_global add = {acc};
    sp_splat_sample(xyz + 3 * (int64_t)i, q, B, add);
}

// The levels up to NWO_LDS_LEVEL, whose four planes fit into LDS: a workgroup adds its samples -- every NWO_LDS_GROUPS-th block of
// NWO_BLOCK of them -- into a copy of the level in LDS and sends each word that is not zero on with one global atomic add.  A word of
// the level takes NWO_LDS_GROUPS adds at most instead of one a sample: measured, the plain kernel spent 12 ms at level 2 and 2.4 ms at
// level 4 of 10^6 samples, and 37 ms at level 4 of 5 10^6, on that contention (profiles/poisson.txt).  The sums are integers: the same
// as the plain kernel's.  Levels 2 and 3 take 16 KB (k_sp_splat_lds), level 4 takes 128 KB, one workgroup a CU (k_sp_splat_lds4)
__device__ __forceinline__ void sp_splat_lds(u64 *s_acc, const float *__restrict__ xyz, const short4 *__restrict__ nq, int n, const nwo_box &B,
                                             u64 *__restrict__ acc)
{
    const int words = 4 << (3 * B.level);
    for (int t = threadIdx.x; t < words; t += NWO_BLOCK) s_acc[t] = 0;
    __syncthreads();
    sp_add_lds add = {s_acc};
    for (int i = blockIdx.x * NWO_BLOCK + threadIdx.x; i < n; i += gridDim.x * NWO_BLOCK) {
        const short4 q = nq[i];
        if (q.w) sp_splat_sample(xyz + 3 * (int64_t)i, q, B, add);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < words; t += NWO_BLOCK) {
        const u64 v = s_acc[t];
        if (v) atomicAdd(acc + t, v);
    }
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_splat_lds(const float *__restrict__ xyz, const short4 *__restrict__ nq, int n, nwo_box B, u64 *__restrict__ acc)
{
    __shared__ u64 s_acc[4 << (3 * (NWO_LDS_LEVEL - 1))];
    sp_splat_lds(s_acc, xyz, nq, n, B, acc);
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_splat_lds4(const float *__restrict__ xyz, const short4 *__restrict__ nq, int n, nwo_box B, u64 *__restrict__ acc)
{
    __shared__ u64 s_acc[4 << (3 * NWO_LDS_LEVEL)];
    sp_splat_lds(s_acc, xyz, nq, n, B, acc);
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_system(const long long *__restrict__ acc, int level, double alpha_s, double inv_s2, double *__restrict__ rhs,
                                                         double *__restrict__ diag)
{
    const int64_t c = (int64_t)blockIdx.x * NWO_BLOCK + threadIdx.x, plane = (int64_t)1 << (3 * level);
    if (c >= plane) return;
    const int m = (1 << level) - 1;
    double r, d;
    nwo_system_node(acc, acc + plane, level, (int)(c & m), (int)((c >> level) & m), (int)(c >> (2 * level)), alpha_s, inv_s2, &r, &d);
    rhs[c] = r;
    diag[c] = d;
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_prolong(const double *__restrict__ coarse, int level, double *__restrict__ chi)
{
    const int64_t c = (int64_t)blockIdx.x * NWO_BLOCK + threadIdx.x;
    if (c >= ((int64_t)1 << (3 * level))) return;
    const int m = (1 << level) - 1;
    chi[c] = nwo_prolong_node(coarse, level, (int)(c & m), (int)((c >> level) & m), (int)(c >> (2 * level)));
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_relax(double *__restrict__ chi, const double *__restrict__ rhs, const double *__restrict__ diag, int level,
                                                        int colour)
{
    const int64_t p = (int64_t)blockIdx.x * NWO_BLOCK + threadIdx.x;
    if (p >= ((int64_t)1 << (3 * level - 1))) return;
    const int m = (1 << level) - 1;
    const int j = (int)((p >> (level - 1)) & m), k = (int)(p >> (2 * level - 1));
    const int i = 2 * (int)(p & (m >> 1)) + ((colour + j + k) & 1);
    const int64_t c = nwo_lin(level, i, j, k);
    chi[c] = nwo_update(rhs[c], nwo_neighbour_sum(chi, level, i, j, k), diag[c]);
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_residual(const double *__restrict__ chi, const double *__restrict__ rhs, const double *__restrict__ diag,
                                                           int level, u64 *__restrict__ out)
{
    __shared__ u64 s_w[NWO_WAVES];
    const int64_t c = (int64_t)blockIdx.x * NWO_BLOCK + threadIdx.x;
    u64 bits = 0;
    if (c < ((int64_t)1 << (3 * level))) {
        const int m = (1 << level) - 1;
        const double S = nwo_neighbour_sum(chi, level, (int)(c & m), (int)((c >> level) & m), (int)(c >> (2 * level)));
        bits = __builtin_bit_cast(u64, nwo_residual(rhs[c], diag[c], chi[c], S));
    }
    const u64 t = sp_block_max(bits, s_w);
    if (threadIdx.x == 0 && t) atomicMax(out, t);
}

__global__ __launch_bounds__(NWO_BLOCK) void k_sp_absmax(const double *__restrict__ chi, int64_t nodes, u64 *__restrict__ out)
{
    __shared__ u64 s_w[NWO_WAVES];
    const int64_t c = (int64_t)blockIdx.x * NWO_BLOCK + threadIdx.x;
    const u64 t = sp_block_max(c < nodes ? __builtin_bit_cast(u64, fabs(chi[c])) : 0ull, s_w);
    if (threadIdx.x == 0 && t) atomicMax(out, t);
}

// sums: sum W, sum W Fl, sum W Fh (Fl = F & 0xffff, Fh = F >> 16)
__global__ __launch_bounds__(NWO_BLOCK) void k_sp_field(const double *__restrict__ chi, const long long *__restrict__ W, int64_t nodes, double E,
                                                        u64 *__restrict__ F, u64 *__restrict__ sums)
{
    __shared__ u64 s_w[NWO_WAVES];
    const int64_t c = (int64_t)blockIdx.x * NWO_BLOCK + threadIdx.x;
    u64 w = 0, f = 0;
    if (c < nodes) {
        w = (u64)W[c];
        f = nwo_quantise(chi[c], E);
        F[c] = f;
    }
    const u64 sw = sp_block_sum(w, s_w), sl = sp_block_sum(w * (f & 0xffffull), s_w), sh = sp_block_sum(w * (f >> 16), s_w);
    if (threadIdx.x == 0 && sw) {
        atomicAdd(sums, sw);
        if (sl) atomicAdd(sums + 1, sl);
        if (sh) atomicAdd(sums + 2, sh);
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;

struct nwo_ctx : bq::Ctx {
    // the samples (nwo_set_samples)
    int n = 0;
    int64_t n_used = 0;
    DevBuf xyz, normals, nq, bad, red;
    // the lattice (nwo_plan)
    bool planned = false;
    float lo[3] = {0, 0, 0}, h = 0;
    int depth = 0, used = 0;
    int64_t occ[NWO_MAX_DEPTH + 1] = {0};
    DevBuf mark;
    // the level at hand (nwo_level_begin)
    int level = 0;
    DevBuf acc, rhs, diag, chi, coarse;
    // the field (nwo_field)
    bool has_field = false;
    DevBuf F;
};

namespace {

#define NWO_HIP(call) BQ_HIP(call, NWO_ERR_NOMEM, NWO_ERR_HIP)

inline int64_t nodes_of(int level) { return (int64_t)1 << (3 * level); }

nwo_box box_of(const nwo_ctx *ctx, int level)
{
    nwo_box B;
    for (int d = 0; d < 3; ++d) B.lo[d] = ctx->lo[d];
    B.hl = nwo_spacing(ctx->h, ctx->depth, level);
    B.level = level;
    return B;
}

int level_begin(nwo_ctx *ctx, int level, double alpha)
{
    hipStream_t st = ctx->stream;
    const int64_t nodes = nodes_of(level);
    ctx->level = 0;
    ctx->has_field = false;
    if (level > NWO_BASE_LEVEL) {                                 // the chi at hand becomes the coarse one
        std::swap(ctx->chi.p, ctx->coarse.p);
        std::swap(ctx->chi.bytes, ctx->coarse.bytes);
    }
    NWO_HIP(ctx->acc.ensure(sizeof(u64) * 4 * (size_t)nodes));
    NWO_HIP(ctx->rhs.ensure(sizeof(double) * (size_t)nodes));
    NWO_HIP(ctx->diag.ensure(sizeof(double) * (size_t)nodes));
    NWO_HIP(ctx->chi.ensure(sizeof(double) * (size_t)nodes));
    NWO_HIP(hipMemsetAsync(ctx->acc.p, 0, sizeof(u64) * 4 * (size_t)nodes, st));
    if (level == NWO_LDS_LEVEL)
        hipLaunchKernelGGL(k_sp_splat_lds4, dim3(std::min(bq::nblk(ctx->n, NWO_BLOCK), NWO_LDS_GROUPS)), dim3(NWO_BLOCK), 0, st, ctx->xyz.as<float>(),
                           ctx->nq.as<short4>(), ctx->n, box_of(ctx, level), ctx->acc.as<u64>());
    else if (level < NWO_LDS_LEVEL)
        hipLaunchKernelGGL(k_sp_splat_lds, dim3(std::min(bq::nblk(ctx->n, NWO_BLOCK), NWO_LDS_GROUPS)), dim3(NWO_BLOCK), 0, st, ctx->xyz.as<float>(),
                           ctx->nq.as<short4>(), ctx->n, box_of(ctx, level), ctx->acc.as<u64>());
    else
        hipLaunchKernelGGL(k_sp_splat, dim3(bq::nblk(ctx->n, NWO_BLOCK)), dim3(NWO_BLOCK), 0, st, ctx->xyz.as<float>(), ctx->nq.as<short4>(), ctx->n,
                           box_of(ctx, level), ctx->acc.as<u64>());
    const double s = (double)(1 << (ctx->used - level));
    hipLaunchKernelGGL(k_sp_system, dim3(bq::nblk(nodes, NWO_BLOCK)), dim3(NWO_BLOCK), 0, st, ctx->acc.as<long long>(), level, alpha / s, 1.0 / (s * s),
                       ctx->rhs.as<double>(), ctx->diag.as<double>());
    if (level == NWO_BASE_LEVEL)
        NWO_HIP(hipMemsetAsync(ctx->chi.p, 0, sizeof(double) * (size_t)nodes, st));
    else
        hipLaunchKernelGGL(k_sp_prolong, dim3(bq::nblk(nodes, NWO_BLOCK)), dim3(NWO_BLOCK), 0, st, ctx->coarse.as<double>(), level, ctx->chi.as<double>());
    NWO_HIP(hipGetLastError());
    NWO_HIP(hipStreamSynchronize(st));
    ctx->level = level;
    return NWO_OK;
}

int relax(nwo_ctx *ctx, int sweeps, double *res_before, double *res_after)
{
    hipStream_t st = ctx->stream;
    const int level = ctx->level;
    const int64_t nodes = nodes_of(level);
    const dim3 all(bq::nblk(nodes, NWO_BLOCK)), half(bq::nblk(nodes / 2, NWO_BLOCK)), blk(NWO_BLOCK);
    double *chi = ctx->chi.as<double>();
    const double *rhs = ctx->rhs.as<double>(), *diag = ctx->diag.as<double>();
    NWO_HIP(ctx->red.ensure(sizeof(u64) * 4));
    NWO_HIP(hipMemsetAsync(ctx->red.p, 0, sizeof(u64) * 4, st));
    ctx->has_field = false;
    hipLaunchKernelGGL(k_sp_residual, all, blk, 0, st, chi, rhs, diag, level, ctx->red.as<u64>());
    for (int s = 0; s < sweeps; ++s) {
        hipLaunchKernelGGL(k_sp_relax, half, blk, 0, st, chi, rhs, diag, level, 0);
        hipLaunchKernelGGL(k_sp_relax, half, blk, 0, st, chi, rhs, diag, level, 1);
    }
    hipLaunchKernelGGL(k_sp_residual, all, blk, 0, st, chi, rhs, diag, level, ctx->red.as<u64>() + 1);
    NWO_HIP(hipGetLastError());
    double res[2];
    NWO_HIP(hipMemcpyAsync(res, ctx->red.p, sizeof(res), hipMemcpyDeviceToHost, st));
    NWO_HIP(hipStreamSynchronize(st));
    if (res_before) *res_before = res[0];
    if (res_after) *res_after = res[1];
    return NWO_OK;
}

}  // namespace

NWO_EXPORT int nwo_abi_version(void) { return NWO_ABI_VERSION; }

NWO_EXPORT int nwo_create(int device, nwo_ctx **out) { return bq::create(device, out, NWO_ERR_BADARG, NWO_ERR_HIP); }

NWO_EXPORT void nwo_destroy(nwo_ctx *ctx) { bq::destroy(ctx); }

NWO_EXPORT const char *nwo_last_error(nwo_ctx *ctx) { return bq::last_error(ctx); }

NWO_EXPORT int nwo_set_samples(nwo_ctx *ctx, const float *xyz, const float *normals, int64_t n, int on_device, int use_lengths, int64_t *n_used,
                               int64_t *n_skipped)
{
    if (!xyz || !normals || n < 1 || n > NWO_MAX_N || (on_device != 0 && on_device != 1) || (use_lengths != 0 && use_lengths != 1)) return NWO_ERR_BADARG;
    if (ctx) { ctx->n = 0; ctx->n_used = 0; ctx->planned = false; ctx->level = 0; ctx->has_field = false; }     // (a failed call leaves no samples)
    if (!on_device) {
        if (!bq::all_finite(xyz, 3 * n)) return fail(ctx, NWO_ERR_NONFINITE, "nwo_set_samples: a position is not finite");
        if (!bq::all_finite(normals, 3 * n)) return fail(ctx, NWO_ERR_NONFINITE, "nwo_set_samples: a normal is not finite");
        if (use_lengths)
            for (int64_t i = 0; i < 3 * n; ++i)
                if (std::fabs(normals[i]) > 1.0f) return fail(ctx, NWO_ERR_BADARG, "nwo_set_samples: a normal component above 1 with use_lengths");
    }
    if (!ctx) return NWO_ERR_BADARG;
    NWO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    NWO_HIP(ctx->xyz.ensure(sizeof(float) * 3 * (size_t)n));
    NWO_HIP(ctx->normals.ensure(sizeof(float) * 3 * (size_t)n));
    NWO_HIP(ctx->nq.ensure(sizeof(short4) * (size_t)n));
    NWO_HIP(ctx->bad.ensure(sizeof(int)));
    NWO_HIP(ctx->red.ensure(sizeof(u64) * 4));
    NWO_HIP(hipMemcpyAsync(ctx->xyz.p, xyz, sizeof(float) * 3 * (size_t)n, kind, st));
    NWO_HIP(hipMemcpyAsync(ctx->normals.p, normals, sizeof(float) * 3 * (size_t)n, kind, st));
    NWO_HIP(hipMemsetAsync(ctx->bad.p, 0, sizeof(int), st));
    NWO_HIP(hipMemsetAsync(ctx->red.p, 0, sizeof(u64) * 4, st));
    hipLaunchKernelGGL(k_sp_prepare, dim3(bq::nblk(n, NWO_BLOCK)), dim3(NWO_BLOCK), 0, st, ctx->xyz.as<float>(), ctx->normals.as<float>(), (int)n, use_lengths,
                       ctx->nq.as<short4>(), ctx->bad.as<int>(), ctx->red.as<u64>());
    NWO_HIP(hipGetLastError());
    int bad = 0;
    u64 used = 0;
    NWO_HIP(hipMemcpyAsync(&bad, ctx->bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    NWO_HIP(hipMemcpyAsync(&used, ctx->red.p, sizeof(u64), hipMemcpyDeviceToHost, st));
    NWO_HIP(hipStreamSynchronize(st));
    if (bad & NWO_BAD_NONFINITE) return fail(ctx, NWO_ERR_NONFINITE, "nwo_set_samples: a position or a normal is not finite");
    if (bad & NWO_BAD_LENGTH) return fail(ctx, NWO_ERR_BADARG, "nwo_set_samples: a normal component above 1 with use_lengths");
    if (n_used) *n_used = (int64_t)used;
    if (n_skipped) *n_skipped = n - (int64_t)used;
    if (used == 0) return fail(ctx, NWO_ERR_EMPTY, "nwo_set_samples: every normal has length 0");
    ctx->n = (int)n;
    ctx->n_used = (int64_t)used;
    return NWO_OK;
}

NWO_EXPORT int nwo_plan(nwo_ctx *ctx, const float *lo, float h, int depth, int fulldepth, double samples_per_node, int *depth_used, int64_t *occ)
{
    if (!lo || !depth_used || depth < NWO_MIN_DEPTH || depth > NWO_MAX_DEPTH || fulldepth < 0) return NWO_ERR_BADARG;
    if (!(h > 0.0f) || !std::isfinite(h) || !(samples_per_node >= 0.0) || !std::isfinite(samples_per_node)) return NWO_ERR_BADARG;
    if (!bq::all_finite(lo, 3)) return fail(ctx, NWO_ERR_NONFINITE, "nwo_plan: the lattice's origin is not finite");
    if (!std::isfinite(nwo_spacing(h, depth, NWO_BASE_LEVEL))) return NWO_ERR_BADARG;
    if (!ctx) return NWO_ERR_BADARG;
    if (ctx->n < 1) return fail(ctx, NWO_ERR_STATE, "nwo_plan: nwo_set_samples first");
    NWO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ctx->planned = false;
    ctx->level = 0;
    ctx->has_field = false;
    for (int d = 0; d < 3; ++d) ctx->lo[d] = lo[d];
    ctx->h = h;
    ctx->depth = depth;
    NWO_HIP(ctx->mark.ensure((size_t)nodes_of(depth)));
    NWO_HIP(ctx->red.ensure(sizeof(u64) * 4));
    u64 count[NWO_MAX_DEPTH + 1] = {0};
    for (int l = NWO_BASE_LEVEL; l <= depth; ++l) {
        const int64_t nodes = nodes_of(l);
        NWO_HIP(hipMemsetAsync(ctx->mark.p, 0, (size_t)nodes, st));
        NWO_HIP(hipMemsetAsync(ctx->red.p, 0, sizeof(u64), st));
        hipLaunchKernelGGL(k_sp_mark, dim3(bq::nblk(ctx->n, NWO_BLOCK)), dim3(NWO_BLOCK), 0, st, ctx->xyz.as<float>(), ctx->nq.as<short4>(), ctx->n, box_of(ctx, l),
                           ctx->mark.as<unsigned char>());
        hipLaunchKernelGGL(k_sp_count, dim3((unsigned)std::min<int64_t>(bq::nblk(nodes, NWO_BLOCK), 4096)), dim3(NWO_BLOCK), 0, st, ctx->mark.as<unsigned char>(),
                           nodes, ctx->red.as<u64>());
        NWO_HIP(hipGetLastError());
        NWO_HIP(hipMemcpyAsync(&count[l], ctx->red.p, sizeof(u64), hipMemcpyDeviceToHost, st));
        NWO_HIP(hipStreamSynchronize(st));
    }
    for (int l = 0; l <= NWO_MAX_DEPTH; ++l) ctx->occ[l] = l <= depth ? (int64_t)count[l] : 0;
    ctx->used = nwo_depth_used(ctx->n_used, ctx->occ, depth, fulldepth, samples_per_node);
    if (ctx->occ[ctx->used] < 1) return fail(ctx, NWO_ERR_HIP, "nwo_plan: the occupancy of the level used is zero");
    *depth_used = ctx->used;
    if (occ)
        for (int l = 0; l <= depth; ++l) occ[l] = ctx->occ[l];
    ctx->planned = true;
    return NWO_OK;
}

NWO_EXPORT int nwo_level_begin(nwo_ctx *ctx, int level, double alpha)
{
    if (level < NWO_BASE_LEVEL || level > NWO_MAX_DEPTH || !(alpha > 0.0) || !std::isfinite(alpha)) return NWO_ERR_BADARG;
    if (!ctx) return NWO_ERR_BADARG;
    if (!ctx->planned) return fail(ctx, NWO_ERR_STATE, "nwo_level_begin: nwo_plan first");
    if (level > ctx->used) return fail(ctx, NWO_ERR_BADARG, "nwo_level_begin: a level above the depth used");
    if (level > NWO_BASE_LEVEL && ctx->level != level - 1) return fail(ctx, NWO_ERR_STATE, "nwo_level_begin: the level below first");
    NWO_HIP(hipSetDevice(ctx->device));
    return level_begin(ctx, level, alpha);
}

NWO_EXPORT int nwo_relax(nwo_ctx *ctx, int sweeps, double *res_before, double *res_after)
{
    if (sweeps < 0) return NWO_ERR_BADARG;
    if (!ctx) return NWO_ERR_BADARG;
    if (ctx->level < NWO_BASE_LEVEL) return fail(ctx, NWO_ERR_STATE, "nwo_relax: nwo_level_begin first");
    NWO_HIP(hipSetDevice(ctx->device));
    return relax(ctx, sweeps, res_before, res_after);
}

NWO_EXPORT int nwo_get_level(nwo_ctx *ctx, int what, void *host_dst)
{
    if (!host_dst || what < NWO_GET_W || what > NWO_GET_CHI) return NWO_ERR_BADARG;
    if (!ctx) return NWO_ERR_BADARG;
    if (ctx->level < NWO_BASE_LEVEL) return fail(ctx, NWO_ERR_STATE, "nwo_get_level: nwo_level_begin first");
    NWO_HIP(hipSetDevice(ctx->device));
    const size_t plane = sizeof(u64) * (size_t)nodes_of(ctx->level);
    const void *src = what == NWO_GET_W ? ctx->acc.p : what == NWO_GET_V ? (const void *)(ctx->acc.as<char>() + plane) : what == NWO_GET_RHS ? ctx->rhs.p
                    : what == NWO_GET_DIAG ? ctx->diag.p : ctx->chi.p;
    NWO_HIP(hipMemcpyAsync(host_dst, src, what == NWO_GET_V ? 3 * plane : plane, hipMemcpyDeviceToHost, ctx->stream));
    NWO_HIP(hipStreamSynchronize(ctx->stream));
    return NWO_OK;
}

NWO_EXPORT int nwo_set_chi(nwo_ctx *ctx, const double *host_src)
{
    if (!host_src) return NWO_ERR_BADARG;
    if (!ctx) return NWO_ERR_BADARG;
    if (ctx->level < NWO_BASE_LEVEL) return fail(ctx, NWO_ERR_STATE, "nwo_set_chi: nwo_level_begin first");
    const int64_t nodes = nodes_of(ctx->level);
    if (!bq::all_finite(host_src, nodes)) return fail(ctx, NWO_ERR_NONFINITE, "nwo_set_chi: a value is not finite");
    NWO_HIP(hipSetDevice(ctx->device));
    ctx->has_field = false;
    NWO_HIP(hipMemcpyAsync(ctx->chi.p, host_src, sizeof(double) * (size_t)nodes, hipMemcpyHostToDevice, ctx->stream));
    NWO_HIP(hipStreamSynchronize(ctx->stream));
    return NWO_OK;
}

NWO_EXPORT int nwo_solve(nwo_ctx *ctx, double pointweight, int iters, int coarse_iters, double *alpha_out, double *residuals)
{
    if (!(pointweight > 0.0) || !std::isfinite(pointweight) || iters < 0 || coarse_iters < 0) return NWO_ERR_BADARG;
    if (!ctx) return NWO_ERR_BADARG;
    if (!ctx->planned) return fail(ctx, NWO_ERR_STATE, "nwo_solve: nwo_plan first");
    const double alpha = nwo_alpha(pointweight, ctx->occ[ctx->used], ctx->n_used);
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(ctx, NWO_ERR_BADARG, "nwo_solve: the screen's weight is not a positive number");
    NWO_HIP(hipSetDevice(ctx->device));
    if (alpha_out) *alpha_out = alpha;
    if (residuals)
        for (int k = 0; k < NWO_RESIDUAL_WORDS; ++k) residuals[k] = 0.0;
    for (int l = NWO_BASE_LEVEL; l <= ctx->used; ++l) {
        int rc = level_begin(ctx, l, alpha);
        if (rc != NWO_OK) return rc;
        double before = 0.0, after = 0.0;
        rc = relax(ctx, l == NWO_BASE_LEVEL ? coarse_iters : iters, &before, &after);
        if (rc != NWO_OK) return rc;
        if (residuals) { residuals[2 * l] = before; residuals[2 * l + 1] = after; }
    }
    return NWO_OK;
}

NWO_EXPORT int nwo_field(nwo_ctx *ctx, uint64_t *thr, double *E_out, uint64_t *sum_w)
{
    if (!ctx) return NWO_ERR_BADARG;
    if (!ctx->planned || ctx->level != ctx->used) return fail(ctx, NWO_ERR_STATE, "nwo_field: the level at hand is not the depth used");
    NWO_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t nodes = nodes_of(ctx->level);
    const dim3 all(bq::nblk(nodes, NWO_BLOCK)), blk(NWO_BLOCK);
    ctx->has_field = false;
    NWO_HIP(ctx->red.ensure(sizeof(u64) * 4));
    NWO_HIP(ctx->F.ensure(sizeof(u64) * (size_t)nodes));
    NWO_HIP(hipMemsetAsync(ctx->red.p, 0, sizeof(u64) * 4, st));
    hipLaunchKernelGGL(k_sp_absmax, all, blk, 0, st, ctx->chi.as<double>(), nodes, ctx->red.as<u64>());
    NWO_HIP(hipGetLastError());
    double M = 0.0;
    NWO_HIP(hipMemcpyAsync(&M, ctx->red.p, sizeof(double), hipMemcpyDeviceToHost, st));
    NWO_HIP(hipStreamSynchronize(st));
    if (!(M > 0.0) || !std::isfinite(M)) return fail(ctx, NWO_ERR_EMPTY, "nwo_field: the solution is zero everywhere (or not finite)");
    const double E = nwo_pow2_above(M);
    hipLaunchKernelGGL(k_sp_field, all, blk, 0, st, ctx->chi.as<double>(), ctx->acc.as<long long>(), nodes, E, ctx->F.as<u64>(), ctx->red.as<u64>() + 1);
    NWO_HIP(hipGetLastError());
    u64 sums[3];
    NWO_HIP(hipMemcpyAsync(sums, ctx->red.as<u64>() + 1, sizeof(sums), hipMemcpyDeviceToHost, st));
    NWO_HIP(hipStreamSynchronize(st));
    if (sums[0] != (u64)ctx->n_used << (3 * NWO_WEIGHT_BITS)) return fail(ctx, NWO_ERR_HIP, "nwo_field: the weights do not add up to the samples");
    if (thr) *thr = nwo_level(sums[1], sums[2], sums[0]);
    if (E_out) *E_out = E;
    if (sum_w) *sum_w = sums[0];
    ctx->has_field = true;
    return NWO_OK;
}

NWO_EXPORT const uint64_t *nwo_field_pointer(nwo_ctx *ctx) { return ctx && ctx->has_field ? ctx->F.as<uint64_t>() : nullptr; }

NWO_EXPORT int nwo_get_field(nwo_ctx *ctx, uint64_t *host_dst)
{
    if (!host_dst) return NWO_ERR_BADARG;
    if (!ctx) return NWO_ERR_BADARG;
    if (!ctx->has_field) return fail(ctx, NWO_ERR_STATE, "nwo_get_field: nwo_field first");
    NWO_HIP(hipSetDevice(ctx->device));
    NWO_HIP(hipMemcpyAsync(host_dst, ctx->F.p, sizeof(u64) * (size_t)nodes_of(ctx->used), hipMemcpyDeviceToHost, ctx->stream));
    NWO_HIP(hipStreamSynchronize(ctx->stream));
    return NWO_OK;
}
