// The level-set skeleton of a mesh on the device (MI355X, gfx950): include/nw_skeleton.h.
//
//   k_sk_bands     one lane per vertex: its band (and the nan / band-range flag); one lane per face: lo, hi and span from its corners'
//                  field; the workgroup's span sum, live faces, live vertices and largest band
//   k_sk_totals    the workgroups' four numbers, one workgroup; integer sums and a maximum: any order gives the same bits
//   bq::scan       piece_start = the exclusive scan of the spans (only after the 64-bit total has been checked against 2^28)
//   k_sk_init      one lane per piece: parent[p] = p, and the piece's face by a binary search in piece_start
//   k_sk_hook      one lane per half-edge h < twin[h] between two live faces: for every band of the edge's range the two faces' pieces are
//                  united in a lock-free union-find (find with path halving; the larger root is hooked under the smaller with a
//                  compare-and-swap, as k_pc_hook does), so a tree's root is its smallest piece
//   k_sk_compress  root of every piece, the root flags; bq::scan_total over the flags ranks the roots: nodes in the order of their
//                  smallest piece
//   k_sk_number    piece_node, and the band of a node from its root piece
//   k_sk_sums      one lane per piece: the piece's terms (nwa_piece_terms) into its node's row, 64-bit integer atomic adds whose results
//                  are not read
//   k_sk_arcs      one key per piece: (node(f, k), node(f, k + 1)) where the face has a band above k, all ones else
//   k_sk_vertex    one lane per corner of a live face: atomic min of the node of piece (f, b(v)) into vertex_node[v]
//
// No workgroup ever waits on another: there is no grid-wide barrier and no flag that another workgroup is spun on.  The loop of a hook
// ends because a failed compare-and-swap means some other lane's succeeded: the number of roots only falls.  Launches follow each other
// on one stream; a launch sees everything the launch before it wrote.
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it); every offset is 64 bits wide.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <chrono>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/nw_skeleton.h"
#include "nw_bq.h"
#include "nw_skeleton_core.h"

#define NWA_EXPORT extern "C" __attribute__((visibility("default")))
#define NWA_BLOCK 256
#define NWA_C_SEGMENTS 0
#define NWA_C_ARC_KEYS 1
#define NWA_C_RETRIES 2
#define NWA_C_ATOMICS 3
#define NWA_COUNTERS 4
#define NWA_NO_ARC 0xffffffffffffffffull

typedef unsigned long long u64;
typedef unsigned int u32;

static_assert(NWA_SUM_COLUMNS == NWA_S_COLUMNS, "the header's row width is the core's");

// the wave's sum into *dst with one atomic, if it is not zero
__device__ __forceinline__ void sk_wave_add(u32 x, u64 *dst)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, (u64)x);
}

// part[4 b + 0 .. 3] = the workgroup's span sum, live faces, live vertices, largest band + 1 (0: none)
__global__ __launch_bounds__(NWA_BLOCK) void k_sk_bands(const double *__restrict__ D, int nv, const int *__restrict__ faces, int nf, double w,
                                                        int *__restrict__ band, u32 *__restrict__ vertex_node, int *__restrict__ lo,
                                                        int *__restrict__ span, u64 *__restrict__ part, int *__restrict__ bad)
{
    __shared__ u64 s_sum[NWA_BLOCK / 64];
    __shared__ int s_max[NWA_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    bool flag = false;
    int live_v = 0, live_f = 0, top = 0;
    u64 sp = 0;
    if (i < nv) {
        const int b = nwa_band(D[i], w, &flag);
        band[i] = b;
        vertex_node[i] = 0xffffffffu;
        live_v = b >= 0 ? 1 : 0;
        top = b + 1;
    }
    if (i < nf) {
        bool ignore = false;                                      // (the corners' own lanes raise the flag)
        const int b0 = nwa_band(D[faces[3 * i]], w, &ignore), b1 = nwa_band(D[faces[3 * i + 1]], w, &ignore), b2 = nwa_band(D[faces[3 * i + 2]], w, &ignore);
        const nwa_face_bands fb = nwa_face(b0, b1, b2);
        lo[i] = fb.lo;
        span[i] = fb.span;
        live_f = fb.span > 0 ? 1 : 0;
        sp = (u64)fb.span;
    }
    if (flag) atomicOr(bad, 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sp += __shfl_xor(sp, o, 64);
        top = max(top, __shfl_xor(top, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sp; s_max[threadIdx.x >> 6] = top; }
    const int nlf = __syncthreads_count(live_f), nlv = __syncthreads_count(live_v);
    if (threadIdx.x == 0) {
        u64 t = 0;
        int m = 0;
        for (int k = 0; k < NWA_BLOCK / 64; ++k) { t += s_sum[k]; m = max(m, s_max[k]); }
        u64 *row = part + 4 * (int64_t)blockIdx.x;
        row[0] = t; row[1] = (u64)nlf; row[2] = (u64)nlv; row[3] = (u64)m;
    }
}

// totals[0 .. 2] = the sums of columns 0 .. 2 of part[nb][4], totals[3] = the maximum of column 3
__global__ __launch_bounds__(NWA_BLOCK) void k_sk_totals(const u64 *__restrict__ part, int64_t nb, u64 *__restrict__ totals)
{
    __shared__ u64 s_acc[NWA_BLOCK];
    const int c = threadIdx.x & 3, s = threadIdx.x >> 2, slices = NWA_BLOCK / 4;
    u64 acc = 0;
    for (int64_t b = s; b < nb; b += slices) {
        const u64 x = part[4 * b + c];
        acc = c == 3 ? (x > acc ? x : acc) : acc + x;
    }
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < 4) {
        u64 t = 0;
        for (int k = 0; k < slices; ++k) {
            const u64 x = s_acc[4 * k + threadIdx.x];
            t = threadIdx.x == 3 ? (x > t ? x : t) : t + x;
        }
        totals[threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(NWA_BLOCK) void k_sk_init(const int *__restrict__ piece_start, int nf, int np, int *__restrict__ parent, int *__restrict__ piece_face)
{
    const int64_t p = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    if (p >= np) return;
    parent[p] = (int)p;
    piece_face[p] = nwa_piece_face(piece_start, nf, (int)p);
}

// ---- union-find, as nw_clustering.hip's (ECL-CC) -------------------------------------------------------------------------------------
__device__ __forceinline__ int sk_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of v with path halving; parent[x] <= x always (hooking only ever lowers it), so the walk ends at the smallest index of the tree
__device__ int sk_find(int *parent, int v)
{
    int p = sk_load(&parent[v]);
    while (true) {
        const int gp = sk_load(&parent[p]);
        if (gp == p) return p;
        __hip_atomic_store(&parent[v], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (any ancestor is a valid parent)
        v = p;
        p = gp;
    }
}

__global__ __launch_bounds__(NWA_BLOCK) void k_sk_hook(const int *__restrict__ faces, const int *__restrict__ twin, int64_t nh, const int *__restrict__ band,
                                                       const int *__restrict__ lo, const int *__restrict__ span, const int *__restrict__ piece_start,
                                                       int *parent, u64 *__restrict__ counters)
{
    const int64_t h = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    u32 retries = 0, issued = 0;
    if (h < nh) {
        const int64_t t = twin[h];
        const int64_t f = h / 3, g = t / 3;
        if (t > h && span[f] > 0 && span[g] > 0) {
            int k0, k1;
            nwa_edge_range(band[faces[h]], band[faces[nwa_next(h)]], &k0, &k1);
            const int pf = piece_start[f] - lo[f], pg = piece_start[g] - lo[g];
            for (int k = k0; k <= k1; ++k) {
                int a = sk_find(parent, pf + k), b = sk_find(parent, pg + k);
                while (a != b) {
                    if (a > b) { const int s = a; a = b; b = s; }
                    // hook root b onto a; if b is no longer a root, climb from what it points to now
                    const int old = atomicCAS(&parent[b], b, a);
                    ++issued;
                    if (old == b) break;
                    ++retries;
                    b = sk_find(parent, old);
                }
            }
        }
    }
    sk_wave_add(retries, counters + NWA_C_RETRIES);
    sk_wave_add(issued, counters + NWA_C_ATOMICS);
}

// root[p] = the root of piece p (a separate array: concurrent path halving may still rewrite parent[])
__global__ __launch_bounds__(NWA_BLOCK) void k_sk_compress(int np, int *parent, int *__restrict__ root, int *__restrict__ is_root)
{
    const int64_t p = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    if (p >= np) return;
    const int r = sk_find(parent, (int)p);
    root[p] = r;
    is_root[p] = r == p ? 1 : 0;
}

__global__ __launch_bounds__(NWA_BLOCK) void k_sk_number(int np, const int *__restrict__ root, const int *__restrict__ rank, const int *__restrict__ piece_face,
                                                         const int *__restrict__ piece_start, const int *__restrict__ lo, int *__restrict__ piece_node,
                                                         int *__restrict__ node_band)
{
    const int64_t p = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    if (p >= np) return;
    const int r = root[p], n = rank[r];
    piece_node[p] = n;
    if (r == p) {
        const int f = piece_face[p];
        node_band[n] = lo[f] + ((int)p - piece_start[f]);
    }
}

__global__ __launch_bounds__(NWA_BLOCK) void k_sk_sums(int np, const float *__restrict__ pos, const double *__restrict__ D, const int *__restrict__ faces,
                                                       const int *__restrict__ piece_face, const int *__restrict__ piece_start, const int *__restrict__ lo,
                                                       const int *__restrict__ piece_node, double w, double low0, double low1, double low2, double q,
                                                       u64 *__restrict__ sums, u64 *__restrict__ counters)
{
    const int64_t p = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    u32 seg = 0;
    if (p < np) {
        const int f = piece_face[p];
        const int k = lo[f] + ((int)p - piece_start[f]);
        const int v[3] = {faces[3 * (int64_t)f], faces[3 * (int64_t)f + 1], faces[3 * (int64_t)f + 2]};
        const double low[3] = {low0, low1, low2};
        u64 add[NWA_S_COLUMNS];
        seg = nwa_piece_terms(pos, D, v, k, w, low, q, add) ? 1 : 0;
        u64 *row = sums + (int64_t)piece_node[p] * NWA_S_COLUMNS;
#pragma unroll
        for (int c = 0; c < NWA_S_SEGMENTS; ++c) atomicAdd(row + c, add[c]);
        if (seg) {
#pragma unroll
            for (int c = NWA_S_SEGMENTS; c < NWA_S_COLUMNS; ++c) atomicAdd(row + c, add[c]);
        }
    }
    sk_wave_add(seg, counters + NWA_C_SEGMENTS);
}

__global__ __launch_bounds__(NWA_BLOCK) void k_sk_arcs(int np, const int *__restrict__ piece_face, const int *__restrict__ piece_start, const int *__restrict__ piece_node,
                                                       u64 *__restrict__ keys, u64 *__restrict__ counters)
{
    const int64_t p = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    u32 has = 0;
    if (p < np) {
        // the piece above it in the same face, if the face has one
        has = (int)p + 1 < piece_start[piece_face[p] + 1] ? 1 : 0;
        keys[p] = has ? nwa_arc_key(piece_node[p], piece_node[p + 1]) : NWA_NO_ARC;
    }
    sk_wave_add(has, counters + NWA_C_ARC_KEYS);
}

__global__ __launch_bounds__(NWA_BLOCK) void k_sk_vertex(const int *__restrict__ faces, int64_t nh, const int *__restrict__ band, const int *__restrict__ lo,
                                                         const int *__restrict__ span, const int *__restrict__ piece_start, const int *__restrict__ piece_node,
                                                         u32 *__restrict__ vertex_node)
{
    const int64_t h = (int64_t)blockIdx.x * NWA_BLOCK + threadIdx.x;
    if (h >= nh) return;
    const int64_t f = h / 3;
    if (span[f] <= 0) return;
    const int v = faces[h];
    atomicMin(vertex_node + (int64_t)v, (u32)piece_node[piece_start[f] + (band[v] - lo[f])]);
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;

struct nwa_ctx : bq::Ctx {
    // the mesh (nwa_set_mesh): nv = 0 until then
    int nv = 0, nf = 0;
    double low[3] = {0, 0, 0}, q = 1.0;
    DevBuf pos, faces, twin;
    // one skeleton
    bool has_result = false;
    int np = 0, nn = 0;
    std::vector<int32_t> arcs;
    DevBuf field, band, vertex_node, lo, span, part, totals, flag, piece_start, scan_tmp, parent, piece_face, root, is_root, rank, piece_node,
        node_band, sums, keys, counters;
};

namespace {

#define NWA_HIP(call) BQ_HIP(call, NWA_ERR_NOMEM, NWA_ERR_HIP)

struct Stage {
    hipStream_t st;
    bool on;
    std::chrono::steady_clock::time_point t0;
    // the microseconds since the last mark into *word, the stream waited for first: only when timing is asked for
    hipError_t mark(int64_t *word)
    {
        if (!on) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(st);
        const auto t1 = std::chrono::steady_clock::now();
        *word += (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
        t0 = t1;
        return e;
    }
};

}  // namespace

NWA_EXPORT int nwa_abi_version(void) { return NWA_ABI_VERSION; }

NWA_EXPORT int nwa_create(int device, nwa_ctx **out) { return bq::create(device, out, NWA_ERR_BADARG, NWA_ERR_HIP); }

NWA_EXPORT void nwa_destroy(nwa_ctx *ctx) { bq::destroy(ctx); }

NWA_EXPORT const char *nwa_last_error(nwa_ctx *ctx) { return bq::last_error(ctx); }

NWA_EXPORT int nwa_set_mesh(nwa_ctx *ctx, const float *positions, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin, int on_device,
                            double *quantum_out)
{
    if (!positions || !faces || !twin || n_vertices < 1 || n_vertices > NWA_MAX_N || n_faces < 1 || n_faces > NWA_MAX_FACES || (on_device != 0 && on_device != 1))
        return NWA_ERR_BADARG;
    if (ctx) { ctx->nv = 0; ctx->has_result = false; }           // (a failed call leaves no mesh, whichever check failed)
    for (int64_t i = 0; i < 3 * n_faces; ++i)
        if (faces[i] < 0 || faces[i] >= n_vertices) return fail(ctx, NWA_ERR_BADARG, "nwa_set_mesh: a face names a vertex that is out of range");
    if (!nwa_twins_ok(faces, twin, n_faces)) return fail(ctx, NWA_ERR_BADARG, "nwa_set_mesh: the twin table is not mutual");
    double low[3], q = 1.0;
    if (!on_device && !nwa_box(positions, n_vertices, low, &q)) return fail(ctx, NWA_ERR_NONFINITE, "nwa_set_mesh: a position is not finite");
    if (!ctx) return NWA_ERR_BADARG;
    NWA_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t pos_bytes = sizeof(float) * 3 * (size_t)n_vertices;
    NWA_HIP(ctx->pos.ensure(pos_bytes));
    NWA_HIP(hipMemcpyAsync(ctx->pos.p, positions, pos_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    NWA_HIP(bq::upload(st, ctx->faces, faces, 3 * n_faces));
    NWA_HIP(bq::upload(st, ctx->twin, twin, 3 * n_faces));
    if (on_device) {
        std::vector<float> host(3 * (size_t)n_vertices);
        NWA_HIP(hipMemcpyAsync(host.data(), ctx->pos.p, pos_bytes, hipMemcpyDeviceToHost, st));
        NWA_HIP(hipStreamSynchronize(st));
        if (!nwa_box(host.data(), n_vertices, low, &q)) return fail(ctx, NWA_ERR_NONFINITE, "nwa_set_mesh: a position is not finite");
    }
    NWA_HIP(hipStreamSynchronize(st));
    ctx->nv = (int)n_vertices;
    ctx->nf = (int)n_faces;
    for (int c = 0; c < 3; ++c) ctx->low[c] = low[c];
    ctx->q = q;
    if (quantum_out) { quantum_out[0] = low[0]; quantum_out[1] = low[1]; quantum_out[2] = low[2]; quantum_out[3] = q; }
    return NWA_OK;
}

NWA_EXPORT int nwa_skeleton(nwa_ctx *ctx, const double *field, int on_device, double band_width, int flags, int64_t *info_out)
{
    if (!field || !info_out || (on_device != 0 && on_device != 1) || (flags & ~NWA_FLAG_TIMING)) return NWA_ERR_BADARG;
    if (!nwa_width_ok(band_width)) return fail(ctx, NWA_ERR_BADARG, "nwa_skeleton: the band width must be positive and finite");
    if (!ctx) return NWA_ERR_BADARG;
    ctx->has_result = false;
    if (ctx->nv < 1) return fail(ctx, NWA_ERR_NOMESH, "nwa_skeleton: nwa_set_mesh first");
    const int nv = ctx->nv, nf = ctx->nf;
    const int64_t nh = 3 * (int64_t)nf;
    if (!on_device && !nwa_field_ok(field, nv, band_width))
        return fail(ctx, NWA_ERR_BADARG, "nwa_skeleton: the field holds a nan or a band beyond 2^30 at band width " + std::to_string(band_width));
    NWA_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int64_t info[NWA_INFO_WORDS] = {0};
    Stage stage = {st, (flags & NWA_FLAG_TIMING) != 0, std::chrono::steady_clock::now()};

    const int nbvf = bq::nblk(std::max<int64_t>(nv, nf), NWA_BLOCK), nbh = bq::nblk(nh, NWA_BLOCK);
    NWA_HIP(ctx->field.ensure(sizeof(double) * (size_t)nv));
    NWA_HIP(hipMemcpyAsync(ctx->field.p, field, sizeof(double) * (size_t)nv, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    NWA_HIP(ctx->band.ensure(sizeof(int) * (size_t)nv));
    NWA_HIP(ctx->vertex_node.ensure(sizeof(u32) * (size_t)nv));
    NWA_HIP(ctx->lo.ensure(sizeof(int) * (size_t)nf));
    NWA_HIP(ctx->span.ensure(sizeof(int) * (size_t)nf));
    NWA_HIP(ctx->piece_start.ensure(sizeof(int) * ((size_t)nf + 1)));
    NWA_HIP(ctx->part.ensure(sizeof(u64) * 4 * (size_t)nbvf));
    NWA_HIP(ctx->totals.ensure(sizeof(u64) * 4));
    NWA_HIP(ctx->flag.ensure(sizeof(int)));
    NWA_HIP(ctx->counters.ensure(sizeof(u64) * NWA_COUNTERS));
    NWA_HIP(hipMemsetAsync(ctx->flag.p, 0, sizeof(int), st));
    NWA_HIP(hipMemsetAsync(ctx->counters.p, 0, sizeof(u64) * NWA_COUNTERS, st));
    NWA_HIP(stage.mark(&info[NWA_INFO_UPLOAD_US]));

    hipLaunchKernelGGL(k_sk_bands, dim3(nbvf), dim3(NWA_BLOCK), 0, st, ctx->field.as<double>(), nv, ctx->faces.as<int>(), nf, band_width, ctx->band.as<int>(),
                       ctx->vertex_node.as<u32>(), ctx->lo.as<int>(), ctx->span.as<int>(), ctx->part.as<u64>(), ctx->flag.as<int>());
    hipLaunchKernelGGL(k_sk_totals, dim3(1), dim3(NWA_BLOCK), 0, st, ctx->part.as<u64>(), (int64_t)nbvf, ctx->totals.as<u64>());
    NWA_HIP(hipGetLastError());
    u64 tot[4];
    int bad = 0;
    NWA_HIP(hipMemcpyAsync(tot, ctx->totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    NWA_HIP(hipMemcpyAsync(&bad, ctx->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    NWA_HIP(hipStreamSynchronize(st));
    NWA_HIP(stage.mark(&info[NWA_INFO_BANDS_US]));
    if (bad) return fail(ctx, NWA_ERR_BADARG, "nwa_skeleton: the field holds a nan or a band beyond 2^30 at band width " + std::to_string(band_width));
    if (tot[0] > (u64)NWA_MAX_PIECES)
        return fail(ctx, NWA_ERR_BADARG, "nwa_skeleton: " + std::to_string(tot[0]) + " pieces, more than 2^28: the band width " + std::to_string(band_width) +
                                             " is too small for this field");
    const int np = (int)tot[0];
    int nn = 0;
    NWA_HIP(bq::scan_exclusive(st, ctx->span.as<int>(), nf, ctx->piece_start.as<int>(), ctx->scan_tmp));
    NWA_HIP(stage.mark(&info[NWA_INFO_SCAN_US]));

    ctx->arcs.clear();
    if (np > 0) {
        const int nbp = bq::nblk(np, NWA_BLOCK);
        NWA_HIP(ctx->parent.ensure(sizeof(int) * (size_t)np));
        NWA_HIP(ctx->piece_face.ensure(sizeof(int) * (size_t)np));
        NWA_HIP(ctx->root.ensure(sizeof(int) * (size_t)np));
        NWA_HIP(ctx->is_root.ensure(sizeof(int) * (size_t)np));
        NWA_HIP(ctx->rank.ensure(sizeof(int) * ((size_t)np + 1)));
        NWA_HIP(ctx->piece_node.ensure(sizeof(int) * ((size_t)np + 1)));
        NWA_HIP(ctx->keys.ensure(sizeof(u64) * (size_t)np));
        hipLaunchKernelGGL(k_sk_init, dim3(nbp), dim3(NWA_BLOCK), 0, st, ctx->piece_start.as<int>(), nf, np, ctx->parent.as<int>(), ctx->piece_face.as<int>());
        NWA_HIP(hipGetLastError());
        NWA_HIP(stage.mark(&info[NWA_INFO_INIT_US]));
        hipLaunchKernelGGL(k_sk_hook, dim3(nbh), dim3(NWA_BLOCK), 0, st, ctx->faces.as<int>(), ctx->twin.as<int>(), nh, ctx->band.as<int>(), ctx->lo.as<int>(),
                           ctx->span.as<int>(), ctx->piece_start.as<int>(), ctx->parent.as<int>(), ctx->counters.as<u64>());
        NWA_HIP(hipGetLastError());
        NWA_HIP(stage.mark(&info[NWA_INFO_HOOK_US]));
        hipLaunchKernelGGL(k_sk_compress, dim3(nbp), dim3(NWA_BLOCK), 0, st, np, ctx->parent.as<int>(), ctx->root.as<int>(), ctx->is_root.as<int>());
        NWA_HIP(hipGetLastError());
        NWA_HIP(stage.mark(&info[NWA_INFO_COMPRESS_US]));
        NWA_HIP(bq::scan_total(st, ctx->is_root.as<int>(), np, ctx->rank.as<int>(), ctx->scan_tmp, &nn));
        NWA_HIP(stage.mark(&info[NWA_INFO_SCAN_US]));
        if (nn < 1 || nn > np) return fail(ctx, NWA_ERR_HIP, "nwa_skeleton: the root count is out of range");
        NWA_HIP(ctx->node_band.ensure(sizeof(int) * (size_t)nn));
        NWA_HIP(ctx->sums.ensure(sizeof(u64) * NWA_S_COLUMNS * (size_t)nn));
        NWA_HIP(hipMemsetAsync(ctx->sums.p, 0, sizeof(u64) * NWA_S_COLUMNS * (size_t)nn, st));
        hipLaunchKernelGGL(k_sk_number, dim3(nbp), dim3(NWA_BLOCK), 0, st, np, ctx->root.as<int>(), ctx->rank.as<int>(), ctx->piece_face.as<int>(),
                           ctx->piece_start.as<int>(), ctx->lo.as<int>(), ctx->piece_node.as<int>(), ctx->node_band.as<int>());
        NWA_HIP(hipGetLastError());
        NWA_HIP(stage.mark(&info[NWA_INFO_COMPRESS_US]));
        hipLaunchKernelGGL(k_sk_sums, dim3(nbp), dim3(NWA_BLOCK), 0, st, np, ctx->pos.as<float>(), ctx->field.as<double>(), ctx->faces.as<int>(),
                           ctx->piece_face.as<int>(), ctx->piece_start.as<int>(), ctx->lo.as<int>(), ctx->piece_node.as<int>(), band_width, ctx->low[0], ctx->low[1],
                           ctx->low[2], ctx->q, ctx->sums.as<u64>(), ctx->counters.as<u64>());
        NWA_HIP(hipGetLastError());
        NWA_HIP(stage.mark(&info[NWA_INFO_SUMS_US]));
        hipLaunchKernelGGL(k_sk_arcs, dim3(nbp), dim3(NWA_BLOCK), 0, st, np, ctx->piece_face.as<int>(), ctx->piece_start.as<int>(), ctx->piece_node.as<int>(),
                           ctx->keys.as<u64>(), ctx->counters.as<u64>());
        NWA_HIP(hipGetLastError());
        NWA_HIP(stage.mark(&info[NWA_INFO_ARCS_US]));
        hipLaunchKernelGGL(k_sk_vertex, dim3(nbh), dim3(NWA_BLOCK), 0, st, ctx->faces.as<int>(), nh, ctx->band.as<int>(), ctx->lo.as<int>(), ctx->span.as<int>(),
                           ctx->piece_start.as<int>(), ctx->piece_node.as<int>(), ctx->vertex_node.as<u32>());
        NWA_HIP(hipGetLastError());
        NWA_HIP(stage.mark(&info[NWA_INFO_VERTEX_US]));
        // the arc keys: down, sorted, made distinct
        std::vector<u64> keys((size_t)np);
        NWA_HIP(hipMemcpyAsync(keys.data(), ctx->keys.p, sizeof(u64) * (size_t)np, hipMemcpyDeviceToHost, st));
        NWA_HIP(hipStreamSynchronize(st));
        NWA_HIP(stage.mark(&info[NWA_INFO_KEYS_DOWNLOAD_US]));
        keys.erase(std::remove(keys.begin(), keys.end(), (u64)NWA_NO_ARC), keys.end());
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
        ctx->arcs.resize(2 * keys.size());
        for (size_t i = 0; i < keys.size(); ++i) {
            ctx->arcs[2 * i] = (int32_t)(keys[i] >> 32);
            ctx->arcs[2 * i + 1] = (int32_t)(keys[i] & 0xffffffffull);
        }
        NWA_HIP(stage.mark(&info[NWA_INFO_DEDUP_US]));
    }
    u64 cnt[NWA_COUNTERS];
    NWA_HIP(hipMemcpyAsync(cnt, ctx->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    NWA_HIP(hipStreamSynchronize(st));
    ctx->np = np;
    ctx->nn = nn;
    ctx->has_result = true;
    info[NWA_INFO_PIECES] = np;
    info[NWA_INFO_NODES] = nn;
    info[NWA_INFO_ARCS] = (int64_t)(ctx->arcs.size() / 2);
    info[NWA_INFO_LIVE_FACES] = (int64_t)tot[1];
    info[NWA_INFO_LIVE_VERTICES] = (int64_t)tot[2];
    info[NWA_INFO_SEGMENTS] = (int64_t)cnt[NWA_C_SEGMENTS];
    info[NWA_INFO_MAX_BAND] = (int64_t)tot[3] - 1;
    info[NWA_INFO_ARC_KEYS] = (int64_t)cnt[NWA_C_ARC_KEYS];
    info[NWA_INFO_HOOK_RETRIES] = (int64_t)cnt[NWA_C_RETRIES];
    info[NWA_INFO_ATOMICS] = (int64_t)cnt[NWA_C_ATOMICS];
    for (int i = 0; i < NWA_INFO_WORDS; ++i) info_out[i] = info[i];
    return NWA_OK;
}

NWA_EXPORT int nwa_fetch(nwa_ctx *ctx, int32_t *piece_start, int32_t *piece_node, int32_t *vertex_node, int32_t *node_band, uint64_t *node_sums, int32_t *arcs)
{
    if (!ctx) return NWA_ERR_BADARG;
    if (!ctx->has_result) return fail(ctx, NWA_ERR_NORESULT, "nwa_fetch: nwa_skeleton first");
    NWA_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t np = (size_t)ctx->np, nn = (size_t)ctx->nn;
    if (piece_start) NWA_HIP(hipMemcpyAsync(piece_start, ctx->piece_start.p, sizeof(int) * ((size_t)ctx->nf + 1), hipMemcpyDeviceToHost, st));
    if (vertex_node) NWA_HIP(hipMemcpyAsync(vertex_node, ctx->vertex_node.p, sizeof(int) * (size_t)ctx->nv, hipMemcpyDeviceToHost, st));
    if (piece_node && np) NWA_HIP(hipMemcpyAsync(piece_node, ctx->piece_node.p, sizeof(int) * np, hipMemcpyDeviceToHost, st));
    if (node_band && nn) NWA_HIP(hipMemcpyAsync(node_band, ctx->node_band.p, sizeof(int) * nn, hipMemcpyDeviceToHost, st));
    if (node_sums && nn) NWA_HIP(hipMemcpyAsync(node_sums, ctx->sums.p, sizeof(u64) * NWA_S_COLUMNS * nn, hipMemcpyDeviceToHost, st));
    NWA_HIP(hipStreamSynchronize(st));
    if (arcs) std::copy(ctx->arcs.begin(), ctx->arcs.end(), arcs);
    return NWA_OK;
}
