// The geodesic graph distance on a mesh on the device (MI355X, gfx950): include/nw_geodesic.h.
//
//   k_gd_weights   one lane per half-edge: the edge's weight; of an interior pair the lane that owns the canonical orientation also
//                  computes the diagonal and writes it (+inf for none) into both half-edges' slots; which arc the lane relaxes later
//                  (nwt_halfedge_setup).  One lane per vertex checks that a position handed over by device pointer is finite
//   k_gd_seed      four phases of one kernel, each a launch: D = +inf and no stamp everywhere; the sources into D with a 64-bit unsigned
//                  atomic min on the double's bits; S = none everywhere; the sources whose d0 is their vertex's D into S
//   k_gd_relax     one round: one lane per half-edge relaxes its arc (nwt_lane_arc: an edge or a diagonal) in both directions, if one
//                  of the arc's two vertices was lowered in the round before.  D is read with 64-bit loads that bypass the L1, the
//                  atomic min is issued only for a strictly smaller candidate, a lowered vertex gets the round's stamp, and a
//                  workgroup one of whose atomics lowered a value sets the round's changed word and sweeps its own half-edges again
//                  (up to NWT_SWEEPS times, __syncthreads between the sweeps)
//   k_gd_labels    one round of the label rule on the final D, in the same shape
//   k_gd_finish    the cap: distance_out and source_out, and the workgroup's counts of reached and in-band vertices
//   k_gd_totals    the workgroups' counts, one workgroup; integer sums: any order gives the same bits
//
// Why rounds over all half-edges and not a work list: see DESIGN.md.  No workgroup ever waits on another: there is no grid-wide barrier,
// no flag another workgroup is spun on and no persistent kernel; rounds are launches, and a launch sees everything the launch before it
// wrote.  Within a launch a lane may read a value that is no longer the latest: it is then an older, larger one, the lane relaxes less
// than it could, and the vertex's stamp brings the arc back in the next round.  The fixed point does not depend on any of it (proof in
// csrc/nw_geodesic_core.h).
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it); every offset is 64 bits wide.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <string>
#include <algorithm>

#include "../../include/nw_geodesic.h"
#include "nw_bq.h"
#include "nw_geodesic_core.h"

#define NWT_EXPORT extern "C" __attribute__((visibility("default")))
#define NWT_BLOCK 256
// the counters a round adds to
#define NWT_C_LOWERED 0
#define NWT_C_RELAXED 1
#define NWT_COUNTERS 2
#define NWT_INF_BITS 0x7ff0000000000000ull

typedef unsigned long long u64;
typedef unsigned int u32;

// loads that are served by the L2, where the atomics of this launch's other lanes land
__device__ __forceinline__ double gd_load(const u64 *D, int v)
{
    return __builtin_bit_cast(double, __hip_atomic_load(D + (int64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ int gd_load(const int *a, int v) { return __hip_atomic_load(a + (int64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the wave's sum into *dst with one atomic, if it is not zero
__device__ __forceinline__ u32 gd_wave_add(u32 x, u64 *dst)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(dst, (u64)x);
    return x;
}

// (eight waves per SIMD asked for: left alone the allocator takes 66 registers for the two unfolded corners)
__global__ __launch_bounds__(NWT_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_gd_weights(const float *__restrict__ pos, int nv, const int *__restrict__ faces, const int *__restrict__ twin,
                                                          int64_t nh, double *__restrict__ we, double *__restrict__ wd, int *__restrict__ other,
                                                          u64 *__restrict__ part_diag, int *__restrict__ bad /* bit 0: a non-finite position */)
{
    const int64_t h = (int64_t)blockIdx.x * NWT_BLOCK + threadIdx.x;
    if (h < nv && !(isfinite(pos[3 * h]) && isfinite(pos[3 * h + 1]) && isfinite(pos[3 * h + 2]))) atomicOr(bad, 1);
    int exists = 0;
    if (h < nh) {
        const nwt_halfedge r = nwt_halfedge_setup(pos, faces, twin, h);
        we[h] = r.we;
        other[h] = r.other;
        if (r.wd_valid) {
            wd[h] = r.wd;
            wd[(int64_t)twin[h]] = r.wd;
            exists = r.wd < INFINITY ? 1 : 0;
        } else if (r.other == NWT_EDGE_ALONE) {
            wd[h] = INFINITY;
        }
    }
    const int n = __syncthreads_count(exists);
    if (threadIdx.x == 0) part_diag[blockIdx.x] = (u64)n;
}

__global__ __launch_bounds__(NWT_BLOCK) void k_gd_seed(int phase, u64 *__restrict__ D, int *__restrict__ S, int *__restrict__ stamp, int nv,
                                                       const int *__restrict__ ids, const double *__restrict__ d0, int ns)
{
    const int64_t i = (int64_t)blockIdx.x * NWT_BLOCK + threadIdx.x;
    if (phase == 0) {
        if (i < nv) { D[i] = NWT_INF_BITS; stamp[i] = -1; }
    } else if (phase == 2) {
        if (i < nv) S[i] = NWT_LABEL_NONE;
    } else if (i < ns) {
        const int v = ids[i];
        const u64 start = __builtin_bit_cast(u64, nwt_start_value(d0 ? d0[i] : 0.0));
        if (phase == 1) {
            atomicMin(D + (int64_t)v, start);
            stamp[v] = 0;
        } else if (D[v] == start) {
            atomicMin(S + (int64_t)v, (int)i);
        }
    }
}

__global__ __launch_bounds__(NWT_BLOCK) void k_gd_relax(const int *__restrict__ faces, const int *__restrict__ other, const double *__restrict__ we,
                                                        const double *__restrict__ wd, int64_t nh, int diagonals, double d_cap, u64 *D, int *stamp,
                                                        int round, int *__restrict__ changed, u64 *__restrict__ counters)
{
    const int64_t h = (int64_t)blockIdx.x * NWT_BLOCK + threadIdx.x;
    int p = 0, q = 0;
    double w = 0.0;
    const bool has = h < nh && nwt_lane_arc(faces, other, we, wd, h, diagonals != 0, &p, &q, &w);
    u32 lowered = 0, relaxed = 0;
    for (int sweep = 0; sweep < NWT_SWEEPS; ++sweep) {
        // the first sweep takes what the round before lowered, a later one what this round has lowered so far
        const int since = sweep == 0 ? round - 1 : round;
        int low = 0;
        if (has && (gd_load(stamp, p) >= since || gd_load(stamp, q) >= since)) {
            ++relaxed;
            const double Dp = gd_load(D, p), Dq = gd_load(D, q);
            double cand;
            if (nwt_relax(Dp, w, d_cap, Dq, &cand)) {
                const u64 c = __builtin_bit_cast(u64, cand);
                if (atomicMin(D + (int64_t)q, c) > c) { ++low; __hip_atomic_store(stamp + (int64_t)q, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            }
            if (nwt_relax(Dq, w, d_cap, Dp, &cand)) {
                const u64 c = __builtin_bit_cast(u64, cand);
                if (atomicMin(D + (int64_t)p, c) > c) { ++low; __hip_atomic_store(stamp + (int64_t)p, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            }
        }
        lowered += (u32)low;
        if (!__syncthreads_or(low)) break;
    }
    if (gd_wave_add(lowered, counters + NWT_C_LOWERED) && (threadIdx.x & 63) == 0) __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    gd_wave_add(relaxed, counters + NWT_C_RELAXED);
}

__global__ __launch_bounds__(NWT_BLOCK) void k_gd_labels(const int *__restrict__ faces, const int *__restrict__ other, const double *__restrict__ we,
                                                         const double *__restrict__ wd, int64_t nh, int diagonals, double d_cap, const u64 *__restrict__ D,
                                                         int *S, int *__restrict__ changed, u64 *__restrict__ counters)
{
    const int64_t h = (int64_t)blockIdx.x * NWT_BLOCK + threadIdx.x;
    int p = 0, q = 0;
    double w = 0.0;
    bool pq = false, qp = false;                              // whether p -> q, q -> p are tight: D is final
    if (h < nh && nwt_lane_arc(faces, other, we, wd, h, diagonals != 0, &p, &q, &w)) {
        const double Dp = __builtin_bit_cast(double, D[p]), Dq = __builtin_bit_cast(double, D[q]);
        pq = nwt_tight(Dp, w, d_cap, Dq);
        qp = nwt_tight(Dq, w, d_cap, Dp);
    }
    u32 lowered = 0, relaxed = 0;
    for (int sweep = 0; sweep < NWT_SWEEPS; ++sweep) {
        int low = 0;
        if (pq || qp) {
            ++relaxed;
            const int Sp = gd_load(S, p), Sq = gd_load(S, q);
            if (pq && Sp < Sq && atomicMin(S + (int64_t)q, Sp) > Sp) ++low;
            if (qp && Sq < Sp && atomicMin(S + (int64_t)p, Sq) > Sq) ++low;
        }
        lowered += (u32)low;
        if (!__syncthreads_or(low)) break;
    }
    if (gd_wave_add(lowered, counters + NWT_C_LOWERED)) __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    gd_wave_add(relaxed, counters + NWT_C_RELAXED);
}

// part[2 b] = the workgroup's vertices with D < +inf, part[2 b + 1] = those with D <= d_cap among them
__global__ __launch_bounds__(NWT_BLOCK) void k_gd_finish(const u64 *__restrict__ D, const int *__restrict__ S, int nv, double d_cap, double *__restrict__ dist_out,
                                                         int *__restrict__ src_out, u64 *__restrict__ part)
{
    const int64_t i = (int64_t)blockIdx.x * NWT_BLOCK + threadIdx.x;
    int reached = 0, in_band = 0;
    if (i < nv) {
        const double d = __builtin_bit_cast(double, D[i]);
        reached = d < INFINITY ? 1 : 0;
        in_band = reached && d <= d_cap ? 1 : 0;
        dist_out[i] = in_band ? d : INFINITY;
        if (S) {
            const int s = S[i];
            src_out[i] = in_band && s != NWT_LABEL_NONE ? s : -1;
        }
    }
    const int nr = __syncthreads_count(reached), nb = __syncthreads_count(in_band);
    if (threadIdx.x == 0) { part[2 * (int64_t)blockIdx.x] = (u64)nr; part[2 * (int64_t)blockIdx.x + 1] = (u64)nb; }
}

// totals[c] = the sum of column c of part[nb][width], width 1 or 2: a thread adds every (NWT_BLOCK / width)-th row of its column, then the
// column's threads are added in order
__global__ __launch_bounds__(NWT_BLOCK) void k_gd_totals(const u64 *__restrict__ part, int64_t nb, int width, u64 *__restrict__ totals)
{
    __shared__ u64 s_acc[NWT_BLOCK];
    const int c = threadIdx.x % width, s = threadIdx.x / width, slices = NWT_BLOCK / width;
    u64 acc = 0;
    for (int64_t b = s; b < nb; b += slices) acc += part[b * width + c];
    s_acc[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < width) {
        u64 t = 0;
        for (int k = 0; k < slices; ++k) t += s_acc[k * width + threadIdx.x];
        totals[threadIdx.x] = t;
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;

struct nwt_ctx : bq::Ctx {
    // the mesh (nwt_set_mesh): nv = 0 until then
    int nv = 0;
    int64_t nh = 0;
    bool has_twin = false;
    int64_t n_diag = 0;
    DevBuf pos, faces, twin, we, wd, other, flag;
    // one field
    DevBuf ids, d0, D, S, stamp, changed, counters, part, totals, dist, src;
};

namespace {

#define NWT_HIP(call) BQ_HIP(call, NWT_ERR_NOMEM, NWT_ERR_HIP)

// Rounds of `launch(round, changed word)` until one changes nothing, the changed words read once per NWT_BATCH rounds.  A fixed point is
// reached within nv rounds (core header, (3)), so a batch is never started after nv + NWT_BATCH rounds.
template <class Launch> int run_rounds(nwt_ctx *ctx, Launch launch, int64_t *rounds, const char *what)
{
    hipStream_t st = ctx->stream;
    int h_changed[NWT_BATCH];
    for (*rounds = 0;;) {
        if (*rounds >= (int64_t)ctx->nv + NWT_BATCH) return fail(ctx, NWT_ERR_INTERNAL, std::string(what) + ": no fixed point within n_vertices + NWT_BATCH rounds");
        NWT_HIP(hipMemsetAsync(ctx->changed.p, 0, sizeof(int) * NWT_BATCH, st));
        for (int i = 0; i < NWT_BATCH; ++i) launch((int)(++*rounds), ctx->changed.as<int>() + i);
        NWT_HIP(hipGetLastError());
        NWT_HIP(hipMemcpyAsync(h_changed, ctx->changed.p, sizeof(h_changed), hipMemcpyDeviceToHost, st));
        NWT_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < NWT_BATCH; ++i)
            if (!h_changed[i]) return NWT_OK;
    }
}

}  // namespace

NWT_EXPORT int nwt_abi_version(void) { return NWT_ABI_VERSION; }

NWT_EXPORT int nwt_create(int device, nwt_ctx **out) { return bq::create(device, out, NWT_ERR_BADARG, NWT_ERR_HIP); }

NWT_EXPORT void nwt_destroy(nwt_ctx *ctx) { bq::destroy(ctx); }

NWT_EXPORT const char *nwt_last_error(nwt_ctx *ctx) { return bq::last_error(ctx); }

NWT_EXPORT int nwt_set_mesh(nwt_ctx *ctx, const float *positions, int64_t n_vertices, const int32_t *faces, int64_t n_faces, const int32_t *twin, int on_device)
{
    if (!positions || !faces || n_vertices < 1 || n_vertices > NWT_MAX_N || n_faces < 1 || n_faces > NWT_MAX_FACES || (on_device != 0 && on_device != 1))
        return NWT_ERR_BADARG;
    if (ctx) ctx->nv = 0;                                         // (a failed call leaves no mesh, whichever check failed)
    for (int64_t i = 0; i < 3 * n_faces; ++i)
        if (faces[i] < 0 || faces[i] >= n_vertices) return fail(ctx, NWT_ERR_BADARG, "nwt_set_mesh: a face names a vertex that is out of range");
    if (twin && !nwt_twins_ok(faces, twin, n_faces)) return fail(ctx, NWT_ERR_BADARG, "nwt_set_mesh: the twin table is not mutual");
    if (!on_device && !bq::all_finite(positions, 3 * n_vertices)) return fail(ctx, NWT_ERR_NONFINITE, "nwt_set_mesh: a position is not finite");
    if (!ctx) return NWT_ERR_BADARG;
    NWT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t nh = 3 * n_faces;
    const int nb = bq::nblk(std::max(nh, n_vertices), NWT_BLOCK);
    NWT_HIP(ctx->pos.ensure(sizeof(float) * 3 * (size_t)n_vertices));
    NWT_HIP(hipMemcpyAsync(ctx->pos.p, positions, sizeof(float) * 3 * (size_t)n_vertices, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    NWT_HIP(bq::upload(st, ctx->faces, faces, nh));
    if (twin) NWT_HIP(bq::upload(st, ctx->twin, twin, nh));
    NWT_HIP(ctx->we.ensure(sizeof(double) * (size_t)nh));
    NWT_HIP(ctx->wd.ensure(sizeof(double) * (size_t)nh));
    NWT_HIP(ctx->other.ensure(sizeof(int) * (size_t)nh));
    NWT_HIP(ctx->part.ensure(sizeof(u64) * 2 * (size_t)nb));
    NWT_HIP(ctx->totals.ensure(sizeof(u64) * 2));
    NWT_HIP(ctx->flag.ensure(sizeof(int)));
    NWT_HIP(hipMemsetAsync(ctx->flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_gd_weights, dim3(nb), dim3(NWT_BLOCK), 0, st, ctx->pos.as<float>(), (int)n_vertices, ctx->faces.as<int>(),
                       twin ? ctx->twin.as<int>() : (const int *)nullptr, nh, ctx->we.as<double>(), ctx->wd.as<double>(), ctx->other.as<int>(), ctx->part.as<u64>(),
                       ctx->flag.as<int>());
    hipLaunchKernelGGL(k_gd_totals, dim3(1), dim3(NWT_BLOCK), 0, st, ctx->part.as<u64>(), (int64_t)nb, 1, ctx->totals.as<u64>());
    NWT_HIP(hipGetLastError());
    u64 n_diag = 0;
    int bad = 0;
    NWT_HIP(hipMemcpyAsync(&n_diag, ctx->totals.p, sizeof(u64), hipMemcpyDeviceToHost, st));
    NWT_HIP(hipMemcpyAsync(&bad, ctx->flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    NWT_HIP(hipStreamSynchronize(st));
    if (bad) return fail(ctx, NWT_ERR_NONFINITE, "nwt_set_mesh: a position is not finite");
    ctx->nv = (int)n_vertices;
    ctx->nh = nh;
    ctx->has_twin = twin != nullptr;
    ctx->n_diag = (int64_t)n_diag;
    return NWT_OK;
}

NWT_EXPORT int nwt_distances(nwt_ctx *ctx, const int32_t *source_ids, const double *source_d0, int64_t n_sources, double d_cap, int flags, double *distance_out,
                             int32_t *source_out, int64_t *info_out)
{
    if (!distance_out || !info_out || (flags & ~NWT_FLAG_DIAGONALS)) return NWT_ERR_BADARG;
    if (!nwt_cap_ok(d_cap)) return fail(ctx, NWT_ERR_BADARG, "nwt_distances: d_cap must be positive (+inf allowed)");
    if (!nwt_sources_ok(source_ids, source_d0, n_sources, ctx && ctx->nv > 0 ? ctx->nv : -1))
        return fail(ctx, NWT_ERR_BADARG, "nwt_distances: 1 to 2^30 sources, ids within the mesh, d0 finite and not negative");
    if (!ctx) return NWT_ERR_BADARG;
    if (ctx->nv < 1) return fail(ctx, NWT_ERR_NOMESH, "nwt_distances: nwt_set_mesh first");
    const int diagonals = (flags & NWT_FLAG_DIAGONALS) ? 1 : 0;
    if (diagonals && !ctx->has_twin) return fail(ctx, NWT_ERR_BADARG, "nwt_distances: diagonals need the twin table (nwt_set_mesh)");
    NWT_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int nv = ctx->nv, ns = (int)n_sources;
    const int64_t nh = ctx->nh;
    const int nbv = bq::nblk(nv, NWT_BLOCK), nbs = bq::nblk(ns, NWT_BLOCK), nbh = bq::nblk(nh, NWT_BLOCK);
    int64_t launches = 0;

    NWT_HIP(bq::upload(st, ctx->ids, source_ids, n_sources));
    if (source_d0) NWT_HIP(bq::upload(st, ctx->d0, source_d0, n_sources));
    NWT_HIP(ctx->D.ensure(sizeof(u64) * (size_t)nv));
    NWT_HIP(ctx->stamp.ensure(sizeof(int) * (size_t)nv));
    if (source_out) {
        NWT_HIP(ctx->S.ensure(sizeof(int) * (size_t)nv));
        NWT_HIP(ctx->src.ensure(sizeof(int) * (size_t)nv));
    }
    NWT_HIP(ctx->dist.ensure(sizeof(double) * (size_t)nv));
    NWT_HIP(ctx->changed.ensure(sizeof(int) * NWT_BATCH));
    NWT_HIP(ctx->counters.ensure(sizeof(u64) * NWT_COUNTERS));
    NWT_HIP(ctx->part.ensure(sizeof(u64) * 2 * (size_t)nbv));
    NWT_HIP(ctx->totals.ensure(sizeof(u64) * 2));
    NWT_HIP(hipMemsetAsync(ctx->counters.p, 0, sizeof(u64) * NWT_COUNTERS, st));
    const double *d0 = source_d0 ? ctx->d0.as<double>() : (const double *)nullptr;
    int *S = source_out ? ctx->S.as<int>() : (int *)nullptr;

    auto seed = [&](int phase, int blocks) {
        hipLaunchKernelGGL(k_gd_seed, dim3(blocks), dim3(NWT_BLOCK), 0, st, phase, ctx->D.as<u64>(), S, ctx->stamp.as<int>(), nv, ctx->ids.as<int>(), d0, ns);
        ++launches;
    };
    seed(0, nbv);
    seed(1, nbs);
    int64_t rounds = 0, label_rounds = 0;
    int r = run_rounds(ctx, [&](int round, int *changed) {
        hipLaunchKernelGGL(k_gd_relax, dim3(nbh), dim3(NWT_BLOCK), 0, st, ctx->faces.as<int>(), ctx->other.as<int>(), ctx->we.as<double>(), ctx->wd.as<double>(), nh,
                           diagonals, d_cap, ctx->D.as<u64>(), ctx->stamp.as<int>(), round, changed, ctx->counters.as<u64>());
        ++launches;
    }, &rounds, "nwt_distances");
    if (r != NWT_OK) return r;
    if (source_out) {
        seed(2, nbv);
        seed(3, nbs);
        r = run_rounds(ctx, [&](int, int *changed) {
            hipLaunchKernelGGL(k_gd_labels, dim3(nbh), dim3(NWT_BLOCK), 0, st, ctx->faces.as<int>(), ctx->other.as<int>(), ctx->we.as<double>(), ctx->wd.as<double>(),
                               nh, diagonals, d_cap, ctx->D.as<u64>(), S, changed, ctx->counters.as<u64>());
            ++launches;
        }, &label_rounds, "nwt_distances (labels)");
        if (r != NWT_OK) return r;
    }
    hipLaunchKernelGGL(k_gd_finish, dim3(nbv), dim3(NWT_BLOCK), 0, st, ctx->D.as<u64>(), S, nv, d_cap, ctx->dist.as<double>(),
                       source_out ? ctx->src.as<int>() : (int *)nullptr, ctx->part.as<u64>());
    hipLaunchKernelGGL(k_gd_totals, dim3(1), dim3(NWT_BLOCK), 0, st, ctx->part.as<u64>(), (int64_t)nbv, 2, ctx->totals.as<u64>());
    launches += 2;
    NWT_HIP(hipGetLastError());

    u64 tot[2], cnt[NWT_COUNTERS];
    NWT_HIP(hipMemcpyAsync(tot, ctx->totals.p, sizeof(tot), hipMemcpyDeviceToHost, st));
    NWT_HIP(hipMemcpyAsync(cnt, ctx->counters.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    NWT_HIP(hipMemcpyAsync(distance_out, ctx->dist.p, sizeof(double) * (size_t)nv, hipMemcpyDeviceToHost, st));
    if (source_out) NWT_HIP(hipMemcpyAsync(source_out, ctx->src.p, sizeof(int) * (size_t)nv, hipMemcpyDeviceToHost, st));
    NWT_HIP(hipStreamSynchronize(st));
    info_out[NWT_INFO_HALFEDGES] = nh;
    info_out[NWT_INFO_DIAGONALS] = diagonals ? ctx->n_diag : 0;
    info_out[NWT_INFO_REACHED] = (int64_t)tot[0];
    info_out[NWT_INFO_IN_BAND] = (int64_t)tot[1];
    info_out[NWT_INFO_ROUNDS] = rounds;
    info_out[NWT_INFO_LABEL_ROUNDS] = label_rounds;
    info_out[NWT_INFO_LAUNCHES] = launches;
    info_out[NWT_INFO_LOWERED] = (int64_t)cnt[NWT_C_LOWERED];
    info_out[NWT_INFO_RELAXED] = (int64_t)cnt[NWT_C_RELAXED];
    info_out[NWT_INFO_BATCH] = NWT_BATCH;
    return NWT_OK;
}
