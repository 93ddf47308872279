// Density isosurface of the localization cloud on the device (MI355X, gfx950): include/nw_isosurface.h.
//
// The start surface of a fit, made from the cloud itself: count per voxel, integer binomial smoothing, a threshold from the median of the
// occupied voxels, and sheet-aware surface nets of `field > thr`.  The definitions are the header's; the NumPy restatement the kernels are
// tested against is tests/isosurface_ref.py.  The scan, the host loop and the bin rule of the radix select, the device buffer with its
// staging and the context's scaffolding are the query units' shared ones (nw_bq.h).
//
//   k_iso_count        one localization per thread, four per thread and workgroup pass: voxel ids are aggregated in an LDS hash table
//                      (2048 slots, four probes) and flushed with one global atomic per slot; what finds no slot goes to HBM directly.
//                      Integer atomics: the counts do not depend on the order of arrival.
//   k_iso_widen        uint32 counts -> the uint64 field
//   k_iso_smooth       one voxel per thread, lanes along x: out = in[-1] + 2 in[0] + in[+1] along one axis, zero beyond the grid
//   k_iso_hist         one byte of a radix select over the field values of the occupied voxels (256 bins in LDS, then HBM)
//   k_iso_pattern      one cell per thread, lanes along x: the 8-bit corner pattern (kept: both emission passes read it, not the field),
//                      the active flag (pattern not 0 or 255) and the border test
//   k_iso_compact      active cells -> their list, in ascending order (exclusive scan of the flags)
//   k_iso_cell_counts  per active cell: its number of sheets and which of its three own edges (from corner 0 along x, y, z) are crossed
//   k_iso_vertices     per active cell: one vertex per sheet (mean of its crossings, ascending edge order) and its key
//   k_iso_quads        per (axis, active cell): the two triangles of the quad around a crossed own edge
//
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/nw_isosurface.h"
#include "nw_bq.h"

#define NWI_EXPORT extern "C" __attribute__((visibility("default")))
#define NWI_BLOCK 256
#define NWI_PER_THREAD 4            // localizations per thread of k_iso_count
#define NWI_HASH 2048               // slots of its LDS table
#define NWI_HASH_SHIFT 21           // 32 - log2(NWI_HASH)
#define NWI_MAX_DIM (1 << 20)       // per axis: the float compare of a voxel coordinate with the dimension is exact
#define NWI_MAX_ACTIVE (1 << 29)    // 3 x the active cells is an int

typedef unsigned long long u64;

struct nwi_grid {
    float lo[3];
    float h, inv_h;
    int dims[3];
};

// ---- density ------------------------------------------------------------------------------------------------------------------------
// voxel coordinate along one axis, as a float (the host check of the localizations uses the same expression)
__host__ __device__ __forceinline__ float iso_voxel_1d(float x, float lo, float inv_h) { return floorf((x - lo) * inv_h); }

__global__ __launch_bounds__(NWI_BLOCK) void k_iso_count(const float *__restrict__ xyz, int n, nwi_grid g, unsigned *__restrict__ count,
                                                         int *__restrict__ bad /* bit 0: non-finite, bit 1: outside the grid */)
{
    __shared__ int s_key[NWI_HASH];
    __shared__ unsigned s_cnt[NWI_HASH];
    for (int t = threadIdx.x; t < NWI_HASH; t += NWI_BLOCK) { s_key[t] = -1; s_cnt[t] = 0u; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (NWI_BLOCK * NWI_PER_THREAD);
#pragma unroll
    for (int k = 0; k < NWI_PER_THREAD; ++k) {
        const int64_t i = base + k * NWI_BLOCK + threadIdx.x;
        if (i >= n) continue;
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (!(isfinite(x) && isfinite(y) && isfinite(z))) { atomicOr(bad, 1); continue; }
        const float fx = iso_voxel_1d(x, g.lo[0], g.inv_h), fy = iso_voxel_1d(y, g.lo[1], g.inv_h), fz = iso_voxel_1d(z, g.lo[2], g.inv_h);
        if (!(fx >= 0.0f && fx < (float)g.dims[0] && fy >= 0.0f && fy < (float)g.dims[1] && fz >= 0.0f && fz < (float)g.dims[2])) {
            atomicOr(bad, 2);
            continue;
        }
        const int v = ((int)fz * g.dims[1] + (int)fy) * g.dims[0] + (int)fx;
        unsigned slot = ((unsigned)v * 2654435761u) >> NWI_HASH_SHIFT;
        bool done = false;
#pragma unroll
        for (int probe = 0; probe < 4 && !done; ++probe) {
            const int old = atomicCAS(&s_key[slot], -1, v);
            if (old == -1 || old == v) { atomicAdd(&s_cnt[slot], 1u); done = true; }
            else slot = (slot + 1) & (NWI_HASH - 1);
        }
        if (!done) atomicAdd(&count[v], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NWI_HASH; t += NWI_BLOCK) {
        const unsigned c = s_cnt[t];
        if (c) atomicAdd(&count[s_key[t]], c);
    }
}

__global__ __launch_bounds__(NWI_BLOCK) void k_iso_widen(const unsigned *__restrict__ count, int n, u64 *__restrict__ field)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) field[i] = (u64)count[i];
}

__global__ __launch_bounds__(NWI_BLOCK) void k_iso_smooth(const u64 *__restrict__ in, u64 *__restrict__ out, int nx, int ny, int nz, int axis)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nx * ny * nz) return;
    const int i = idx % nx, j = (idx / nx) % ny, k = idx / (nx * ny);
    const int c = axis == 0 ? i : axis == 1 ? j : k;
    const int dim = axis == 0 ? nx : axis == 1 ? ny : nz;
    const int stride = axis == 0 ? 1 : axis == 1 ? nx : nx * ny;
    u64 s = 2ull * in[idx];
    if (c > 0) s += in[idx - stride];
    if (c < dim - 1) s += in[idx + stride];
    out[idx] = s;
}

// ---- radix select ---------------------------------------------------------------------------------------------------------------------
// hist[b] += the occupied voxels whose field value has the bits above shift + 8 equal to `prefix` and byte b at `shift`
__global__ __launch_bounds__(NWI_BLOCK) void k_iso_hist(const u64 *__restrict__ field, const unsigned *__restrict__ count, int n, u64 prefix, int shift,
                                                        unsigned *__restrict__ hist)
{
    __shared__ unsigned s_h[256];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (count[i] == 0u) continue;
        const int b = bq::radix_bin(field[i], prefix, shift);
        if (b >= 0) atomicAdd(&s_h[b], 1u);
    }
    __syncthreads();
    const unsigned c = s_h[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], c);
}

// ---- surface nets ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NWI_BLOCK) void k_iso_pattern(const u64 *__restrict__ field, u64 thr, int nx, int ny, int nz, unsigned char *__restrict__ cfg,
                                                           int *__restrict__ act, int *__restrict__ flags /* bit 0: an inside node on the outermost layer */)
{
    const int cx = nx - 1, cy = ny - 1, cz = nz - 1;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cx * cy * cz) return;
    const int i = c % cx, j = (c / cx) % cy, k = c / (cx * cy);
    const int node = (k * ny + j) * nx + i;
    unsigned p = 0;
    bool border = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int dx = q & 1, dy = (q >> 1) & 1, dz = q >> 2;
        const bool inside = field[node + dx + dy * nx + dz * nx * ny] > thr;
        p |= (inside ? 1u : 0u) << q;
        const int x = i + dx, y = j + dy, z = k + dz;
        border |= inside && (x == 0 || x == nx - 1 || y == 0 || y == ny - 1 || z == 0 || z == nz - 1);
    }
    cfg[c] = (unsigned char)p;
    act[c] = (p != 0u && p != 255u) ? 1 : 0;
    if (border) atomicOr(flags, 1);
}

__global__ __launch_bounds__(NWI_BLOCK) void k_iso_compact(const int *__restrict__ act, const int *__restrict__ scan, int n, int *__restrict__ alist)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n && act[c]) alist[scan[c]] = c;
}

// tab16: 16 bytes per pattern: [0..11] the rank of edge e's sheet among the pattern's sheets (255: not crossed), [12..15] the sheets
// themselves in ascending order (255: none)
__global__ __launch_bounds__(NWI_BLOCK) void k_iso_cell_counts(const int *__restrict__ alist, int na, const unsigned char *__restrict__ cfg,
                                                               const unsigned char *__restrict__ tab16, int *__restrict__ vcnt, int *__restrict__ qflag)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    const unsigned p = cfg[alist[a]];
    const unsigned roots = *(const unsigned *)(tab16 + 16 * p + 12);
    int ns = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) ns += ((roots >> (8 * s)) & 255u) != 255u;
    vcnt[a] = ns;
    const unsigned b0 = p & 1u;
    qflag[a] = b0 != ((p >> 1) & 1u);
    qflag[na + a] = b0 != ((p >> 2) & 1u);
    qflag[2 * na + a] = b0 != ((p >> 4) & 1u);
}

__global__ __launch_bounds__(NWI_BLOCK) void k_iso_vertices(const int *__restrict__ alist, int na, const unsigned char *__restrict__ cfg,
                                                            const unsigned char *__restrict__ tab16, const int *__restrict__ voff,
                                                            const u64 *__restrict__ field, u64 thr, nwi_grid g,
                                                            float *__restrict__ verts, long long *__restrict__ keys)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= na) return;
    const int nx = g.dims[0], ny = g.dims[1];
    const int cx = nx - 1, cy = ny - 1;
    const int c = alist[a];
    const int i = c % cx, j = (c / cx) % cy, k = c / (cx * cy);
    const int node = (k * ny + j) * nx + i;
    const uint4 row = *(const uint4 *)(tab16 + 16 * (unsigned)cfg[c]);
    const unsigned rw[4] = {row.x, row.y, row.z, row.w};
    u64 f[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) f[q] = field[node + (q & 1) + ((q >> 1) & 1) * nx + (q >> 2) * nx * ny];
    float sx[4] = {0.f, 0.f, 0.f, 0.f}, sy[4] = {0.f, 0.f, 0.f, 0.f}, sz[4] = {0.f, 0.f, 0.f, 0.f};
    int cn[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int axis = e >> 2, ea = e & 1, eb = (e >> 1) & 1, ua = (axis + 1) % 3, va = (axis + 2) % 3;
        const int k0 = (ea << ua) | (eb << va), k1 = k0 | (1 << axis);
        const unsigned r = (rw[e >> 2] >> (8 * (e & 3))) & 255u;
        if (r == 255u) continue;
        // crossing parameter from the integer field: (f0 - thr) / (f0 - f1), the differences exact in 64 bits, then float32
        const float t = (float)(long long)(f[k0] - thr) / (float)(long long)(f[k0] - f[k1]);
        float p[3];
        p[axis] = t;
        p[ua] = (float)ea;
        p[va] = (float)eb;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (r == (unsigned)s) { sx[s] += p[0]; sy[s] += p[1]; sz[s] += p[2]; cn[s] += 1; }
    }
    const int vb = voff[a];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const unsigned root = (rw[3] >> (8 * s)) & 255u;
        if (root == 255u) continue;
        const float m = (float)cn[s];
        const int64_t v = (int64_t)vb + s;
        verts[3 * v] = g.lo[0] + (((float)i + 0.5f) + sx[s] / m) * g.h;
        verts[3 * v + 1] = g.lo[1] + (((float)j + 0.5f) + sy[s] / m) * g.h;
        verts[3 * v + 2] = g.lo[2] + (((float)k + 0.5f) + sz[s] / m) * g.h;
        keys[v] = (long long)c * 16 + (long long)root;
    }
}

__global__ __launch_bounds__(NWI_BLOCK) void k_iso_quads(const int *__restrict__ alist, int na, const unsigned char *__restrict__ cfg,
                                                         const unsigned char *__restrict__ tab16, const int *__restrict__ scan, const int *__restrict__ voff,
                                                         const int *__restrict__ qflag, const int *__restrict__ qoff, int nx, int ny, int nz,
                                                         int *__restrict__ faces)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * na || !qflag[idx]) return;
    const int axis = idx / na, a = idx - axis * na;
    const int cd[3] = {nx - 1, ny - 1, nz - 1};
    const int c = alist[a];
    const int low[3] = {c % cd[0], (c / cd[0]) % cd[1], c / (cd[0] * cd[1])};          // the edge's lower node = the cell's corner 0
    const int ua = (axis + 1) % 3, va = (axis + 2) % 3;
    int v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                                                       // counter-clockwise about +axis: (1,1) (0,1) (0,0) (1,0)
        const int qa = (q == 0 || q == 3) ? 1 : 0, qb = q < 2 ? 1 : 0;
        int cl[3] = {low[0], low[1], low[2]};
        // (a crossed edge has an inside end, which is no border node once the border test has passed: the four cells exist; clamped all the same)
        cl[ua] = max(cl[ua] - qa, 0);
        cl[va] = max(cl[va] - qb, 0);
        const int nc = (cl[2] * cd[1] + cl[1]) * cd[0] + cl[0];
        const unsigned r = tab16[16 * (unsigned)cfg[nc] + axis * 4 + qa + 2 * qb];
        v[q] = voff[scan[nc]] + (int)(r & 3u);
    }
    if (!(cfg[c] & 1u)) { const int t0 = v[0], t1 = v[1]; v[0] = v[3]; v[1] = v[2]; v[2] = t1; v[3] = t0; }    // outside at the lower node: normal -axis
    int *o = faces + 6 * (int64_t)qoff[idx];
    if (((low[0] + low[1] + low[2]) & 1) == 0) {
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
        o[3] = v[0]; o[4] = v[2]; o[5] = v[3];
    } else {
        o[0] = v[0]; o[1] = v[1]; o[2] = v[3];
        o[3] = v[1]; o[4] = v[2]; o[5] = v[3];
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwi_ctx : bq::Ctx {
    // the field (nwi_density)
    nwi_grid grid{};
    int n_vox = 0, passes = 0;
    int64_t n_points = 0;
    bool have_counts = false;       // the field came from nwi_density: nwi_threshold_auto has counts to select over
    DevBuf counts, field_a, field_b, pts;
    u64 *field = nullptr;
    // the sheet table
    bool have_table = false;
    DevBuf tab16;
    // the extraction
    int64_t n_vertices = -1, n_faces = -1;
    DevBuf cfg, act, scan, alist, vcnt, voff, qflag, qoff, verts, keys, faces, small, scan_tmp;
};

namespace {

#define NWI_HIP(call) BQ_HIP(call, NWI_ERR_NOMEM, NWI_ERR_HIP)

}  // namespace

NWI_EXPORT int nwi_abi_version(void) { return NWI_ABI_VERSION; }

NWI_EXPORT int nwi_create(int device, nwi_ctx **out) { return bq::create(device, out, NWI_ERR_BADARG, NWI_ERR_HIP); }

NWI_EXPORT void nwi_destroy(nwi_ctx *ctx) { bq::destroy(ctx); }

NWI_EXPORT const char *nwi_last_error(nwi_ctx *ctx) { return bq::last_error(ctx); }

NWI_EXPORT int nwi_set_sheet_table(nwi_ctx *ctx, const int8_t *table)
{
    if (!table) return NWI_ERR_BADARG;
    std::vector<unsigned char> t16(256 * 16, 255);
    for (int p = 0; p < 256; ++p) {
        const int8_t *row = table + 12 * p;
        int ns = 0;
        for (int e = 0; e < 12; ++e) {
            const int axis = e >> 2, ea = e & 1, eb = (e >> 1) & 1, ua = (axis + 1) % 3, va = (axis + 2) % 3;
            const int k0 = (ea << ua) | (eb << va), k1 = k0 | (1 << axis);
            const bool crossed = ((p >> k0) & 1) != ((p >> k1) & 1);
            const int l = row[e];
            if (crossed != (l >= 0)) return NWI_ERR_BADARG;
            if (!crossed) continue;
            if (l > e || row[l] != l) return NWI_ERR_BADARG;
            if (l == e) {
                if (ns >= 4) return NWI_ERR_BADARG;
                t16[16 * p + 12 + ns++] = (unsigned char)e;
            }
            int rank = 0;
            for (int q = 0; q < l; ++q) rank += row[q] == q;
            t16[16 * p + e] = (unsigned char)rank;
        }
    }
    if (!ctx) return NWI_ERR_BADARG;
    NWI_HIP(hipSetDevice(ctx->device));
    ctx->have_table = false;
    NWI_HIP(bq::upload(ctx->stream, ctx->tab16, t16.data(), (int64_t)t16.size()));
    NWI_HIP(hipStreamSynchronize(ctx->stream));                 // (t16 is a local)
    ctx->have_table = true;
    return NWI_OK;
}

NWI_EXPORT int nwi_density(nwi_ctx *ctx, const float *xyz, int64_t n_points, int points_on_device, const float *lo, float h, const int32_t *dims,
                           int passes, uint64_t *field_out, uint32_t *counts_out)
{
    if (!xyz || !lo || !dims || n_points < 1 || n_points > (1ll << 30) || passes < 0 || passes > NWI_MAX_PASSES) return NWI_ERR_BADARG;
    if (!(h > 0.0f) || !std::isfinite(h) || (points_on_device != 0 && points_on_device != 1)) return NWI_ERR_BADARG;
    int64_t nvox = 1;
    for (int d = 0; d < 3; ++d) {
        if (!std::isfinite(lo[d]) || dims[d] < 3 || dims[d] > NWI_MAX_DIM) return NWI_ERR_BADARG;
        nvox *= dims[d];
    }
    if (nvox > (1ll << 30)) return NWI_ERR_BADARG;
    nwi_grid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = lo[d]; g.dims[d] = dims[d]; }
    g.h = h;
    g.inv_h = 1.0f / h;
    if (!points_on_device) {
        for (int64_t i = 0; i < n_points; ++i) {
            for (int d = 0; d < 3; ++d) {
                const float x = xyz[3 * i + d];
                if (!std::isfinite(x)) return fail(ctx, NWI_ERR_NONFINITE, "nwi_density: a localization is not finite");
                const float v = iso_voxel_1d(x, g.lo[d], g.inv_h);
                if (!(v >= 0.0f && v < (float)g.dims[d])) return fail(ctx, NWI_ERR_OUTSIDE, "nwi_density: a localization lies outside the grid");
            }
        }
    }
    if (!ctx) return NWI_ERR_BADARG;
    NWI_HIP(hipSetDevice(ctx->device));
    const int n = (int)n_points, nv = (int)nvox;
    ctx->n_vox = 0;
    ctx->have_counts = false;
    ctx->n_vertices = ctx->n_faces = -1;
    const float *src = xyz;
    if (!points_on_device) {
        NWI_HIP(bq::upload(ctx->stream, ctx->pts, xyz, 3 * n_points));
        src = ctx->pts.as<float>();
    }
    NWI_HIP(ctx->counts.ensure(sizeof(unsigned) * (size_t)nv));
    NWI_HIP(ctx->field_a.ensure(sizeof(u64) * (size_t)nv));
    if (passes > 0) NWI_HIP(ctx->field_b.ensure(sizeof(u64) * (size_t)nv));
    NWI_HIP(ctx->small.ensure(sizeof(unsigned) * 512));
    NWI_HIP(hipMemsetAsync(ctx->counts.p, 0, sizeof(unsigned) * (size_t)nv, ctx->stream));
    NWI_HIP(hipMemsetAsync(ctx->small.p, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_iso_count, dim3(nblk(n, NWI_BLOCK * NWI_PER_THREAD)), dim3(NWI_BLOCK), 0, ctx->stream, src, n, g, ctx->counts.as<unsigned>(),
                       ctx->small.as<int>());
    NWI_HIP(hipGetLastError());
    int bad = 0;
    NWI_HIP(hipMemcpyAsync(&bad, ctx->small.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NWI_HIP(hipStreamSynchronize(ctx->stream));
    if (bad & 1) return fail(ctx, NWI_ERR_NONFINITE, "nwi_density: a localization is not finite");
    if (bad & 2) return fail(ctx, NWI_ERR_OUTSIDE, "nwi_density: a localization lies outside the grid");
    u64 *cur = ctx->field_a.as<u64>(), *nxt = ctx->field_b.as<u64>();
    hipLaunchKernelGGL(k_iso_widen, dim3(nblk(nv)), dim3(NWI_BLOCK), 0, ctx->stream, ctx->counts.as<unsigned>(), nv, cur);
    for (int p = 0; p < passes; ++p)
        for (int axis = 0; axis < 3; ++axis) {
            hipLaunchKernelGGL(k_iso_smooth, dim3(nblk(nv)), dim3(NWI_BLOCK), 0, ctx->stream, cur, nxt, g.dims[0], g.dims[1], g.dims[2], axis);
            std::swap(cur, nxt);
        }
    NWI_HIP(hipGetLastError());
    if (field_out) NWI_HIP(hipMemcpyAsync(field_out, cur, sizeof(u64) * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
    if (counts_out) NWI_HIP(hipMemcpyAsync(counts_out, ctx->counts.p, sizeof(unsigned) * (size_t)nv, hipMemcpyDeviceToHost, ctx->stream));
    NWI_HIP(hipStreamSynchronize(ctx->stream));
    ctx->field = cur;
    ctx->grid = g;
    ctx->passes = passes;
    ctx->n_points = n_points;
    ctx->n_vox = nv;
    ctx->have_counts = true;
    return NWI_OK;
}

NWI_EXPORT int nwi_set_field(nwi_ctx *ctx, const uint64_t *field, int on_device, const float *lo, float h, const int32_t *dims)
{
    if (!field || !lo || !dims || (on_device != 0 && on_device != 1) || !(h > 0.0f) || !std::isfinite(h)) return NWI_ERR_BADARG;
    int64_t nvox = 1;
    for (int d = 0; d < 3; ++d) {
        if (!std::isfinite(lo[d]) || dims[d] < 3 || dims[d] > NWI_MAX_DIM) return NWI_ERR_BADARG;
        nvox *= dims[d];
    }
    if (nvox > (1ll << 30)) return NWI_ERR_BADARG;
    if (!ctx) return NWI_ERR_BADARG;
    NWI_HIP(hipSetDevice(ctx->device));
    ctx->n_vox = 0;
    ctx->have_counts = false;
    ctx->n_vertices = ctx->n_faces = -1;
    NWI_HIP(ctx->field_a.ensure(sizeof(u64) * (size_t)nvox));
    NWI_HIP(ctx->small.ensure(sizeof(unsigned) * 512));         // (nwi_extract's flag word lives there)
    NWI_HIP(hipMemcpyAsync(ctx->field_a.p, field, sizeof(u64) * (size_t)nvox, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    NWI_HIP(hipStreamSynchronize(ctx->stream));                 // (the caller's field is not read after the call)
    for (int d = 0; d < 3; ++d) { ctx->grid.lo[d] = lo[d]; ctx->grid.dims[d] = dims[d]; }
    ctx->grid.h = h;
    ctx->grid.inv_h = 1.0f / h;
    ctx->field = ctx->field_a.as<u64>();
    ctx->passes = 0;
    ctx->n_points = 0;
    ctx->n_vox = (int)nvox;
    return NWI_OK;
}

NWI_EXPORT int nwi_threshold_auto(nwi_ctx *ctx, double fraction, uint64_t *median, uint64_t *thr, double *density, int64_t *n_occupied)
{
    if (!thr || !(fraction >= 0.0) || !std::isfinite(fraction)) return NWI_ERR_BADARG;
    if (!ctx) return NWI_ERR_BADARG;
    if (ctx->n_vox < 1 || !ctx->have_counts) return fail(ctx, NWI_ERR_STATE, "nwi_threshold_auto: nwi_density first");
    NWI_HIP(hipSetDevice(ctx->device));
    // no field value exceeds n_points * 4^(3 passes): the bytes above it are zero and need no pass
    const u64 vmax = (u64)ctx->n_points << (6 * ctx->passes);
    int shift = 56;
    while (shift > 0 && (vmax >> shift) == 0ull) shift -= 8;
    // the lower median of the occupied voxels' field values (the first pass sees every occupied voxel)
    int64_t rank = -1, occupied = 0;
    uint64_t prefix = 0;
    const auto pass = [&](uint64_t pre, int sh, unsigned *hist) {
        hipLaunchKernelGGL(k_iso_hist, dim3(std::min(nblk(ctx->n_vox), 2048)), dim3(NWI_BLOCK), 0, ctx->stream, ctx->field, ctx->counts.as<unsigned>(),
                           ctx->n_vox, (u64)pre, sh, hist);
    };
    const auto lower_median = [&](int64_t total) { occupied = total; return (total - 1) / 2; };
    unsigned *bins = ctx->small.as<unsigned>() + 256;           // (small[0] is the counting kernel's flag word)
    NWI_HIP(bq::select_u64(ctx->stream, bins, shift, pass, lower_median, &prefix, &rank));
    if (occupied == 0) return fail(ctx, NWI_ERR_EMPTY, "nwi_threshold_auto: no occupied voxel");
    if (rank < 0) return fail(ctx, NWI_ERR_HIP, "nwi_threshold_auto: the histogram does not hold the rank");
    const double t = std::floor(fraction * (double)prefix);
    if (!(t < 18446744073709551616.0)) return fail(ctx, NWI_ERR_BADARG, "nwi_threshold_auto: fraction * median does not fit the field");
    *thr = (u64)t;
    if (median) *median = prefix;
    if (n_occupied) *n_occupied = occupied;
    if (density) *density = (double)*thr / (std::ldexp(1.0, 6 * ctx->passes) * (double)ctx->grid.h * (double)ctx->grid.h * (double)ctx->grid.h);
    return NWI_OK;
}

NWI_EXPORT int nwi_extract(nwi_ctx *ctx, uint64_t thr, int64_t *n_vertices, int64_t *n_faces)
{
    if (!n_vertices || !n_faces) return NWI_ERR_BADARG;
    if (!ctx) return NWI_ERR_BADARG;
    if (ctx->n_vox < 1) return fail(ctx, NWI_ERR_STATE, "nwi_extract: nwi_density first");
    if (!ctx->have_table) return fail(ctx, NWI_ERR_STATE, "nwi_extract: nwi_set_sheet_table first");
    NWI_HIP(hipSetDevice(ctx->device));
    ctx->n_vertices = ctx->n_faces = -1;
    const nwi_grid g = ctx->grid;
    const int nx = g.dims[0], ny = g.dims[1], nz = g.dims[2];
    const int ncell = (nx - 1) * (ny - 1) * (nz - 1);
    NWI_HIP(ctx->cfg.ensure((size_t)ncell));
    NWI_HIP(ctx->act.ensure(sizeof(int) * (size_t)ncell));
    NWI_HIP(ctx->scan.ensure(sizeof(int) * ((size_t)ncell + 1)));
    int *flags = ctx->small.as<int>() + 1;
    NWI_HIP(hipMemsetAsync(flags, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_iso_pattern, dim3(nblk(ncell)), dim3(NWI_BLOCK), 0, ctx->stream, ctx->field, (u64)thr, nx, ny, nz, ctx->cfg.as<unsigned char>(),
                       ctx->act.as<int>(), flags);
    NWI_HIP(hipGetLastError());
    int na = 0, fl = 0;
    NWI_HIP(hipMemcpyAsync(&fl, flags, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));         // (arrives with the scan's total)
    NWI_HIP(bq::scan_total(ctx->stream, ctx->act.as<int>(), ncell, ctx->scan.as<int>(), ctx->scan_tmp, &na));
    if (fl & 1) return fail(ctx, NWI_ERR_BORDER, "nwi_extract: an inside node on the outermost layer of the grid (pad the grid)");
    if (na < 1) return fail(ctx, NWI_ERR_EMPTY, "nwi_extract: no lattice edge crosses the threshold");
    if (na > NWI_MAX_ACTIVE) return fail(ctx, NWI_ERR_BADARG, "nwi_extract: more than 2^29 surface cells");
    NWI_HIP(ctx->alist.ensure(sizeof(int) * (size_t)na));
    NWI_HIP(ctx->vcnt.ensure(sizeof(int) * (size_t)na));
    NWI_HIP(ctx->voff.ensure(sizeof(int) * ((size_t)na + 1)));
    NWI_HIP(ctx->qflag.ensure(sizeof(int) * 3 * (size_t)na));
    NWI_HIP(ctx->qoff.ensure(sizeof(int) * (3 * (size_t)na + 1)));
    hipLaunchKernelGGL(k_iso_compact, dim3(nblk(ncell)), dim3(NWI_BLOCK), 0, ctx->stream, ctx->act.as<int>(), ctx->scan.as<int>(), ncell, ctx->alist.as<int>());
    hipLaunchKernelGGL(k_iso_cell_counts, dim3(nblk(na)), dim3(NWI_BLOCK), 0, ctx->stream, ctx->alist.as<int>(), na, ctx->cfg.as<unsigned char>(),
                       ctx->tab16.as<unsigned char>(), ctx->vcnt.as<int>(), ctx->qflag.as<int>());
    NWI_HIP(hipGetLastError());
    int nv = 0, nq = 0;
    NWI_HIP(bq::scan_total(ctx->stream, ctx->vcnt.as<int>(), na, ctx->voff.as<int>(), ctx->scan_tmp, &nv));
    NWI_HIP(bq::scan_total(ctx->stream, ctx->qflag.as<int>(), 3 * na, ctx->qoff.as<int>(), ctx->scan_tmp, &nq));
    if (nv < 1 || nq < 1 || nv > 4 * (int64_t)na || nq > 3 * (int64_t)na) return fail(ctx, NWI_ERR_HIP, "nwi_extract: the counts of the surface cells do not add up");
    NWI_HIP(ctx->verts.ensure(sizeof(float) * 3 * (size_t)nv));
    NWI_HIP(ctx->keys.ensure(sizeof(long long) * (size_t)nv));
    NWI_HIP(ctx->faces.ensure(sizeof(int) * 6 * (size_t)nq));
    hipLaunchKernelGGL(k_iso_vertices, dim3(nblk(na)), dim3(NWI_BLOCK), 0, ctx->stream, ctx->alist.as<int>(), na, ctx->cfg.as<unsigned char>(),
                       ctx->tab16.as<unsigned char>(), ctx->voff.as<int>(), ctx->field, (u64)thr, g, ctx->verts.as<float>(), ctx->keys.as<long long>());
    hipLaunchKernelGGL(k_iso_quads, dim3(nblk(3 * (int64_t)na)), dim3(NWI_BLOCK), 0, ctx->stream, ctx->alist.as<int>(), na, ctx->cfg.as<unsigned char>(),
                       ctx->tab16.as<unsigned char>(), ctx->scan.as<int>(), ctx->voff.as<int>(), ctx->qflag.as<int>(), ctx->qoff.as<int>(), nx, ny, nz,
                       ctx->faces.as<int>());
    NWI_HIP(hipGetLastError());
    NWI_HIP(hipStreamSynchronize(ctx->stream));
    ctx->n_vertices = nv;
    ctx->n_faces = 2 * (int64_t)nq;
    *n_vertices = ctx->n_vertices;
    *n_faces = ctx->n_faces;
    return NWI_OK;
}

NWI_EXPORT int nwi_get(nwi_ctx *ctx, float *vertices, int32_t *faces, int64_t *keys)
{
    if (!ctx) return NWI_ERR_BADARG;
    if (ctx->n_vertices < 1) return fail(ctx, NWI_ERR_STATE, "nwi_get: nwi_extract first");
    NWI_HIP(hipSetDevice(ctx->device));
    if (vertices) NWI_HIP(hipMemcpyAsync(vertices, ctx->verts.p, sizeof(float) * 3 * (size_t)ctx->n_vertices, hipMemcpyDeviceToHost, ctx->stream));
    if (faces) NWI_HIP(hipMemcpyAsync(faces, ctx->faces.p, sizeof(int) * 3 * (size_t)ctx->n_faces, hipMemcpyDeviceToHost, ctx->stream));
    if (keys) NWI_HIP(hipMemcpyAsync(keys, ctx->keys.p, sizeof(long long) * (size_t)ctx->n_vertices, hipMemcpyDeviceToHost, ctx->stream));
    NWI_HIP(hipStreamSynchronize(ctx->stream));
    return NWI_OK;
}
