// Exact ray casting against a triangle mesh on the device (MI355X, gfx950): include/nw_rays.h.
//
//   nwc_set_mesh    (bq::FaceGrid::set_faces)   the mesh query units' shared intake (nw_bq.h): k_bq_face_setup, one thread per face, the
//                                     float64 centroid and rho_f, the largest centroid-to-corner distance, a hair enlarged so that
//                                     rounding can only make a bound weaker; k_bq_rho_reduce, rho_max and the sum of rho_f, one
//                                     workgroup, a fixed order; bq::bounds, the centroids' box
//                   (bq::FaceGrid::bin)   the shared point grid in double over the centroids (bq::size_grid, bq::build_grid); a sorted
//                                     point carries its face id
//   nwc_cast        k_rc_first        one lane per ray, nw_rays_core.h's walk: the ray clipped against the centroids' box dilated by
//                                     rho_max, its arc length inside cut into pieces of one cell size, per piece the cells that overlap
//                                     a box around its midpoint, row by row; a centroid whose arc coordinate falls into the piece and
//                                     whose ball touches the line gets the exact test.  Stops before a piece that begins beyond the
//                                     best hit's reach.
//                   k_rc_count        the same walk to its end: the number of faces hit as well (NWC_COUNT)
//                   k_rc_totals       with NWC_STATS: the sums of the lanes' three counters, one workgroup, integers
//
// The point grid, the face grid, the device buffer with its staging and the context's scaffolding are the query units' shared ones
// (nw_bq.h); the starting cell size is the distance unit's (twice the mean rho_f: a face or two per occupied cell).
// All stores are vector stores in plain C++; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <string>
#include <algorithm>

#include "../../include/nw_rays.h"
#include "nw_bq.h"
#include "nw_rays_core.h"

#define NWC_EXPORT extern "C" __attribute__((visibility("default")))
#define NWC_BLOCK 256

static_assert(sizeof(nwc_point) == sizeof(bq::PtF64) && offsetof(nwc_point, i) == offsetof(bq::PtF64, i), "nwc_point is bq::PtF64");

// ---- the cast ---------------------------------------------------------------------------------------------------------------------------
struct rc_rays {
    const double *origin, *dir;
    const int *skip_vertex, *skip_face;   // either may be nullptr
    int n;
    double t_max;
};

struct rc_out {
    double *t;                            // any may be nullptr
    int *face, *info, *hits;
    long long *stats;                     // [3][n]: pieces, centroids read, exact tests
};

template <bool COUNT> __device__ __forceinline__ void rc_cast(const nwc_mesh &m, const rc_rays &q, const rc_out &out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= q.n) return;
    const nwc_ray r = nwc_make_ray(q.origin + 3 * (int64_t)i, q.dir + 3 * (int64_t)i, q.skip_vertex ? q.skip_vertex[i] : -1,
                                   q.skip_face ? q.skip_face[i] : -1, q.t_max);
    nwc_walk_stats st;
    const nwc_best b = nwc_walk<COUNT>(m, r, &st);
    if (out.t) out.t[i] = b.t;
    if (out.face) out.face[i] = b.face;
    if (out.info) out.info[i] = b.info;
    if (COUNT && out.hits) out.hits[i] = b.hits;
    if (out.stats) {
        out.stats[i] = st.pieces;
        out.stats[(int64_t)q.n + i] = st.read;
        out.stats[2 * (int64_t)q.n + i] = st.tested;
    }
}

__global__ __launch_bounds__(NWC_BLOCK) void k_rc_first(nwc_mesh m, rc_rays q, rc_out out) { rc_cast<false>(m, q, out); }

__global__ __launch_bounds__(NWC_BLOCK) void k_rc_count(nwc_mesh m, rc_rays q, rc_out out) { rc_cast<true>(m, q, out); }

// out[k] = the sum of a[k n .. (k + 1) n), k = 0, 1, 2
__global__ __launch_bounds__(NWC_BLOCK) void k_rc_totals(const long long *__restrict__ a, int n, long long *__restrict__ out)
{
    __shared__ long long s_t[3][NWC_BLOCK / 64];
    long long t0 = 0, t1 = 0, t2 = 0;
    for (int j = threadIdx.x; j < n; j += NWC_BLOCK) { t0 += a[j]; t1 += a[(int64_t)n + j]; t2 += a[2 * (int64_t)n + j]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { t0 += __shfl_xor(t0, o, 64); t1 += __shfl_xor(t1, o, 64); t2 += __shfl_xor(t2, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_t[0][threadIdx.x >> 6] = t0; s_t[1][threadIdx.x >> 6] = t1; s_t[2][threadIdx.x >> 6] = t2; }
    __syncthreads();
    if (threadIdx.x < 3) out[threadIdx.x] = ((s_t[threadIdx.x][0] + s_t[threadIdx.x][1]) + s_t[threadIdx.x][2]) + s_t[threadIdx.x][3];
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nwc_ctx : bq::Ctx {
    bq::FaceGrid m;               // the mesh of the last nwc_set_mesh and its grid (m.nf == 0: the context holds no mesh)
    // nwc_cast
    int64_t stats[3] = {0, 0, 0};
    long long tot_h[3] = {0, 0, 0};
    DevBuf up_o, up_d, up_sv, up_sf, qmm, t, face, info, hits, st, tot;
};

namespace {

#define NWC_HIP(call) BQ_HIP(call, NWC_ERR_NOMEM, NWC_ERR_HIP)

const bq::FaceCodes NWC_FACE_CODES = {NWC_ERR_BADARG, NWC_ERR_NONFINITE, NWC_ERR_NOMEM, NWC_ERR_HIP};

}  // namespace

NWC_EXPORT int nwc_abi_version(void) { return NWC_ABI_VERSION; }

NWC_EXPORT int nwc_create(int device, nwc_ctx **out) { return bq::create(device, out, NWC_ERR_BADARG, NWC_ERR_HIP); }

NWC_EXPORT void nwc_destroy(nwc_ctx *ctx) { bq::destroy(ctx); }

NWC_EXPORT const char *nwc_last_error(nwc_ctx *ctx) { return bq::last_error(ctx); }

NWC_EXPORT int nwc_set_mesh(nwc_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces)
{
    if (ctx) { ctx->m.nf = 0; ctx->stats[0] = ctx->stats[1] = ctx->stats[2] = 0; }
    bq::FaceStatus s = bq::check_faces(pos, n_vertices, faces, n_faces);
    if (!s.ok()) return bq::face_fail(ctx, "nwc_set_mesh", s, NWC_FACE_CODES);
    if (!ctx) return NWC_ERR_BADARG;
    NWC_HIP(hipSetDevice(ctx->device));
    bq::FaceGrid &m = ctx->m;
    s = m.set_faces(ctx->stream, pos, n_vertices, faces, n_faces);
    // cell size: the distance unit's, twice the mean rho_f with bq::face_cell's floor
    if (s.ok()) s = m.bin(ctx->stream, bq::face_cell(2.0 * m.rho_mean, m.emax()));
    if (!s.ok()) { m.nf = 0; return bq::face_fail(ctx, "nwc_set_mesh", s, NWC_FACE_CODES); }
    return NWC_OK;
}

namespace {

// (n,3) doubles, on the host (checked here) or on the device (checked there); nothing of the caller's is uploaded:
// *amax = the largest coordinate in magnitude
int check_triples(nwc_ctx *ctx, const double *src, int64_t n, bool *dev, double *amax, const char *what)
{
    *amax = 0.0;
    *dev = bq::on_device(src);
    if (!*dev) {
        if (!bq::all_finite(src, 3 * n)) return fail(ctx, NWC_ERR_NONFINITE, std::string("nwc_cast: ") + what + " is not finite");
        for (int64_t i = 0; i < 3 * n; ++i) *amax = std::max(*amax, std::fabs(src[i]));
        return NWC_OK;
    }
    bq::Grid<double> box;
    bool finite[2];
    NWC_HIP(bq::bounds<double>(ctx->stream, ctx->qmm, src, (int)n, nullptr, 0, &box, finite));
    if (!finite[0]) return fail(ctx, NWC_ERR_NONFINITE, std::string("nwc_cast: ") + what + " is not finite");
    for (int k = 0; k < 3; ++k) *amax = std::max(*amax, std::max(std::fabs(box.lo[k]), std::fabs(box.hi[k])));
    return NWC_OK;
}

// what nwc_cast has checked: the rays as given, and which of the four arrays are host memory to be uploaded
struct rc_args {
    const double *origin, *dir;
    const int32_t *skip_vertex, *skip_face;
    bool up_o, up_d, up_sv, up_sf;
    int n, flags;
    double t_max;
    double *t_out;
    int32_t *face_out, *info_out, *hits_out;
};

// every buffer first, then the uploads, the launch and the copies back.  The caller synchronises the stream if this fails, so that
// no copy from or to the caller's arrays is still in flight when nwc_cast returns.
int cast_checked(nwc_ctx *ctx, const rc_args &a)
{
    const int nq = a.n;
    if (a.up_o) NWC_HIP(ctx->up_o.ensure(sizeof(double) * 3 * (size_t)nq));
    if (a.up_d) NWC_HIP(ctx->up_d.ensure(sizeof(double) * 3 * (size_t)nq));
    if (a.up_sv) NWC_HIP(ctx->up_sv.ensure(sizeof(int) * (size_t)nq));
    if (a.up_sf) NWC_HIP(ctx->up_sf.ensure(sizeof(int) * (size_t)nq));
    rc_out out;
    out.t = nullptr; out.face = out.info = out.hits = nullptr; out.stats = nullptr;
    if (a.t_out) { NWC_HIP(ctx->t.ensure(sizeof(double) * (size_t)nq)); out.t = ctx->t.as<double>(); }
    if (a.face_out) { NWC_HIP(ctx->face.ensure(sizeof(int) * (size_t)nq)); out.face = ctx->face.as<int>(); }
    if (a.info_out) { NWC_HIP(ctx->info.ensure(sizeof(int) * (size_t)nq)); out.info = ctx->info.as<int>(); }
    if (a.hits_out) { NWC_HIP(ctx->hits.ensure(sizeof(int) * (size_t)nq)); out.hits = ctx->hits.as<int>(); }
    if (a.flags & NWC_STATS) {
        NWC_HIP(ctx->st.ensure(sizeof(long long) * 3 * (size_t)nq));
        NWC_HIP(ctx->tot.ensure(sizeof(long long) * 3));
        out.stats = ctx->st.as<long long>();
    }
    rc_rays q;
    q.n = nq;
    q.t_max = a.t_max;
    q.origin = a.origin; q.dir = a.dir; q.skip_vertex = a.skip_vertex; q.skip_face = a.skip_face;
    if (a.up_o) { NWC_HIP(bq::upload(ctx->stream, ctx->up_o, a.origin, 3 * (int64_t)nq)); q.origin = ctx->up_o.as<double>(); }
    if (a.up_d) { NWC_HIP(bq::upload(ctx->stream, ctx->up_d, a.dir, 3 * (int64_t)nq)); q.dir = ctx->up_d.as<double>(); }
    if (a.up_sv) { NWC_HIP(bq::upload(ctx->stream, ctx->up_sv, a.skip_vertex, (int64_t)nq)); q.skip_vertex = ctx->up_sv.as<int>(); }
    if (a.up_sf) { NWC_HIP(bq::upload(ctx->stream, ctx->up_sf, a.skip_face, (int64_t)nq)); q.skip_face = ctx->up_sf.as<int>(); }
    const bq::FaceGrid &fg = ctx->m;
    nwc_mesh m;
    m.pos = fg.mpos.as<float>(); m.faces = fg.mfaces.as<int>(); m.nf = fg.nf;
    m.pts = fg.sorted.as<nwc_point>(); m.cstart = fg.cstart.as<int>(); m.rho = fg.rho.as<double>();
    m.rho_max = fg.rho_max; m.h = fg.g.h;
    m.lo0 = fg.g.lo[0]; m.lo1 = fg.g.lo[1]; m.lo2 = fg.g.lo[2];
    m.hi0 = fg.g.hi[0]; m.hi1 = fg.g.hi[1]; m.hi2 = fg.g.hi[2];
    m.d0 = fg.g.dims[0]; m.d1 = fg.g.dims[1]; m.d2 = fg.g.dims[2];
    if (a.flags & NWC_COUNT) hipLaunchKernelGGL(k_rc_count, dim3(nblk(nq)), dim3(NWC_BLOCK), 0, ctx->stream, m, q, out);
    else hipLaunchKernelGGL(k_rc_first, dim3(nblk(nq)), dim3(NWC_BLOCK), 0, ctx->stream, m, q, out);
    if (a.flags & NWC_STATS) hipLaunchKernelGGL(k_rc_totals, dim3(1), dim3(NWC_BLOCK), 0, ctx->stream, (const long long *)out.stats, nq, ctx->tot.as<long long>());
    NWC_HIP(hipGetLastError());
    long long *tot = ctx->tot_h;                                  // (in the context: a copy into it may outlive this function)
    tot[0] = tot[1] = tot[2] = 0;
    if (a.t_out) NWC_HIP(hipMemcpyAsync(a.t_out, ctx->t.p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (a.face_out) NWC_HIP(hipMemcpyAsync(a.face_out, ctx->face.p, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (a.info_out) NWC_HIP(hipMemcpyAsync(a.info_out, ctx->info.p, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (a.hits_out) NWC_HIP(hipMemcpyAsync(a.hits_out, ctx->hits.p, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, ctx->stream));
    if (a.flags & NWC_STATS) NWC_HIP(hipMemcpyAsync(tot, ctx->tot.p, sizeof(ctx->tot_h), hipMemcpyDeviceToHost, ctx->stream));
    NWC_HIP(hipStreamSynchronize(ctx->stream));                   // (the caller's arrays are free from here on)
    for (int k = 0; k < 3; ++k) ctx->stats[k] = tot[k];
    return NWC_OK;
}

}  // namespace

NWC_EXPORT int nwc_cast(nwc_ctx *ctx, const double *origin, const double *dir, int64_t n, const int32_t *skip_vertex, const int32_t *skip_face,
                        double t_max, int flags, double *t_out, int32_t *face_out, int32_t *info_out, int32_t *hits_out)
{
    if (ctx) ctx->stats[0] = ctx->stats[1] = ctx->stats[2] = 0;
    if (!origin || !dir || n < 1 || n > (1ll << 30) || (flags & ~(NWC_COUNT | NWC_STATS))) return fail(ctx, NWC_ERR_BADARG, "nwc_cast: a NULL array of rays, a size out of range or an unknown flag");
    if (!(t_max >= 0.0)) return fail(ctx, NWC_ERR_BADARG, "nwc_cast: t_max is negative or not a number");
    if (hits_out && !(flags & NWC_COUNT)) return fail(ctx, NWC_ERR_BADARG, "nwc_cast: hits_out needs NWC_COUNT");
    if (!ctx) return NWC_ERR_BADARG;
    if (ctx->m.nf < 1) return fail(ctx, NWC_ERR_NOMESH, "nwc_cast: the context holds no mesh");
    NWC_HIP(hipSetDevice(ctx->device));
    // every check of the rays comes before the first upload of any of them
    rc_args a;
    a.origin = origin; a.dir = dir; a.skip_vertex = skip_vertex; a.skip_face = skip_face;
    a.n = (int)n; a.flags = flags; a.t_max = t_max;
    a.t_out = t_out; a.face_out = face_out; a.info_out = info_out; a.hits_out = hits_out;
    int code;
    bool o_dev, d_dev;
    double omax, dmax, gmax = 0.0;
    if ((code = check_triples(ctx, origin, n, &o_dev, &omax, "an origin")) != NWC_OK) return code;
    if ((code = check_triples(ctx, dir, n, &d_dev, &dmax, "a direction")) != NWC_OK) return code;
    // the walk's allowance for rounding grows with the coordinates (nw_rays_core.h: E); beyond a cell it would make every piece read
    // the whole grid, so such a ray is refused rather than walked for minutes.  (A direction needs no such limit: the walk follows it
    // scaled by its largest component, and its length bounds nothing.)
    for (int k = 0; k < 3; ++k) gmax = std::max(gmax, std::max(std::fabs(ctx->m.g.lo[k]), std::fabs(ctx->m.g.hi[k])));
    if (!(NWC_REL_SLACK * (omax + gmax) <= ctx->m.g.h)) return fail(ctx, NWC_ERR_BADARG, "nwc_cast: an origin lies more than 1e9 cells from the origin of the coordinates");
    a.up_o = !o_dev;
    a.up_d = !d_dev;
    a.up_sv = skip_vertex && !bq::on_device(skip_vertex);
    a.up_sf = skip_face && !bq::on_device(skip_face);
    code = cast_checked(ctx, a);
    if (code != NWC_OK) (void)hipStreamSynchronize(ctx->stream);   // (nothing of the caller's is still being read or written)
    return code;
}

NWC_EXPORT int nwc_get_stats(nwc_ctx *ctx, int64_t out[3])
{
    if (!ctx || !out) return fail(ctx, NWC_ERR_BADARG, "nwc_get_stats: a NULL argument");
    for (int k = 0; k < 3; ++k) out[k] = ctx->stats[k];
    return NWC_OK;
}
