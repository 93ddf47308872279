// The kernels the query units share (nw_bq.h), in a unit of their own because a __global__ function defined in two units collides at
// link time through its host stubs:
//   k_bq_scan_*                        the exclusive scan: int, three launches, exact (the per-iteration scan of nanowrap.hip is another one)
//   k_bq_bbox_*                        bounding box (ordered keys, atomicMin / atomicMax) and finiteness of a cloud
//   k_bq_cell_count_*, k_bq_scatter_*  counting sort of a cloud by cell of its grid, with the scan between them; a sorted point carries
//                                      its index in the caller's array (the one scatter of the four cloud query units)
//   k_bq_face_setup, k_bq_rho_reduce   the face grid of the mesh query units: a face's float64 centroid and radius, rho_max and the sum
// The grid's kernels are written once as templates over the coordinate type and wrapped in plain kernels _f32 / _f64:
// build.kernel_resources names a kernel without its template arguments, so two instantiations of one template would share a budget row.
//
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <limits>

#include "nw_bq.h"
#include "nw_device.h"

#define BQ_SCAN_BLOCK 256
#define BQ_SCAN_TILE 2048           // 256 threads x 8

__global__ __launch_bounds__(BQ_SCAN_BLOCK) void k_bq_scan_tiles(const int *__restrict__ in, int n, int *__restrict__ bsum)
{
    __shared__ int s_w[4];
    const int base = blockIdx.x * BQ_SCAN_TILE + threadIdx.x * 8;
    int s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += (base + k < n) ? in[base + k] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(1024) void k_bq_scan_bsums(int *__restrict__ bsum, int nb)
{
    __shared__ int s_w[16];
    __shared__ int s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int base = 0; base < nb; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        const int inc = nw_wave_incl_scan(v, lane);
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wv; ++w) woff += s_w[w];
        const int carry = s_carry;
        if (i < nb) bsum[i] = carry + woff + inc - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + woff + inc;
        __syncthreads();
    }
}

__global__ __launch_bounds__(BQ_SCAN_BLOCK) void k_bq_scan_final(const int *__restrict__ in, int n, const int *__restrict__ bsum, int *__restrict__ out)
{
    __shared__ int s_w[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int base = blockIdx.x * BQ_SCAN_TILE + threadIdx.x * 8;
    int v[8];
    int s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = (base + k < n) ? in[base + k] : 0; s += v[k]; }
    const int inc = nw_wave_incl_scan(s, lane);
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int off = bsum[blockIdx.x] + inc - s;
    for (int w = 0; w < wv; ++w) off += s_w[w];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (base + k < n) out[base + k] = off;
        off += v[k];
        if (base + k == n - 1) out[n] = off;
    }
}

hipError_t bq::scan_exclusive(hipStream_t stream, const int *in, int n, int *out, DevBuf &tmp)
{
    const int nb = (n + BQ_SCAN_TILE - 1) / BQ_SCAN_TILE;
    BQ_TRY(tmp.ensure(sizeof(int) * (size_t)(nb + 1)));
    hipLaunchKernelGGL(k_bq_scan_tiles, dim3(nb), dim3(BQ_SCAN_BLOCK), 0, stream, in, n, tmp.as<int>());
    hipLaunchKernelGGL(k_bq_scan_bsums, dim3(1), dim3(1024), 0, stream, tmp.as<int>(), nb);
    hipLaunchKernelGGL(k_bq_scan_final, dim3(nb), dim3(BQ_SCAN_BLOCK), 0, stream, in, n, tmp.as<int>(), out);
    return hipGetLastError();
}

hipError_t bq::scan_total(hipStream_t stream, const int *in, int n, int *out, DevBuf &tmp, int *total)
{
    BQ_TRY(scan_exclusive(stream, in, n, out, tmp));
    BQ_TRY(hipMemcpyAsync(total, out + n, sizeof(int), hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

// ---- point grid -------------------------------------------------------------------------------------------------------------------------
#define BQ_BLOCK 256

namespace {

// mm[7]: min xyz, max xyz (ordered keys), non-finite flag
template <class T> __device__ __forceinline__ void bbox_body(const T *__restrict__ xyz, int n, typename bq::GridOf<T>::key *__restrict__ mm)
{
    typedef typename bq::GridOf<T>::key K;
    K lo[3], hi[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = std::numeric_limits<K>::max(); hi[d] = std::numeric_limits<K>::min(); }
    int bad = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const T x = xyz[3 * (int64_t)i + d];
            if (!isfinite(x)) { bad = 1; continue; }
            lo[d] = min(lo[d], bq::enc_ord(x));
            hi[d] = max(hi[d], bq::enc_ord(x));
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[d] = min(lo[d], __shfl_xor(lo[d], o, 64)); hi[d] = max(hi[d], __shfl_xor(hi[d], o, 64)); }
    }
    bad = __ballot(bad) != 0;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int d = 0; d < 3; ++d) { atomicMin(&mm[d], lo[d]); atomicMax(&mm[3 + d], hi[d]); }
        if (bad) atomicOr(&mm[6], (K)1);
    }
}

template <class T> __device__ __forceinline__ void cell_count_body(const T *__restrict__ xyz, int n, const bq::Grid<T> &g, int *__restrict__ cell,
                                                                   int *__restrict__ count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const T x = xyz[3 * (int64_t)i], y = xyz[3 * (int64_t)i + 1], z = xyz[3 * (int64_t)i + 2];
    const int c = (bq::cell_1d(z, g.lo[2], g.h, g.dims[2]) * g.dims[1] + bq::cell_1d(y, g.lo[1], g.h, g.dims[1])) * g.dims[0] + bq::cell_1d(x, g.lo[0], g.h, g.dims[0]);
    cell[i] = c;
    atomicAdd(&count[c], 1);
}

// (the one line that differs between the two scatters)
__device__ __forceinline__ bq::PtF32 point_of(const float *p, int i) { return {p[0], p[1], p[2], i}; }
__device__ __forceinline__ bq::PtF64 point_of(const double *p, int i) { return {p[0], p[1], p[2], i}; }

template <class T> __device__ __forceinline__ void scatter_body(const T *__restrict__ xyz, int n, const int *__restrict__ cell, int *__restrict__ cursor,
                                                                typename bq::GridOf<T>::point *__restrict__ sorted)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int slot = atomicAdd(&cursor[cell[i]], 1);          // (order inside a cell is arbitrary: no query may depend on it)
    if (slot < 0 || slot >= n) return;                        // (cannot happen: the cursors start at the scan of the counts)
    sorted[slot] = point_of(xyz + 3 * (int64_t)i, i);
}

}  // namespace

__global__ __launch_bounds__(BQ_BLOCK) void k_bq_bbox_f32(const float *__restrict__ xyz, int n, int *__restrict__ mm) { bbox_body(xyz, n, mm); }
__global__ __launch_bounds__(BQ_BLOCK) void k_bq_bbox_f64(const double *__restrict__ xyz, int n, unsigned long long *__restrict__ mm) { bbox_body(xyz, n, mm); }
__global__ __launch_bounds__(BQ_BLOCK) void k_bq_cell_count_f32(const float *__restrict__ xyz, int n, bq::Grid<float> g, int *__restrict__ cell, int *__restrict__ count) { cell_count_body(xyz, n, g, cell, count); }
__global__ __launch_bounds__(BQ_BLOCK) void k_bq_cell_count_f64(const double *__restrict__ xyz, int n, bq::Grid<double> g, int *__restrict__ cell, int *__restrict__ count) { cell_count_body(xyz, n, g, cell, count); }
__global__ __launch_bounds__(BQ_BLOCK) void k_bq_scatter_f32(const float *__restrict__ xyz, int n, const int *__restrict__ cell, int *__restrict__ cursor, bq::PtF32 *__restrict__ sorted) { scatter_body(xyz, n, cell, cursor, sorted); }
__global__ __launch_bounds__(BQ_BLOCK) void k_bq_scatter_f64(const double *__restrict__ xyz, int n, const int *__restrict__ cell, int *__restrict__ cursor, bq::PtF64 *__restrict__ sorted) { scatter_body(xyz, n, cell, cursor, sorted); }

// the kernels of a coordinate type
static constexpr auto bbox_kernel(const float *) { return k_bq_bbox_f32; }
static constexpr auto bbox_kernel(const double *) { return k_bq_bbox_f64; }
static constexpr auto cell_count_kernel(const float *) { return k_bq_cell_count_f32; }
static constexpr auto cell_count_kernel(const double *) { return k_bq_cell_count_f64; }
static constexpr auto scatter_kernel(const float *) { return k_bq_scatter_f32; }
static constexpr auto scatter_kernel(const double *) { return k_bq_scatter_f64; }

template <class T> hipError_t bq::bounds(hipStream_t stream, DevBuf &keys, const T *xyz0, int n0, const T *xyz1, int n1, Grid<T> *g, bool finite[2])
{
    typedef typename GridOf<T>::key K;
    const K top = std::numeric_limits<K>::max(), bottom = std::numeric_limits<K>::min();
    const K mm0[14] = {top, top, top, bottom, bottom, bottom, 0, top, top, top, bottom, bottom, bottom, 0};
    K mm[14];
    BQ_TRY(keys.ensure(sizeof(mm0)));
    BQ_TRY(hipMemcpyAsync(keys.p, mm0, sizeof(mm0), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(bbox_kernel(xyz0), dim3(std::min(nblk(n0), 1024)), dim3(BQ_BLOCK), 0, stream, xyz0, n0, keys.as<K>());
    if (xyz1) hipLaunchKernelGGL(bbox_kernel(xyz1), dim3(std::min(nblk(n1), 1024)), dim3(BQ_BLOCK), 0, stream, xyz1, n1, keys.as<K>() + 7);
    BQ_TRY(hipGetLastError());
    BQ_TRY(hipMemcpyAsync(mm, keys.p, sizeof(mm), hipMemcpyDeviceToHost, stream));
    BQ_TRY(hipStreamSynchronize(stream));
    for (int d = 0; d < 3; ++d) { g->lo[d] = dec_ord(mm[d]); g->hi[d] = dec_ord(mm[3 + d]); }
    finite[0] = mm[6] == 0;
    finite[1] = mm[13] == 0;
    return hipSuccess;
}

template <class T> hipError_t bq::build_grid(hipStream_t stream, const T *xyz, int n, const Grid<T> &g, DevBuf &cell, DevBuf &cursor, DevBuf &scan_tmp,
                                             DevBuf &cstart, DevBuf &sorted, int *total)
{
    typedef typename GridOf<T>::point P;
    const int64_t ncell = g.cells();
    BQ_TRY(cell.ensure(sizeof(int) * (size_t)n));
    BQ_TRY(cursor.ensure(sizeof(int) * (size_t)(ncell + 1)));                                    // counts, then the cursors
    BQ_TRY(cstart.ensure(sizeof(int) * (size_t)(ncell + 1)));
    BQ_TRY(sorted.ensure(sizeof(P) * (size_t)n));
    BQ_TRY(hipMemsetAsync(cursor.p, 0, sizeof(int) * (size_t)(ncell + 1), stream));
    hipLaunchKernelGGL(cell_count_kernel(xyz), dim3(nblk(n)), dim3(BQ_BLOCK), 0, stream, xyz, n, g, cell.as<int>(), cursor.as<int>());
    BQ_TRY(hipGetLastError());
    BQ_TRY(scan_exclusive(stream, cursor.as<int>(), (int)ncell, cstart.as<int>(), scan_tmp));
    BQ_TRY(hipMemcpyAsync(cursor.p, cstart.p, sizeof(int) * (size_t)ncell, hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(scatter_kernel(xyz), dim3(nblk(n)), dim3(BQ_BLOCK), 0, stream, xyz, n, cell.as<int>(), cursor.as<int>(), sorted.as<P>());
    BQ_TRY(hipGetLastError());
    // (the total is read once the scatter is queued: one wait for both, after which the caller's xyz is no longer read)
    *total = -1;
    BQ_TRY(hipMemcpyAsync(total, cstart.as<int>() + ncell, sizeof(int), hipMemcpyDeviceToHost, stream));
    return hipStreamSynchronize(stream);
}

template hipError_t bq::bounds<float>(hipStream_t, DevBuf &, const float *, int, const float *, int, Grid<float> *, bool[2]);
template hipError_t bq::bounds<double>(hipStream_t, DevBuf &, const double *, int, const double *, int, Grid<double> *, bool[2]);
template hipError_t bq::build_grid<float>(hipStream_t, const float *, int, const Grid<float> &, DevBuf &, DevBuf &, DevBuf &, DevBuf &, DevBuf &, int *);
template hipError_t bq::build_grid<double>(hipStream_t, const double *, int, const Grid<double> &, DevBuf &, DevBuf &, DevBuf &, DevBuf &, DevBuf &, int *);

// ---- cloud grid -------------------------------------------------------------------------------------------------------------------------
// (returns the CloudStatus of a failed HIP call with the call's text)
#define BQ_CLOUD_TRY(expr)                                                                                     \
    do {                                                                                                       \
        const hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) { CloudStatus s_(CLOUD_HIP); s_.hip = e_; s_.call = #expr; return s_; }          \
    } while (0)

bq::CloudStatus bq::CloudGrid::set_cloud(hipStream_t stream, const float *xyz, int64_t count, bool on_device)
{
    forget();
    BQ_CLOUD_TRY(cloud.ensure(sizeof(float) * 3 * (size_t)count));
    BQ_CLOUD_TRY(hipMemcpyAsync(cloud.p, xyz, sizeof(float) * 3 * (size_t)count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    bool finite[2];
    BQ_CLOUD_TRY(bounds<float>(stream, mm, cloud.as<float>(), (int)count, nullptr, 0, &g, finite));
    if (!finite[0]) return CLOUD_NONFINITE;
    n = (int)count;
    return CLOUD_OK;
}

bq::CloudStatus bq::CloudGrid::bin(hipStream_t stream, double h0)
{
    const double ext[3] = {(double)g.hi[0] - (double)g.lo[0], (double)g.hi[1] - (double)g.lo[1], (double)g.hi[2] - (double)g.lo[2]};
    double h = 0.0;
    const Bins b = keep_or_rebin(CLOUD_GRID_RULE, n, ext, h0, &h_start, &h, g.dims);
    if (b == BINS_KEPT) return CLOUD_OK;
    if (b == BINS_NONE) return CLOUD_NO_GRID;
    // the float the kernels divide by (dims were counted with the double: a cell index that the rounding pushes past them is clamped
    // into the last cell, as every cell index is, which only brings its points into an earlier ring)
    g.h = (float)h;
    if (!(g.h > 0.0f) || !std::isfinite(g.h)) return CLOUD_BAD_CELL;
    int total = -1;
    BQ_CLOUD_TRY(build_grid<float>(stream, cloud.as<float>(), n, g, cell, cursor, scan_tmp, cstart, sorted, &total));
    if (total != n) return CLOUD_BAD_TOTAL;
    h_start = h0;
    return CLOUD_OK;
}

// ---- face grid --------------------------------------------------------------------------------------------------------------------------
// one thread per face: the float64 centroid and rho_f, a hair enlarged so that rounding can only make a bound weaker
__global__ __launch_bounds__(BQ_BLOCK) void k_bq_face_setup(const float *__restrict__ pos, const int *__restrict__ faces, int nf,
                                                            double *__restrict__ cen, double *__restrict__ rho)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int a = faces[3 * (int64_t)f], b = faces[3 * (int64_t)f + 1], c = faces[3 * (int64_t)f + 2];
    double m[3];
    const double r = bq::face_centroid(pos + 3 * (int64_t)a, pos + 3 * (int64_t)b, pos + 3 * (int64_t)c, m);
    cen[3 * (int64_t)f] = m[0];
    cen[3 * (int64_t)f + 1] = m[1];
    cen[3 * (int64_t)f + 2] = m[2];
    rho[f] = r * (1.0 + BQ_FACE_RHO_SLACK);
}

// out[0] = the largest rho, out[1] = their sum: one workgroup, a butterfly within each wave, then the four waves in order.  The sum is
// an input to the cell size and so to every walk's statistics: its order is fixed.
__global__ __launch_bounds__(BQ_BLOCK) void k_bq_rho_reduce(const double *__restrict__ rho, int nf, double *__restrict__ out)
{
    __shared__ double s_m[BQ_BLOCK / 64], s_s[BQ_BLOCK / 64];
    double m = 0.0, s = 0.0;
    for (int j = threadIdx.x; j < nf; j += BQ_BLOCK) { m = fmax(m, rho[j]); s += rho[j]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmax(m, __shfl_xor(m, o, 64)); s += __shfl_xor(s, o, 64); }
    if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_s[threadIdx.x >> 6] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
        out[1] = ((s_s[0] + s_s[1]) + s_s[2]) + s_s[3];
    }
}

hipError_t bq::face_setup(hipStream_t stream, const float *pos, const int *faces, int nf, double *cen, double *rho)
{
    hipLaunchKernelGGL(k_bq_face_setup, dim3(nblk(nf)), dim3(BQ_BLOCK), 0, stream, pos, faces, nf, cen, rho);
    return hipGetLastError();
}

// (returns the FaceStatus of a failed HIP call with the call's text)
#define BQ_FACE_TRY(expr)                                                                                      \
    do {                                                                                                       \
        const hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) { FaceStatus s_(FACES_HIP); s_.hip = e_; s_.call = #expr; return s_; }           \
    } while (0)

bq::FaceStatus bq::FaceGrid::set_faces(hipStream_t stream, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, Setup own,
                                       void *user)
{
    nf = 0;
    nv = 0;
    h_start = 0.0;
    const int n = (int)n_faces;
    BQ_FACE_TRY(upload(stream, mpos, pos, 3 * n_vertices));
    BQ_FACE_TRY(upload(stream, mfaces, faces, 3 * n_faces));
    BQ_FACE_TRY(cen.ensure(sizeof(double) * 3 * (size_t)n));
    BQ_FACE_TRY(rho.ensure(sizeof(double) * (size_t)n));
    BQ_FACE_TRY(red.ensure(sizeof(double) * 2));
    if (own) BQ_FACE_TRY(own(user, stream, mpos.as<float>(), n_vertices, mfaces.as<int>(), n, cen.as<double>(), rho.as<double>()));
    else BQ_FACE_TRY(face_setup(stream, mpos.as<float>(), mfaces.as<int>(), n, cen.as<double>(), rho.as<double>()));
    hipLaunchKernelGGL(k_bq_rho_reduce, dim3(1), dim3(BQ_BLOCK), 0, stream, rho.as<double>(), n, red.as<double>());
    BQ_FACE_TRY(hipGetLastError());
    double r[2] = {0.0, 0.0};
    BQ_FACE_TRY(hipMemcpyAsync(r, red.p, sizeof(r), hipMemcpyDeviceToHost, stream));
    BQ_FACE_TRY(hipStreamSynchronize(stream));                    // (r is a stack array, and the uploads' sources are the caller's)
    bool finite[2];
    BQ_FACE_TRY(bounds<double>(stream, mm, cen.as<double>(), n, nullptr, 0, &g, finite));
    if (!finite[0] || !std::isfinite(r[0]) || !std::isfinite(r[1])) return FACES_NONFINITE;
    if (!std::isfinite(emax())) return FACES_BAD_EXTENT;
    rho_max = r[0];
    rho_mean = r[1] / (double)n;
    nv = n_vertices;
    nf = n;
    return FACES_OK;
}

bq::FaceStatus bq::FaceGrid::bin(hipStream_t stream, double h0)
{
    const double ext[3] = {g.hi[0] - g.lo[0], g.hi[1] - g.lo[1], g.hi[2] - g.lo[2]};
    const Bins b = face_bins(nf, ext, h0, &h_start, &g.h, g.dims);
    if (b == BINS_KEPT) return FACES_OK;
    if (b == BINS_NONE) return FACES_NO_GRID;
    int total = -1;
    BQ_FACE_TRY(build_grid<double>(stream, cen.as<double>(), nf, g, cell, ccount, scan_tmp, cstart, sorted, &total));
    if (total != nf) return FACES_BAD_TOTAL;
    h_start = h0;
    return FACES_OK;
}
