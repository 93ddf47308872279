// What the query units (nw_holepunch.hip, nw_surgery.hip, nw_isosurface.hip, nw_evaluation.hip, nw_simulation.hip) share: the device
// buffer and the staging of host arrays into it, the base of their contexts with its create / destroy / last_error bodies, the HIP-call
// macro, the host checks of a mesh and of finiteness, the ordered-key maps, the exclusive scan, the point grid (bounding box, sizing,
// counting sort by cell, the cell index of a coordinate) in float and in double, the cloud grid of the four cloud query units (the
// intake of a cloud: the copy, its box, its finiteness; and its binning at a cell size), the face grid of the six mesh query units (the
// intake of a mesh: centroids, radii, their reduction, the centroids' box; and their binning at a cell size), and the host loop of the
// 64-bit radix select.  Kernels and host entries are in nw_bq.hip; what needs no HIP is in nw_bq_core.h.  Each C-ABI keeps its own
// status codes and error texts: everything here that can fail returns a hipError_t, a flag, a CloudStatus or a FaceStatus, and its user
// says what that means (cloud_fail and face_fail hold the words the units share; the prefix and the status are the unit's).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <string>
#include <algorithm>
#include <numeric>

#include "nw_bq_core.h"

namespace bq {

// monotone float <-> int and double <-> 64-bit maps (atomicMin / atomicMax on floating-point values)
__host__ __device__ __forceinline__ int enc_ord(float f)
{
    const int i = __builtin_bit_cast(int, f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}

__host__ __device__ __forceinline__ float dec_ord(int v) { return __builtin_bit_cast(float, v >= 0 ? v : v ^ 0x7fffffff); }

__host__ __device__ __forceinline__ unsigned long long enc_ord(double d)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__host__ __device__ __forceinline__ double dec_ord(unsigned long long e)
{
    return __builtin_bit_cast(double, (e >> 63) ? (e ^ 0x8000000000000000ull) : ~e);
}

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t b)
    {
        if (b <= bytes && p) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, std::max<size_t>(b, 256));
        if (e == hipSuccess) bytes = std::max<size_t>(b, 256);
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T *as() const { return (T *)p; }
};

// what every context starts with; its DevBuf members free themselves when destroy() deletes it
struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
};

inline int fail(Ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

// (expects `ctx` in scope; returns the user's ABI's out-of-memory or HIP status with the call's text in last_error)
#define BQ_HIP(call, ERR_NOMEM, ERR_HIP)                                                                       \
    do {                                                                                                       \
        hipError_t e_ = (call);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return bq::fail(ctx, e_ == hipErrorOutOfMemory ? (ERR_NOMEM) : (ERR_HIP), std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// (for what returns a hipError_t itself)
#define BQ_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

inline int nblk(int64_t n, int b = 256) { return (int)((n + b - 1) / b); }

template <class C> int create(int device, C **out, int err_badarg, int err_hip)
{
    if (!out || device < 0) return err_badarg;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return err_hip;
    if (device >= ndev) return err_badarg;
    if (hipSetDevice(device) != hipSuccess) return err_hip;
    C *ctx = new C();
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return err_hip; }
    *out = ctx;
    return 0;
}

template <class C> void destroy(C *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    const hipStream_t stream = ctx->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete ctx;                                               // (the buffers go first, then the stream they were used on)
    if (stream) (void)hipStreamDestroy(stream);
}

inline const char *last_error(const Ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

// ---- host arrays ------------------------------------------------------------------------------------------------------------------------
template <class T> bool all_finite(const T *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// host-side check of the mesh arguments (before any HIP call): sizes within the limits of the int kernels, pos finite, faces in range
inline bool mesh_ok(const float *pos, int64_t nv, const int32_t *faces, int64_t nf)
{
    if (!pos || !faces || nv < 3 || nf < 1 || nv > (1ll << 30) || nf > (1ll << 29)) return false;
    if (!all_finite(pos, 3 * nv)) return false;
    for (int64_t i = 0; i < 3 * nf; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return false;
    return true;
}

// src[0..n) into buf on `stream` (the copy is asynchronous: src must outlive the stream's next synchronisation)
template <class T> hipError_t upload(hipStream_t stream, DevBuf &buf, const T *src, int64_t n)
{
    BQ_TRY(buf.ensure(sizeof(T) * (size_t)n));
    return hipMemcpyAsync(buf.p, src, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, stream);
}

// whether kernels can read p in place (device memory); a host pointer is to be uploaded first
inline bool on_device(const void *p)
{
    hipPointerAttribute_t attr;
    const bool dev = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();                                  // (a host pointer leaves an error behind on some runtimes)
    return dev;
}

// ---- exclusive scan (nw_bq.hip) ---------------------------------------------------------------------------------------------------------
// exclusive scan of in[0..n) on `stream`: out[0..n] with out[n] = the total; tmp holds the tile sums
hipError_t scan_exclusive(hipStream_t stream, const int *in, int n, int *out, DevBuf &tmp);

// the same, and out[n] read back into *total: the stream is synchronised.  What range the total may lie in is its user's to check.
hipError_t scan_total(hipStream_t stream, const int *in, int n, int *out, DevBuf &tmp, int *total);

// ---- point grid (nw_bq.hip), T = float or double ----------------------------------------------------------------------------------------
// a cloud's bounding box cut into cubes of side h; cell (x, y, z) has the id (z * dims[1] + y) * dims[0] + x
template <class T> struct Grid {
    T lo[3], hi[3];
    T h;
    int dims[3];
    int64_t cells() const { return (int64_t)dims[0] * dims[1] * dims[2]; }
};

// the ordered key of a coordinate, and a point in cell order: its coordinates and its index in the caller's array.  The fourth word of
// a float point is that index as an int, not a float: a kernel that needs the coordinates only may read the point as a float4 and
// leave .w alone (hole punching, the neighbour unit).
struct PtF64 { double x, y, z; long long i; };
template <class T> struct GridOf;
template <> struct GridOf<float> { typedef int key; typedef PtF32 point; };
template <> struct GridOf<double> { typedef unsigned long long key; typedef PtF64 point; };

// cell index along one axis: the same expression for binning and for every query
template <class T> __device__ __forceinline__ int cell_1d(T x, T lo, T h, int dim)
{
    const T t = floor((x - lo) / h);
    // (clamped as a T first: a coordinate far outside the box must not overflow the int conversion)
    return (int)fmin(fmax(t, (T)0), (T)(dim - 1));
}

// bounding box of xyz0[0..n0) into g->lo / g->hi (over its finite coordinates) and finite[k] = whether every coordinate of cloud k is
// finite; the second cloud may be absent (nullptr).  `keys` holds the ordered keys; one round trip, the stream is synchronised.
template <class T> hipError_t bounds(hipStream_t stream, DevBuf &keys, const T *xyz0, int n0, const T *xyz1, int n1, Grid<T> *g, bool finite[2]);

// counting sort of xyz[0..n) by cell of g (count, scan, scatter): cstart[0 .. cells] = where each cell's points start in `sorted`
// (GridOf<T>::point, in arbitrary order within a cell); *total = cstart[cells], which is n unless something went wrong.  `cell` and
// `cursor` are work buffers; the stream is synchronised.
template <class T> hipError_t build_grid(hipStream_t stream, const T *xyz, int n, const Grid<T> &g, DevBuf &cell, DevBuf &cursor, DevBuf &scan_tmp,
                                         DevBuf &cstart, DevBuf &sorted, int *total);

// ---- cloud grid (nw_bq.hip) -------------------------------------------------------------------------------------------------------------
// What the cloud query units (nw_neighbours, nw_clustering, nw_pairs, nw_structure) do with a cloud before they walk it: the copy onto
// the device, its box and finiteness, and the cloud binned into the float point grid, a sorted point carrying its index.

// how taking a cloud in or binning it ended; every C-ABI gives that its own status and its own text (cloud_fail)
enum CloudCheck {
    CLOUD_OK = 0,
    CLOUD_NONFINITE,          // a localization is not finite
    CLOUD_NO_GRID,            // no cell size keeps the grid within its cap
    CLOUD_BAD_CELL,           // the cell size is not a positive float
    CLOUD_BAD_TOTAL,          // the cell counts do not add up to the cloud
    CLOUD_HIP                 // a HIP call failed: `hip`, and `call` names it
};

struct CloudStatus {
    CloudCheck check = CLOUD_OK;
    hipError_t hip = hipSuccess;
    const char *call = "";
    CloudStatus(CloudCheck c = CLOUD_OK) : check(c) {}
    bool ok() const { return check == CLOUD_OK; }
};

// the statuses of a C-ABI that a CloudStatus maps to
struct CloudCodes { int badarg, nonfinite, nomem, hip; };

// a failed CloudStatus as the ABI's status, with "<who>: <what>" in last_error (who = the ABI's function for an intake, its prefix for a
// binning)
inline int cloud_fail(Ctx *ctx, const char *who, const CloudStatus &s, const CloudCodes &c)
{
    const std::string w = std::string(who) + ": ";
    switch (s.check) {
    case CLOUD_NONFINITE: return fail(ctx, c.nonfinite, w + "a localization is not finite");
    case CLOUD_NO_GRID: return fail(ctx, c.badarg, w + "no cell size keeps the grid within its cap");
    case CLOUD_BAD_CELL: return fail(ctx, c.badarg, w + "the cell size is not a positive float");
    case CLOUD_BAD_TOTAL: return fail(ctx, c.hip, w + "the cell counts do not add up to the cloud");
    default: return fail(ctx, s.hip == hipErrorOutOfMemory ? c.nomem : c.hip, w + s.call + ": " + hipGetErrorString(s.hip));
    }
}

// A unit checks its arguments itself, before any HIP call and before it looks at its context: NULL, n, on_device, and the finiteness of
// a host array.  What a host array with a non-finite value does to a cloud taken in earlier differs between the units and is part of
// their ABIs: pairs and structure forget() it (a failed call leaves no cloud, whichever check failed), neighbours and clustering
// return before anything is reset and keep answering from it.
struct CloudGrid {
    int n = 0;                    // 0: no cloud
    Grid<float> g{};              // lo, hi: the cloud's box; h, dims: the grid at hand
    double h_start = 0.0;         // the cell size the grid at hand was sized from (0: none)
    DevBuf cloud, mm, cell, cursor, cstart, sorted, scan_tmp;

    void forget() { n = 0; h_start = 0.0; }

    // Takes in xyz[0..3 count) from the host or the device: the copy, its box, and the device's verdict on its finiteness.  The stream
    // is synchronised: the caller's array is free afterwards.  n stays 0 unless all is well, and the grid at hand is forgotten either
    // way.
    CloudStatus set_cloud(hipStream_t stream, const float *xyz, int64_t count, bool on_device);

    // the widest axis of the cloud's box
    double emax() const
    {
        double e = 0.0;
        for (int d = 0; d < 3; ++d) e = std::max(e, (double)g.hi[d] - (double)g.lo[d]);
        return e;
    }

    // The grid for the starting cell size h0 (cloud_cell of the unit's candidate, or the neighbour unit's own rule): the one at hand if
    // it was sized from the same h0, else the cloud binned anew under CLOUD_GRID_RULE (keep_or_rebin, build_grid: `sorted` holds the
    // cloud as PtF32 in cell order, cstart the cells' starts), which synchronises the stream once.
    CloudStatus bin(hipStream_t stream, double h0);
};

// ---- face grid (nw_bq.hip) --------------------------------------------------------------------------------------------------------------
// What the mesh query units (nw_distance, nw_intersections, nw_rays, nw_volume, nw_proximity, nw_mapping) do with a mesh before they walk
// it: every face's float64 centroid and radius rho_f (face_centroid, enlarged by BQ_FACE_RHO_SLACK), rho_max and the mean rho_f, the
// centroids' box, and the centroids binned into the double point grid, a sorted point carrying its face id.

// how taking a mesh in or binning it ended; every C-ABI gives that its own status and its own text (face_fail)
enum FaceCheck {
    FACES_OK = 0,
    FACES_BAD_SIZE,           // a NULL array or a size out of range
    FACES_BAD_POSITION,       // a vertex position is not finite
    FACES_BAD_INDEX,          // a face index outside the vertices
    FACES_NONFINITE,          // a face's centroid or radius is not a finite double
    FACES_BAD_EXTENT,         // the mesh's extent is not a finite double
    FACES_NO_GRID,            // no cell size keeps the grid within its cap
    FACES_BAD_TOTAL,          // the cell counts do not add up to the faces
    FACES_HIP                 // a HIP call failed: `hip`, and `call` names it
};

struct FaceStatus {
    FaceCheck check = FACES_OK;
    hipError_t hip = hipSuccess;
    const char *call = "";
    FaceStatus(FaceCheck c = FACES_OK) : check(c) {}
    bool ok() const { return check == FACES_OK; }
};

// the host checks of a mesh's arguments, in this order and before any HIP call: NULL or sizes beyond the int kernels, finiteness of pos,
// range of the face indices
inline FaceStatus check_faces(const float *pos, int64_t nv, const int32_t *faces, int64_t nf)
{
    if (!pos || !faces || nv < 3 || nf < 1 || nv > (1ll << 30) || nf > (1ll << 29)) return FACES_BAD_SIZE;
    if (!all_finite(pos, 3 * nv)) return FACES_BAD_POSITION;
    for (int64_t i = 0; i < 3 * nf; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return FACES_BAD_INDEX;
    return FACES_OK;
}

// a half-edge twin table: -1 (a border) or an involution within [0, 3F)
inline bool twin_ok(const int32_t *twin, int64_t nf)
{
    const int64_t nh = 3 * nf;
    for (int64_t h = 0; h < nh; ++h) {
        const int32_t t = twin[h];
        if (t == -1) continue;
        if (t < 0 || t >= nh || twin[t] != h) return false;
    }
    return true;
}

// the statuses of a C-ABI that a FaceStatus maps to
struct FaceCodes { int badarg, nonfinite, nomem, hip; };

// a failed FaceStatus as the ABI's status, with "<who>: <what>" in last_error (who = the ABI's function)
inline int face_fail(Ctx *ctx, const char *who, const FaceStatus &s, const FaceCodes &c)
{
    const std::string w = std::string(who) + ": ";
    switch (s.check) {
    case FACES_BAD_SIZE: return fail(ctx, c.badarg, w + "a NULL array or a size out of range");
    case FACES_BAD_POSITION: return fail(ctx, c.nonfinite, w + "a vertex position is not finite");
    case FACES_BAD_INDEX: return fail(ctx, c.badarg, w + "a face index outside the vertices");
    case FACES_NONFINITE: return fail(ctx, c.nonfinite, w + "a face's centroid or radius is not a finite double");
    case FACES_BAD_EXTENT: return fail(ctx, c.badarg, w + "the mesh's extent is not a finite double");
    case FACES_NO_GRID: return fail(ctx, c.badarg, w + "no cell size keeps the grid within its cap");
    case FACES_BAD_TOTAL: return fail(ctx, c.hip, w + "the cell counts do not add up to the faces");
    default: return fail(ctx, s.hip == hipErrorOutOfMemory ? c.nomem : c.hip, w + s.call + ": " + hipGetErrorString(s.hip));
    }
}

// centroid and radius of faces[0..nf) into cen (3 per face) and rho on `stream` (k_bq_face_setup); nothing is waited for
hipError_t face_setup(hipStream_t stream, const float *pos, const int *faces, int nf, double *cen, double *rho);

struct FaceGrid {
    int nf = 0;                   // 0: no mesh
    int64_t nv = 0;
    double rho_max = 0.0, rho_mean = 0.0;
    Grid<double> g{};             // lo, hi: the centroids' box; h, dims: the grid at hand
    double h_start = 0.0;         // the cell size the grid at hand was sized from (0: none)
    DevBuf mpos, mfaces, cen, rho, red, mm, cell, ccount, cstart, sorted, scan_tmp;

    // a unit's own kernel in place of k_bq_face_setup, queued on the stream between the uploads and the reduction (the mapping
    // unit's also scatters the faces' areas)
    typedef hipError_t (*Setup)(void *user, hipStream_t stream, const float *pos, int64_t nv, const int *faces, int nf, double *cen, double *rho);

    // Takes in a mesh that check_faces has passed: the uploads, centroids and radii, their reduction (k_bq_rho_reduce), the centroids'
    // box, and the checks that all of it is finite.  The stream is synchronised: the caller's arrays are free afterwards.  nf stays 0
    // unless all is well, and the grid at hand is forgotten either way.
    FaceStatus set_faces(hipStream_t stream, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, Setup own = nullptr,
                         void *user = nullptr);

    // the widest axis of the centroids' box
    double emax() const
    {
        double e = 0.0;
        for (int d = 0; d < 3; ++d) e = std::max(e, g.hi[d] - g.lo[d]);
        return e;
    }

    // The grid for the starting cell size h0 (face_cell of the unit's candidate): the one at hand if it was sized from the same h0, else
    // the centroids binned anew (face_bins, build_grid), which synchronises the stream.
    FaceStatus bin(hipStream_t stream, double h0);
};

// ---- radix select -----------------------------------------------------------------------------------------------------------------------
// The key of a given rank among the 64-bit keys that `pass` sees, a byte per pass from `shift` down.  pass(prefix, shift, hist) launches
// one histogram pass on `stream` (bin radix_bin(key, prefix, shift) of every key, added to the 256 device counters at hist);
// rank_of(total) names the 0-based rank once the first pass has counted the keys.  *rank = the rank that is left among the keys equal
// to *key, or -1 if a histogram did not hold the rank (an empty set of keys is one way).
template <class Pass, class RankOf>
hipError_t select_u64(hipStream_t stream, unsigned *hist, int shift, Pass pass, RankOf rank_of, uint64_t *key, int64_t *rank)
{
    uint64_t prefix = 0;
    *rank = -1;
    for (bool first = true; shift >= 0; shift -= 8, first = false) {
        unsigned h[256];
        BQ_TRY(hipMemsetAsync(hist, 0, sizeof(h), stream));
        pass(prefix, shift, hist);
        BQ_TRY(hipGetLastError());
        BQ_TRY(hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, stream));
        BQ_TRY(hipStreamSynchronize(stream));
        if (first) *rank = rank_of(std::accumulate(h, h + 256, (int64_t)0));
        const int b = select_bin(h, *rank);
        if (b < 0) { *rank = -1; return hipSuccess; }
        prefix = (prefix << 8) | (uint64_t)b;
    }
    *key = prefix;
    return hipSuccess;
}

}  // namespace bq
