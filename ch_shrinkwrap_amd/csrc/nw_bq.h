// What the block-boundary query units (nw_holepunch.hip, nw_surgery.hip) share: the device buffer, the base of their contexts with its
// create / destroy / last_error bodies, the HIP-call macro, the host check of a mesh, the ordered-int map and the exclusive scan
// (kernels and host entry in nw_bq.hip).  Each C-ABI keeps its own status codes: what needs one takes it from its user.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <string>
#include <algorithm>

namespace bq {

// monotone float <-> int map (atomicMin / atomicMax on floats)
__host__ __device__ __forceinline__ int enc_ord(float f)
{
    const int i = __builtin_bit_cast(int, f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}

__host__ __device__ __forceinline__ float dec_ord(int v) { return __builtin_bit_cast(float, v >= 0 ? v : v ^ 0x7fffffff); }

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

// host-side check of the mesh arguments (before any HIP call): sizes within the limits of the int kernels, pos finite, faces in range
inline bool mesh_ok(const float *pos, int64_t nv, const int32_t *faces, int64_t nf)
{
    if (!pos || !faces || nv < 3 || nf < 1 || nv > (1ll << 30) || nf > (1ll << 29)) return false;
    for (int64_t i = 0; i < 3 * nv; ++i)
        if (!std::isfinite(pos[i])) return false;
    for (int64_t i = 0; i < 3 * nf; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return false;
    return true;
}

// exclusive scan of in[0..n) on `stream`: out[0..n] with out[n] = the total; tmp holds the tile sums (nw_bq.hip)
hipError_t scan_exclusive(hipStream_t stream, const int *in, int n, int *out, DevBuf &tmp);

}  // namespace bq
