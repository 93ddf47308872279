// The exclusive scan of the block-boundary query units (nw_bq.h): int, three launches, exact.  It lives in a unit of its own because a
// __global__ function defined in two units collides at link time through its host stubs.  The per-iteration scan of nanowrap.hip
// (nw_kernels.h: fused tile sums, recorded in the block's hipGraph) is a different one.
//
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
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
    const hipError_t e = tmp.ensure(sizeof(int) * (size_t)(nb + 1));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bq_scan_tiles, dim3(nb), dim3(BQ_SCAN_BLOCK), 0, stream, in, n, tmp.as<int>());
    hipLaunchKernelGGL(k_bq_scan_bsums, dim3(1), dim3(1024), 0, stream, tmp.as<int>(), nb);
    hipLaunchKernelGGL(k_bq_scan_final, dim3(nb), dim3(BQ_SCAN_BLOCK), 0, stream, in, n, tmp.as<int>(), out);
    return hipGetLastError();
}
