// Block-boundary surgery queries on the device (MI355X, gfx950): include/nw_surgery.h.
//
// remove_necks and remove_extra_short_edges (upstream _membrane_mesh.pyx:1201-1239) and remove_inner_surfaces ask mesh-wide questions
// that host code would answer in O(faces) Python passes or, for the winding numbers, in O(queries x faces):
//   k_ws_init / k_ws_hook / k_ws_compress   union-find over the twin table (ECL-CC): a face hooks the larger of two roots onto the smaller
//                                           with atomicCAS, so every root is its component's minimum face id whatever the schedule; one
//                                           hooking launch, however long the component (no propagation rounds);
//   bq::scan_total + k_ws_number            roots are flagged, scanned (the query units' shared scan, nw_bq.h) and every face
//                                           takes its root's rank: labels in order of the components' smallest face ids;
//   k_ws_stats                              one thread per face, float64 terms turned into 64-bit fixed point and summed by wave when the
//                                           wave's faces share a label (the usual case), by lane otherwise: integer sums, the same bytes
//                                           on every run;
//   k_ws_active / k_ws_winding              one thread per face and eight queries per workgroup: solid angles in float64, summed in fixed
//                                           point per (query, component); a (query, component) pair outside the component's box is not
//                                           evaluated;
//   k_ws_lengths / k_ws_hist / k_ws_pick    half-edge lengths (float32, no contraction: -ffp-contract=off) and a radix select of the two
//                                           middle elements over their bits (non-negative floats order as their bit patterns), four passes
//                                           of 8 bits, no sort;
//   k_ws_flag                               heads of the half-edges shorter than threshold * median.
//
// All stores are vector stores; no kernel uses scratch (build.py's KERNEL_BUDGETS checks it).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cmath>
#include <cfloat>
#include <climits>
#include <string>
#include <vector>
#include <algorithm>

#include "../../include/nw_surgery.h"
#include "nw_bq.h"
#include "nw_device.h"

#define NWS_EXPORT extern "C" __attribute__((visibility("default")))
#define NWS_BLOCK 256
#define NWS_WQ 8                    // queries per k_ws_winding workgroup
#define NWS_WF 4                    // faces per k_ws_winding thread

typedef long long i64;
typedef unsigned long long u64;

// ---- union-find (ECL-CC) ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ws_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of v with path halving; parent[x] <= x always (hooking only ever lowers it), so the walk ends at the smallest id of the tree
__device__ int ws_find(int *parent, int v)
{
    int p = ws_load(&parent[v]);
    while (true) {
        const int gp = ws_load(&parent[p]);
        if (gp == p) return p;
        __hip_atomic_store(&parent[v], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (any ancestor is a valid parent)
        v = p;
        p = gp;
    }
}

__global__ __launch_bounds__(NWS_BLOCK) void k_ws_init(const unsigned char *__restrict__ mask, int nf, int *__restrict__ parent)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    parent[f] = (mask == nullptr || mask[f]) ? f : -1;
}

__global__ __launch_bounds__(NWS_BLOCK) void k_ws_hook(const int *__restrict__ twin, int nf, int *parent)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf || ws_load(&parent[f]) < 0) return;
    for (int k = 0; k < 3; ++k) {
        const int t = twin[3 * f + k];
        if (t < 0) continue;
        const int g = t / 3;
        if (g <= f || ws_load(&parent[g]) < 0) continue;        // (each edge once, from its smaller face)
        int a = ws_find(parent, f), b = ws_find(parent, g);
        while (a != b) {
            if (a > b) { const int s = a; a = b; b = s; }
            // hook root b onto a; if b is no longer a root, climb from what it points to now
            const int old = atomicCAS(&parent[b], b, a);
            if (old == b) break;
            b = ws_find(parent, old);
        }
    }
}

// root[f] = the root of f (a separate array: concurrent path halving may still rewrite parent[] while this runs)
__global__ __launch_bounds__(NWS_BLOCK) void k_ws_compress(int nf, int *parent, int *__restrict__ root, int *__restrict__ is_root)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    if (ws_load(&parent[f]) < 0) { root[f] = -1; is_root[f] = 0; return; }
    const int r = ws_find(parent, f);
    root[f] = r;
    is_root[f] = (r == f) ? 1 : 0;
}

__global__ __launch_bounds__(NWS_BLOCK) void k_ws_number(int nf, const int *__restrict__ rank, int *__restrict__ label /* in: root, out: label */)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const int r = label[f];
    label[f] = r < 0 ? -1 : rank[r];
}

// ---- per-component statistics ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ i64 ws_wave_sum(i64 v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int ws_wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int ws_wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// the label every lane of the wave holds (lanes with -1 aside), or -2 if they differ; -1 if no lane holds one
__device__ __forceinline__ int ws_wave_label(int lab)
{
    const u64 live = __ballot(lab >= 0);
    if (live == 0ull) return -1;
    const int first = __shfl(lab, __ffsll((unsigned long long)live) - 1, 64);
    return __ballot(lab >= 0 && lab != first) == 0ull ? first : -2;
}

struct ws_acc {
    u64 *count, *area, *vol, *border;      // C each (fixed point for area / vol, two's complement in u64)
    u64 *nrm;                              // 3C: sum of (p1 - p0) x (p2 - p0), fixed point (the volume's change of origin)
    int *bbox;                             // 6C ordered ints
};

// the frame of one call: terms are taken relative to o (the float32 centre of pos's bounding box), so that their fixed-point scales follow
// the mesh's extent and not its distance from the origin
struct ws_frame {
    double o[3];
    double s_area, s_vol, s_nrm;
};

__global__ __launch_bounds__(NWS_BLOCK) void k_ws_stats(const float *__restrict__ pos, const int *__restrict__ faces, const int *__restrict__ twin,
                                                        const int *__restrict__ label, int nf, ws_frame fr, ws_acc acc)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const int lab = f < nf ? label[f] : -1;
    i64 ca = 0, cv = 0, cb = 0, cc = 0, cn[3] = {0, 0, 0};
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    if (lab >= 0) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        // (a float32 minus the float32 centre is exact in float64 unless the two are 2^29 apart)
        const double x0 = (double)pos[3 * i0] - fr.o[0], y0 = (double)pos[3 * i0 + 1] - fr.o[1], z0 = (double)pos[3 * i0 + 2] - fr.o[2];
        const double x1 = (double)pos[3 * i1] - fr.o[0], y1 = (double)pos[3 * i1 + 1] - fr.o[1], z1 = (double)pos[3 * i1 + 2] - fr.o[2];
        const double x2 = (double)pos[3 * i2] - fr.o[0], y2 = (double)pos[3 * i2 + 1] - fr.o[1], z2 = (double)pos[3 * i2 + 2] - fr.o[2];
        const double ax = x1 - x0, ay = y1 - y0, az = z1 - z0, bx = x2 - x0, by = y2 - y0, bz = z2 - z0;
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double area = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
        const double vol = (x0 * (y1 * z2 - z1 * y2) + y0 * (z1 * x2 - x1 * z2) + z0 * (x1 * y2 - y1 * x2)) / 6.0;
        // p0 . (p1 x p2) = q0 . (q1 x q2) + o . ((q1 - q0) x (q2 - q0)) with q = p - o: the second part is summed apart, added on the host
        ca = llrint(area * fr.s_area);
        cv = llrint(vol * fr.s_vol);
        cn[0] = llrint(cx * fr.s_nrm);
        cn[1] = llrint(cy * fr.s_nrm);
        cn[2] = llrint(cz * fr.s_nrm);
        cc = 1;
        for (int k = 0; k < 3; ++k) {
            const int t = twin[3 * f + k];
            cb += (t < 0 || label[t / 3] != lab) ? 1 : 0;
        }
        const int ids[3] = {i0, i1, i2};
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d) { const int o = bq::enc_ord(pos[3 * ids[c] + d]); lo[d] = min(lo[d], o); hi[d] = max(hi[d], o); }
    }
    // one atomic per wave when every lane of the wave holds a face of the same component (lanes without a face join any wave)
    const int wl = ws_wave_label(lab);
    int c = lab;
    if (wl == -1) return;
    if (wl >= 0) {
        ca = ws_wave_sum(ca); cv = ws_wave_sum(cv); cb = ws_wave_sum(cb); cc = ws_wave_sum(cc);
        for (int d = 0; d < 3; ++d) cn[d] = ws_wave_sum(cn[d]);
        for (int d = 0; d < 3; ++d) { lo[d] = ws_wave_min(lo[d]); hi[d] = ws_wave_max(hi[d]); }
        if ((threadIdx.x & 63) != 0) return;
        c = wl;
    }
    if (c < 0) return;
    atomicAdd(&acc.count[c], (u64)cc);
    atomicAdd(&acc.area[c], (u64)ca);
    atomicAdd(&acc.vol[c], (u64)cv);
    atomicAdd(&acc.border[c], (u64)cb);
    for (int d = 0; d < 3; ++d) atomicAdd(&acc.nrm[3 * c + d], (u64)cn[d]);
    for (int d = 0; d < 3; ++d) { atomicMin(&acc.bbox[6 * c + d], lo[d]); atomicMax(&acc.bbox[6 * c + 3 + d], hi[d]); }
}

__global__ __launch_bounds__(NWS_BLOCK) void k_ws_bbox_init(int *__restrict__ bbox, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bbox[i] = (i % 6) < 3 ? INT_MAX : INT_MIN;
}

// ---- winding numbers ---------------------------------------------------------------------------------------------------------------
// active[q * C + c] = 1 if component c is evaluated for query q: not the query's own, and its box holds the point
__global__ __launch_bounds__(NWS_BLOCK) void k_ws_active(const float *__restrict__ queries, const int *__restrict__ qcomp, int nq, int nc,
                                                         const int *__restrict__ bbox, unsigned char *__restrict__ active)
{
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (i64)nq * nc) return;
    const int q = (int)(i / nc), c = (int)(i % nc);
    bool in = qcomp == nullptr || qcomp[q] != c;
    for (int d = 0; d < 3 && in; ++d) {
        const float x = queries[3 * q + d];
        in = bbox[6 * c + d] != INT_MAX && x >= bq::dec_ord(bbox[6 * c + d]) && x <= bq::dec_ord(bbox[6 * c + 3 + d]);
    }
    active[i] = in ? 1 : 0;
}

// the NWS_WQ sums of every lane go to their (query, component) accumulators: one atomic per wave and query when the wave's labels agree
__device__ __forceinline__ void ws_flush(u64 *__restrict__ wacc, int nc, int q0, int nq, int lab, i64 *acc)
{
    const int wl = ws_wave_label(lab);
#pragma unroll
    for (int j = 0; j < NWS_WQ; ++j) {
        if (wl >= 0) {
            const i64 s = ws_wave_sum(acc[j]);
            if ((threadIdx.x & 63) == 0 && q0 + j < nq && s != 0) atomicAdd(&wacc[(i64)(q0 + j) * nc + wl], (u64)s);
        } else if (lab >= 0 && q0 + j < nq && acc[j] != 0) {
            atomicAdd(&wacc[(i64)(q0 + j) * nc + lab], (u64)acc[j]);
        }
        acc[j] = 0;
    }
}

// grid (face tiles, query groups): thread t of a workgroup takes faces base + t + 256 k (k < NWS_WF), for NWS_WQ queries at once
__global__ __launch_bounds__(NWS_BLOCK) void k_ws_winding(const float *__restrict__ pos, const int *__restrict__ faces, const int *__restrict__ label,
                                                          int nf, int nc, const float *__restrict__ queries, int nq,
                                                          const unsigned char *__restrict__ active, double scale, u64 *__restrict__ wacc)
{
    const int q0 = blockIdx.y * NWS_WQ;
    double qx[NWS_WQ], qy[NWS_WQ], qz[NWS_WQ];
#pragma unroll
    for (int j = 0; j < NWS_WQ; ++j) {
        const int q = min(q0 + j, nq - 1);
        qx[j] = queries[3 * q]; qy[j] = queries[3 * q + 1]; qz[j] = queries[3 * q + 2];
    }
    i64 acc[NWS_WQ];
#pragma unroll
    for (int j = 0; j < NWS_WQ; ++j) acc[j] = 0;
    int cur = -1;
    const int base = blockIdx.x * (NWS_BLOCK * NWS_WF) + threadIdx.x;
    for (int k = 0; k < NWS_WF; ++k) {
        const int f = base + k * NWS_BLOCK;
        const int lab = f < nf ? label[f] : -1;
        // a new label in any lane: the sums so far go out (the ballot is the wave's: every lane takes the same branch)
        if (__ballot(cur >= 0 && lab != cur) != 0ull) ws_flush(wacc, nc, q0, nq, cur, acc);
        cur = lab;
        if (lab < 0) continue;
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        const double x0 = pos[3 * i0], y0 = pos[3 * i0 + 1], z0 = pos[3 * i0 + 2];
        const double x1 = pos[3 * i1], y1 = pos[3 * i1 + 1], z1 = pos[3 * i1 + 2];
        const double x2 = pos[3 * i2], y2 = pos[3 * i2 + 1], z2 = pos[3 * i2 + 2];
#pragma unroll
        for (int j = 0; j < NWS_WQ; ++j) {
            if (q0 + j >= nq || !active[(i64)(q0 + j) * nc + lab]) continue;
            const double ax = x0 - qx[j], ay = y0 - qy[j], az = z0 - qz[j];
            const double bx = x1 - qx[j], by = y1 - qy[j], bz = z1 - qz[j];
            const double cx = x2 - qx[j], cy = y2 - qy[j], cz = z2 - qz[j];
            const double la = sqrt(ax * ax + ay * ay + az * az), lb = sqrt(bx * bx + by * by + bz * bz), lc = sqrt(cx * cx + cy * cy + cz * cz);
            const double det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
            const double den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (ax * cx + ay * cy + az * cz) * lb + (bx * cx + by * cy + bz * cz) * la;
            // Omega = 2 atan2(det, den), w = Omega / (4 pi)
            acc[j] += llrint(atan2(det, den) * (0.5 / M_PI) * scale);
        }
    }
    ws_flush(wacc, nc, q0, nq, cur, acc);
}

// ---- short edges -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NWS_BLOCK) void k_ws_lengths(const float *__restrict__ pos, const int *__restrict__ faces, int nh, float *__restrict__ len)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nh) return;
    const int f = h / 3, k = h - 3 * f;
    const int o = faces[h], d = faces[3 * f + (k == 2 ? 0 : k + 1)];
    const float e0 = pos[3 * d] - pos[3 * o], e1 = pos[3 * d + 1] - pos[3 * o + 1], e2 = pos[3 * d + 2] - pos[3 * o + 2];
    const float r0 = e0 * e0, r1 = e1 * e1, r2 = e2 * e2;       // (-ffp-contract=off: every product rounded, as numpy / nwr_mesh_geometry)
    len[h] = sqrtf((r0 + r1) + r2);
}

// radix select state: for the two targets (the (n-1)/2-th and n/2-th smallest), the bits fixed so far and the rank left within them
struct ws_sel {
    unsigned prefix[2];
    int k[2];
    float median, thr;
};

__global__ __launch_bounds__(NWS_BLOCK) void k_ws_hist(const float *__restrict__ len, int n, int shift, const ws_sel *__restrict__ sel, int *__restrict__ hist)
{
    __shared__ int s_h[2][256];
    s_h[0][threadIdx.x] = 0;
    s_h[1][threadIdx.x] = 0;
    __syncthreads();
    const unsigned hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    const unsigned p0 = sel->prefix[0], p1 = sel->prefix[1];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned b = __float_as_uint(len[i]);
        const int bin = (b >> shift) & 255;
        if ((b & hmask) == p0) atomicAdd(&s_h[0][bin], 1);
        if (p1 != p0 && (b & hmask) == p1) atomicAdd(&s_h[1][bin], 1);
    }
    __syncthreads();
    if (s_h[0][threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_h[0][threadIdx.x]);
    if (s_h[1][threadIdx.x]) atomicAdd(&hist[256 + threadIdx.x], s_h[1][threadIdx.x]);
}

// one wave: the bin that holds each target's rank, by a prefix sum over the 256 bins (4 per lane); the histograms are cleared for the
// next pass, and the last pass writes the median and the threshold
__global__ __launch_bounds__(64) void k_ws_pick(int *__restrict__ hist, int shift, int n, float threshold, ws_sel *__restrict__ sel)
{
    const int lane = threadIdx.x;
    const unsigned p0 = sel->prefix[0], p1 = sel->prefix[1];
    unsigned np[2];
    int nk[2];
    for (int t = 0; t < 2; ++t) {
        // (while both targets share their prefix, only the first histogram is filled: both read it)
        const int *h = hist + ((t == 1 && p1 != p0) ? 256 : 0);
        int v[4], s = 0;
        for (int j = 0; j < 4; ++j) { v[j] = h[4 * lane + j]; s += v[j]; }
        const int inc = nw_wave_incl_scan(s, lane);
        const int k = sel->k[t];
        int excl = inc - s, hit = -1, before = 0;
        for (int j = 0; j < 4; ++j) {
            if (hit < 0 && k >= excl && k < excl + v[j]) { hit = 4 * lane + j; before = excl; }
            excl += v[j];
        }
        const u64 m = __ballot(hit >= 0);
        const int src = m ? __ffsll((unsigned long long)m) - 1 : 0;
        const int bin = __shfl(hit, src, 64), bef = __shfl(before, src, 64);
        np[t] = (t == 0 ? p0 : p1) | ((unsigned)max(bin, 0) << shift);
        nk[t] = k - bef;
    }
    __syncthreads();
    for (int j = 0; j < 4; ++j) { hist[4 * lane + j] = 0; hist[256 + 4 * lane + j] = 0; }
    if (lane == 0) {
        sel->prefix[0] = np[0]; sel->prefix[1] = np[1];
        sel->k[0] = nk[0]; sel->k[1] = nk[1];
        if (shift == 0) {
            const float a = __uint_as_float(np[0]), b = __uint_as_float(np[1]);
            // numpy: the middle element, or mean() of the two middle ones in float32 (their sum, then divided by 2)
            const float med = (n & 1) ? a : (a + b) / 2.0f;
            sel->median = med;
            sel->thr = threshold * med;
        }
    }
}

__global__ __launch_bounds__(NWS_BLOCK) void k_ws_flag(const float *__restrict__ len, const int *__restrict__ faces, int nh, const ws_sel *__restrict__ sel,
                                                       unsigned char *__restrict__ flag)
{
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= nh) return;
    if (len[h] < sel->thr) {
        const int f = h / 3, k = h - 3 * f;
        flag[faces[3 * f + (k == 2 ? 0 : k + 1)]] = 1;       // (the head: every writer stores the same byte)
    }
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
using bq::DevBuf;
using bq::fail;
using bq::nblk;

struct nws_ctx : bq::Ctx {
    DevBuf pos, faces, twin, label, a, b, c, d, e, f;
};

namespace {

#define NWS_HIP(call) BQ_HIP(call, NWS_ERR_NOMEM, NWS_ERR_HIP)

#define NWS_TRY(call)                                                                                          \
    do {                                                                                                       \
        const int r_ = (call);                                                                                 \
        if (r_ != NWS_OK) return r_;                                                                           \
    } while (0)

int check_twin(const int32_t *twin, int64_t nf)
{
    if (!twin) return NWS_ERR_BADARG;
    for (int64_t i = 0; i < 3 * nf; ++i)
        if (twin[i] < -1 || twin[i] >= 3 * nf) return NWS_ERR_BADARG;
    return NWS_OK;
}

int check_label(const int32_t *label, int64_t nf, int32_t nc)
{
    if (!label || nc < 0) return NWS_ERR_BADARG;
    for (int64_t i = 0; i < nf; ++i)
        if (label[i] < -1 || label[i] >= nc) return NWS_ERR_BADARG;
    return NWS_OK;
}

// 2^k with n_terms * bound * 2^k <= 2^62: the fixed-point scale of a sum of n_terms terms of magnitude <= bound
double fixed_scale(double n_terms, double bound)
{
    bound = std::max(bound * std::max(n_terms, 1.0), 1e-300);
    return std::ldexp(1.0, (int)std::floor(62.0 - std::log2(bound)));
}

// the frame of pos: o = the centre of its bounding box rounded to float32, M = max |p - o|, and the fixed-point scales that follow from M
ws_frame make_frame(const float *pos, int64_t nv, int nf)
{
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int64_t i = 0; i < nv; ++i)
        for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], pos[3 * i + d]); hi[d] = std::max(hi[d], pos[3 * i + d]); }
    ws_frame fr;
    double M = 1e-30;
    for (int d = 0; d < 3; ++d) {
        fr.o[d] = nv > 0 ? (double)(float)(0.5 * ((double)lo[d] + (double)hi[d])) : 0.0;
        if (nv > 0) M = std::max(M, std::max((double)hi[d] - fr.o[d], fr.o[d] - (double)lo[d]));
    }
    fr.s_area = fixed_scale(nf, 6.0 * M * M);
    fr.s_vol = fixed_scale(nf, M * M * M);
    fr.s_nrm = fixed_scale(nf, 12.0 * M * M);
    return fr;
}

// the accumulators of k_ws_stats into the ctx's buffers c (u64: count, area, volume, border, C each, then the 3C normal sums) and d (bbox,
// 6C ordered ints); pos, faces, twin and label are on the device already
int run_stats(nws_ctx *ctx, int nf, int nc, const ws_frame &fr)
{
    NWS_HIP(ctx->c.ensure(sizeof(u64) * 7 * (size_t)nc));
    NWS_HIP(ctx->d.ensure(sizeof(int) * 6 * (size_t)nc));
    NWS_HIP(hipMemsetAsync(ctx->c.p, 0, sizeof(u64) * 7 * (size_t)nc, ctx->stream));
    hipLaunchKernelGGL(k_ws_bbox_init, dim3(nblk(6 * (int64_t)nc)), dim3(NWS_BLOCK), 0, ctx->stream, ctx->d.as<int>(), 6 * nc);
    ws_acc acc;
    u64 *base = ctx->c.as<u64>();
    acc.count = base; acc.area = base + nc; acc.vol = base + 2 * (size_t)nc; acc.border = base + 3 * (size_t)nc; acc.nrm = base + 4 * (size_t)nc;
    acc.bbox = ctx->d.as<int>();
    hipLaunchKernelGGL(k_ws_stats, dim3(nblk(nf)), dim3(NWS_BLOCK), 0, ctx->stream, ctx->pos.as<float>(), ctx->faces.as<int>(), ctx->twin.as<int>(),
                       ctx->label.as<int>(), nf, fr, acc);
    NWS_HIP(hipGetLastError());
    return NWS_OK;
}

}  // namespace

NWS_EXPORT int nws_abi_version(void) { return NWS_ABI_VERSION; }

NWS_EXPORT int nws_create(int device, nws_ctx **out) { return bq::create(device, out, NWS_ERR_BADARG, NWS_ERR_HIP); }

NWS_EXPORT void nws_destroy(nws_ctx *ctx) { bq::destroy(ctx); }

NWS_EXPORT const char *nws_last_error(nws_ctx *ctx) { return bq::last_error(ctx); }

NWS_EXPORT int nws_label_faces(nws_ctx *ctx, const int32_t *faces, const int32_t *twin, const uint8_t *mask, int64_t n_faces, int32_t *label_out,
                               int32_t *n_components_out)
{
    if (!faces || !label_out || !n_components_out || n_faces < 1 || n_faces > (1ll << 29)) return NWS_ERR_BADARG;
    NWS_TRY(check_twin(twin, n_faces));
    if (!ctx) return NWS_ERR_BADARG;
    NWS_HIP(hipSetDevice(ctx->device));
    const int nf = (int)n_faces;
    NWS_HIP(bq::upload(ctx->stream, ctx->twin, twin, 3 * n_faces));
    const unsigned char *dmask = nullptr;
    if (mask) {
        NWS_HIP(bq::upload(ctx->stream, ctx->a, mask, n_faces));
        dmask = ctx->a.as<unsigned char>();
    }
    NWS_HIP(ctx->b.ensure(sizeof(int) * (size_t)nf));            // parent
    NWS_HIP(ctx->c.ensure(sizeof(int) * (size_t)nf));            // is_root
    NWS_HIP(ctx->d.ensure(sizeof(int) * (size_t)(nf + 1)));      // rank (exclusive scan of is_root; d[nf] = the count)
    NWS_HIP(ctx->label.ensure(sizeof(int) * (size_t)nf));        // root, then label
    int *parent = ctx->b.as<int>(), *is_root = ctx->c.as<int>(), *rank = ctx->d.as<int>(), *label = ctx->label.as<int>();
    hipLaunchKernelGGL(k_ws_init, dim3(nblk(nf)), dim3(NWS_BLOCK), 0, ctx->stream, dmask, nf, parent);
    hipLaunchKernelGGL(k_ws_hook, dim3(nblk(nf)), dim3(NWS_BLOCK), 0, ctx->stream, ctx->twin.as<int>(), nf, parent);
    hipLaunchKernelGGL(k_ws_compress, dim3(nblk(nf)), dim3(NWS_BLOCK), 0, ctx->stream, nf, parent, label, is_root);
    NWS_HIP(hipGetLastError());
    int nc = 0;
    NWS_HIP(bq::scan_total(ctx->stream, is_root, nf, rank, ctx->e, &nc));
    hipLaunchKernelGGL(k_ws_number, dim3(nblk(nf)), dim3(NWS_BLOCK), 0, ctx->stream, nf, rank, label);
    NWS_HIP(hipGetLastError());
    NWS_HIP(hipMemcpyAsync(label_out, label, sizeof(int) * (size_t)nf, hipMemcpyDeviceToHost, ctx->stream));
    NWS_HIP(hipStreamSynchronize(ctx->stream));
    *n_components_out = nc;
    return NWS_OK;
}

NWS_EXPORT int nws_component_stats(nws_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, const int32_t *twin, const int32_t *label,
                                   int64_t n_faces, int32_t n_components, int64_t *face_count, double *area, double *volume, float *bbox,
                                   int64_t *n_border)
{
    if (n_components < 0 || n_components > (1 << 28)) return NWS_ERR_BADARG;
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return NWS_ERR_BADARG;
    NWS_TRY(check_twin(twin, n_faces));
    NWS_TRY(check_label(label, n_faces, n_components));
    if (!ctx) return NWS_ERR_BADARG;
    if (n_components == 0) return NWS_OK;
    NWS_HIP(hipSetDevice(ctx->device));
    const int nf = (int)n_faces, nc = n_components;
    NWS_HIP(bq::upload(ctx->stream, ctx->pos, pos, 3 * n_vertices));
    NWS_HIP(bq::upload(ctx->stream, ctx->faces, faces, 3 * n_faces));
    NWS_HIP(bq::upload(ctx->stream, ctx->twin, twin, 3 * n_faces));
    NWS_HIP(bq::upload(ctx->stream, ctx->label, label, n_faces));
    const ws_frame fr = make_frame(pos, n_vertices, nf);
    NWS_TRY(run_stats(ctx, nf, nc, fr));
    std::vector<u64> acc(7 * (size_t)nc);
    std::vector<int> bb(6 * (size_t)nc);
    NWS_HIP(hipMemcpyAsync(acc.data(), ctx->c.p, sizeof(u64) * acc.size(), hipMemcpyDeviceToHost, ctx->stream));
    NWS_HIP(hipMemcpyAsync(bb.data(), ctx->d.p, sizeof(int) * bb.size(), hipMemcpyDeviceToHost, ctx->stream));
    NWS_HIP(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < nc; ++c) {
        if (face_count) face_count[c] = (int64_t)acc[c];
        if (area) area[c] = (double)(int64_t)acc[nc + c] / fr.s_area;
        if (volume) {
            // about o, plus o . (sum of the face normals) / 6: the volume about the origin (the second part is ~0 for a closed component)
            const u64 *n = &acc[4 * (size_t)nc + 3 * (size_t)c];
            const double shift = (fr.o[0] * (double)(int64_t)n[0] + fr.o[1] * (double)(int64_t)n[1] + fr.o[2] * (double)(int64_t)n[2]) / fr.s_nrm;
            volume[c] = (double)(int64_t)acc[2 * (size_t)nc + c] / fr.s_vol + shift / 6.0;
        }
        if (n_border) n_border[c] = (int64_t)acc[3 * (size_t)nc + c];
        if (bbox)
            for (int d = 0; d < 6; ++d) {
                const int o = bb[6 * (size_t)c + d];
                bbox[6 * (size_t)c + d] = (o == INT_MAX) ? FLT_MAX : (o == INT_MIN) ? -FLT_MAX : bq::dec_ord(o);
            }
    }
    return NWS_OK;
}

NWS_EXPORT int nws_winding(nws_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, const int32_t *label, int64_t n_faces,
                           int32_t n_components, const float *queries, const int32_t *query_component, int64_t n_queries, double *w_out)
{
    if (!queries || !w_out || n_queries < 0 || n_queries > (1 << 24) || n_components < 0 || n_components > (1 << 24) ||
        n_queries * (int64_t)n_components > (1ll << 28))
        return NWS_ERR_BADARG;
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return NWS_ERR_BADARG;
    NWS_TRY(check_label(label, n_faces, n_components));
    if (!bq::all_finite(queries, 3 * n_queries)) return NWS_ERR_BADARG;
    if (query_component)
        for (int64_t i = 0; i < n_queries; ++i)
            if (query_component[i] < -1 || query_component[i] >= n_components) return NWS_ERR_BADARG;
    if (!ctx) return NWS_ERR_BADARG;
    const int64_t nw = n_queries * (int64_t)n_components;
    if (nw == 0) return NWS_OK;
    NWS_HIP(hipSetDevice(ctx->device));
    const int nf = (int)n_faces, nc = n_components, nq = (int)n_queries;
    NWS_HIP(bq::upload(ctx->stream, ctx->pos, pos, 3 * n_vertices));
    NWS_HIP(bq::upload(ctx->stream, ctx->faces, faces, 3 * n_faces));
    NWS_HIP(bq::upload(ctx->stream, ctx->label, label, n_faces));
    NWS_HIP(bq::upload(ctx->stream, ctx->a, queries, 3 * n_queries));
    const int *dqc = nullptr;
    if (query_component) {
        NWS_HIP(bq::upload(ctx->stream, ctx->b, query_component, n_queries));
        dqc = ctx->b.as<int>();
    }
    // the boxes: k_ws_stats over a twin table of -1 (the border counts it also makes are not read)
    NWS_HIP(ctx->twin.ensure(sizeof(int) * 3 * (size_t)nf));
    NWS_HIP(hipMemsetAsync(ctx->twin.p, 0xff, sizeof(int) * 3 * (size_t)nf, ctx->stream));
    NWS_TRY(run_stats(ctx, nf, nc, make_frame(pos, n_vertices, nf)));
    NWS_HIP(ctx->e.ensure((size_t)nw));
    NWS_HIP(ctx->f.ensure(sizeof(u64) * (size_t)nw));
    NWS_HIP(hipMemsetAsync(ctx->f.p, 0, sizeof(u64) * (size_t)nw, ctx->stream));
    hipLaunchKernelGGL(k_ws_active, dim3(nblk(nw)), dim3(NWS_BLOCK), 0, ctx->stream, ctx->a.as<float>(), dqc, nq, nc, ctx->d.as<int>(),
                       ctx->e.as<unsigned char>());
    const double scale = std::ldexp(1.0, 62 - (int)std::ceil(std::log2((double)nf + 1.0)));
    const dim3 grid((unsigned)((nf + NWS_BLOCK * NWS_WF - 1) / (NWS_BLOCK * NWS_WF)), (unsigned)((nq + NWS_WQ - 1) / NWS_WQ));
    hipLaunchKernelGGL(k_ws_winding, grid, dim3(NWS_BLOCK), 0, ctx->stream, ctx->pos.as<float>(), ctx->faces.as<int>(), ctx->label.as<int>(), nf, nc,
                       ctx->a.as<float>(), nq, ctx->e.as<unsigned char>(), scale, ctx->f.as<u64>());
    NWS_HIP(hipGetLastError());
    std::vector<u64> acc((size_t)nw);
    NWS_HIP(hipMemcpyAsync(acc.data(), ctx->f.p, sizeof(u64) * (size_t)nw, hipMemcpyDeviceToHost, ctx->stream));
    NWS_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < nw; ++i) w_out[i] = (double)(int64_t)acc[i] / scale;
    return NWS_OK;
}

NWS_EXPORT int nws_short_edge_vertices(nws_ctx *ctx, const float *pos, int64_t n_vertices, const int32_t *faces, int64_t n_faces, float threshold,
                                       uint8_t *flag_out, float *median_out)
{
    if (!flag_out || !(threshold >= 0.0f) || !std::isfinite(threshold)) return NWS_ERR_BADARG;
    if (!bq::mesh_ok(pos, n_vertices, faces, n_faces)) return NWS_ERR_BADARG;
    if (!ctx) return NWS_ERR_BADARG;
    NWS_HIP(hipSetDevice(ctx->device));
    const int nh = (int)(3 * n_faces);
    NWS_HIP(bq::upload(ctx->stream, ctx->pos, pos, 3 * n_vertices));
    NWS_HIP(bq::upload(ctx->stream, ctx->faces, faces, 3 * n_faces));
    NWS_HIP(ctx->a.ensure(sizeof(float) * (size_t)nh));          // lengths
    NWS_HIP(ctx->b.ensure(sizeof(int) * 512));                   // two histograms
    NWS_HIP(ctx->c.ensure(sizeof(ws_sel)));
    NWS_HIP(ctx->e.ensure((size_t)n_vertices));                  // flags
    ws_sel init{};
    init.k[0] = (nh - 1) / 2;
    init.k[1] = nh / 2;
    NWS_HIP(hipMemcpyAsync(ctx->c.p, &init, sizeof(ws_sel), hipMemcpyHostToDevice, ctx->stream));
    NWS_HIP(hipMemsetAsync(ctx->b.p, 0, sizeof(int) * 512, ctx->stream));
    NWS_HIP(hipMemsetAsync(ctx->e.p, 0, (size_t)n_vertices, ctx->stream));
    hipLaunchKernelGGL(k_ws_lengths, dim3(nblk(nh)), dim3(NWS_BLOCK), 0, ctx->stream, ctx->pos.as<float>(), ctx->faces.as<int>(), nh, ctx->a.as<float>());
    const int hist_blocks = std::min(nblk(nh), 1024);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_ws_hist, dim3(hist_blocks), dim3(NWS_BLOCK), 0, ctx->stream, ctx->a.as<float>(), nh, shift, ctx->c.as<ws_sel>(), ctx->b.as<int>());
        hipLaunchKernelGGL(k_ws_pick, dim3(1), dim3(64), 0, ctx->stream, ctx->b.as<int>(), shift, nh, threshold, ctx->c.as<ws_sel>());
    }
    hipLaunchKernelGGL(k_ws_flag, dim3(nblk(nh)), dim3(NWS_BLOCK), 0, ctx->stream, ctx->a.as<float>(), ctx->faces.as<int>(), nh, ctx->c.as<ws_sel>(),
                       ctx->e.as<unsigned char>());
    NWS_HIP(hipGetLastError());
    ws_sel out{};
    NWS_HIP(hipMemcpyAsync(&out, ctx->c.p, sizeof(ws_sel), hipMemcpyDeviceToHost, ctx->stream));
    NWS_HIP(hipMemcpyAsync(flag_out, ctx->e.p, (size_t)n_vertices, hipMemcpyDeviceToHost, ctx->stream));
    NWS_HIP(hipStreamSynchronize(ctx->stream));
    if (median_out) *median_out = out.median;
    return NWS_OK;
}
