// Device side of the balanced k-d work list (the rules and their host restatement: nw_partition_core.h).  Runs once per cloud, from
// resort_by_projection: one workgroup per start segment does every level of its segment in LDS.  A level sorts each of its segments by
// counting -- rank = how many composites (16-bit key, position) of the segment are smaller -- which is quadratic in the segment,
// stable by construction and needs neither scans nor atomics on the data path; the lanes of a wave read the same composite at a time
// (an LDS broadcast).  Quadratic is affordable up to nwp::SORT_MAX localizations; the few larger segments of the first levels are
// parted instead, one after the other by the whole workgroup: a radix select of the cut key (two histograms of a byte) and a scan.
#pragma once
#include "nw_partition_core.h"

#define NWP_CAP 16384                // localizations of a start segment: what 144 KB of LDS hold (positions fit a composite's 16 bits)
#define NWP_MIN_LEAF 32              // the box table below has NWP_CAP / NWP_MIN_LEAF rows
#define NWP_THREADS 1024             // one workgroup per CU (its LDS): sixteen waves to count with

// largest aligned Morton block of the sorted key list at every level: max_block[l] (zeroed by the caller)
__global__ void k_kd_block_max(const unsigned *__restrict__ key, int N, int *__restrict__ max_block)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned k = key[i];
    for (int l = 0; l < nwp::LEVELS; ++l) {
        const int shift = 3 * l;
        if (i > 0 && (key[i - 1] >> shift) == (k >> shift)) break;         // not a head here, nor at any coarser level
        int lo = i + 1, hi = N;                                             // first position past the block
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((key[mid] >> shift) == (k >> shift)) lo = mid + 1; else hi = mid;
        }
        if (lo - i > __atomic_load_n(&max_block[l], __ATOMIC_RELAXED)) atomicMax(&max_block[l], lo - i);      // (few blocks get past the look)
    }
}

// start segments of the Morton blocks [bstart[b], bstart[b + 1]): how many, and where
__global__ void k_kd_seg_counts(const int *__restrict__ bstart, int nblocks, int cap, int leaf, int *__restrict__ nsegs)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    nsegs[b] = nwp::chunk_count(bstart[b + 1] - bstart[b], cap, leaf);
}

__global__ void k_kd_fill_segs(const int *__restrict__ bstart, const int *__restrict__ sstart, int nblocks, int cap, int leaf, NwItem *__restrict__ segs)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    const int p0 = bstart[b], p1 = bstart[b + 1], m = p1 - p0;
    if (m <= 0) return;
    const int per = m > cap ? nwp::chunk_len(m, cap, leaf) : m;
    int o = sstart[b];
    for (int p = p0; p < p1; p += per) {
        NwItem s;
        s.p0 = p; s.n = min(per, p1 - p);
        segs[o++] = s;
    }
}

// the leaves of every start segment: runs of `leaf` positions from its start (nw_partition_core.h: cut_rank)
__global__ void k_kd_leaf_counts(const NwItem *__restrict__ segs, int nsegs, int leaf, int *__restrict__ nleaves)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsegs) return;
    nleaves[s] = (segs[s].n + leaf - 1) / leaf;
}

__global__ void k_kd_fill_leaves(const NwItem *__restrict__ segs, const int *__restrict__ lstart, int nsegs, int leaf, NwItem *__restrict__ leaves)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsegs) return;
    const NwItem sg = segs[s];
    int o = lstart[s];
    for (int p = 0; p < sg.n; p += leaf) {
        NwItem w;
        w.p0 = sg.p0 + p; w.n = min(leaf, sg.n - p);
        leaves[o++] = w;
    }
}

// how many of comp[s0, s0 + n) are smaller than `me` (s0 is a multiple of 4: segments start on leaf boundaries)
__device__ __forceinline__ int nwkd_rank_u32(const unsigned *comp, int s0, int n, unsigned me)
{
    const uint4 *c4 = reinterpret_cast<const uint4 *>(comp + s0);
    int rank = 0;
    const int q = n >> 2;
    for (int t = 0; t < q; ++t) {
        const uint4 v = c4[t];
        rank += (v.x < me ? 1 : 0) + (v.y < me ? 1 : 0) + (v.z < me ? 1 : 0) + (v.w < me ? 1 : 0);
    }
    for (int t = s0 + 4 * q; t < s0 + n; ++t) rank += comp[t] < me ? 1 : 0;
    return rank;
}

// The workgroup parts idx_in[s0, s0 + n) at rank nl into idx_out: the nl first by (key, position) go left, both parts keep their order.
// keys[s0, s0 + n) holds the 16-bit keys; hist (256), wsum (2 x 16) and pick (4) are scratch.  Ends with a barrier.
__device__ __forceinline__ void nwkd_part_segment(const unsigned short *idx_in, unsigned short *idx_out, const unsigned *keys, int s0, int n, int nl,
                                                 unsigned *hist, int *wsum, int *pick)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // radix select of the key of rank nl - 1 (0-based), a byte at a time from the top
    int below = 0;                       // keys known to be smaller than the prefix so far
    unsigned prefix = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = pass == 0 ? 8 : 0;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int j = s0 + tid; j < s0 + n; j += NWP_THREADS) {
            const unsigned k = keys[j];
            if (pass == 0 || (k >> 8) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int acc = below, b = 0;
            while (b < 255 && acc + (int)hist[b] < nl) { acc += (int)hist[b]; ++b; }
            pick[0] = b; pick[1] = acc;
        }
        __syncthreads();
        prefix = (prefix << 8) | (unsigned)pick[0];
        below = pick[1];
        __syncthreads();
    }
    const unsigned K = prefix;           // the cut key: `below` keys are smaller, and the first nl - below of the equal ones go left too
    const int take = nl - below;
    // every thread owns a run of positions; counts of smaller and of equal keys before each run
    const int per = (n + NWP_THREADS - 1) / NWP_THREADS;
    const int j0 = min(s0 + tid * per, s0 + n), j1 = min(j0 + per, s0 + n);
    int lt = 0, eq = 0;
    for (int j = j0; j < j1; ++j) { const unsigned k = keys[j]; lt += k < K ? 1 : 0; eq += k == K ? 1 : 0; }
    const int lt_in = nw_wave_incl_scan(lt, lane), eq_in = nw_wave_incl_scan(eq, lane);
    if (lane == 63) { wsum[wave] = lt_in; wsum[16 + wave] = eq_in; }
    __syncthreads();
    int lt_before = lt_in - lt, eq_before = eq_in - eq;
    for (int v = 0; v < wave; ++v) { lt_before += wsum[v]; eq_before += wsum[16 + v]; }
    int left_before = lt_before + min(eq_before, take);
    for (int j = j0; j < j1; ++j) {
        const unsigned k = keys[j];
        const bool left = k < K || (k == K && eq_before < take);
        eq_before += k == K ? 1 : 0;
        const int to = left ? s0 + left_before : s0 + nl + (j - s0 - left_before);
        left_before += left ? 1 : 0;
        idx_out[to] = idx_in[j];
    }
    __syncthreads();
}

// One workgroup per start segment.  order_in: position of the key-sorted list -> slot of the current layout; foot (x, y, z, signed
// height) and face are indexed by that slot.  order_out: the same list with every start segment partitioned.
__global__ __launch_bounds__(NWP_THREADS) void k_kd_partition(const NwItem *__restrict__ segs, int nsegs, const int *__restrict__ order_in,
                                                              const float4 *__restrict__ foot, const int *__restrict__ face, int leaf, float w,
                                                              int *__restrict__ order_out)
{
    __shared__ unsigned short idx[2][NWP_CAP];                   // position -> position at the start, before and after a level
    __shared__ __attribute__((aligned(16))) unsigned comp[NWP_CAP];
    __shared__ unsigned box[NWP_CAP / NWP_MIN_LEAF][2 * nwp::AXES];      // per segment of a level (row = first position / leaf): min, max
    __shared__ unsigned hist[256];
    __shared__ int wsum[2 * (NWP_THREADS / 64)], pick[4];
    if ((int)blockIdx.x >= nsegs) return;
    const NwItem sg = segs[blockIdx.x];
    const int n = sg.n, p0 = sg.p0, tid = (int)threadIdx.x;
    if (n > NWP_CAP || leaf < NWP_MIN_LEAF) {                    // (the host never asks for it) leave the order as it is
        for (int j = tid; j < n; j += NWP_THREADS) order_out[p0 + j] = order_in[p0 + j];
        return;
    }
    for (int j = tid; j < n; j += NWP_THREADS) idx[0][j] = (unsigned short)j;
    int cur = 0;
    for (int depth = 0; depth < nwp::MAX_DEPTH; ++depth) {
        int any = 0;
        for (int j = tid; j < n; j += NWP_THREADS) any |= nwp::seg_at(n, leaf, depth, j).n > leaf ? 1 : 0;
        for (int k = tid; k < (NWP_CAP / NWP_MIN_LEAF) * 2 * nwp::AXES; k += NWP_THREADS)
            box[k / (2 * nwp::AXES)][k % (2 * nwp::AXES)] = (k % (2 * nwp::AXES)) < nwp::AXES ? 0xffffffffu : 0u;
        if (!__syncthreads_or(any)) break;                       // (also orders idx[cur] and the cleared boxes before their use)
        // the boxes of this level's segments
        for (int j = tid; j < n; j += NWP_THREADS) {
            const nwp::Seg s = nwp::seg_at(n, leaf, depth, j);
            if (s.n <= leaf) continue;
            const float4 f = foot[order_in[p0 + idx[cur][j]]];
            float c[nwp::AXES];
            nwp::coords(f.x, f.y, f.z, f.w, w, c);
            unsigned *b = box[s.s0 / leaf];
            for (int a = 0; a < nwp::AXES; ++a) {
                const unsigned e = nwp::enc(c[a]);
                atomicMin(&b[a], e);
                atomicMax(&b[nwp::AXES + a], e);
            }
        }
        __syncthreads();
        // composites: (key on the segment's widest axis, position)
        for (int j = tid; j < n; j += NWP_THREADS) {
            const nwp::Seg s = nwp::seg_at(n, leaf, depth, j);
            if (s.n <= leaf) continue;
            const unsigned *b = box[s.s0 / leaf];
            float lo[nwp::AXES], hi[nwp::AXES];
            for (int a = 0; a < nwp::AXES; ++a) { lo[a] = nwp::dec(b[a]); hi[a] = nwp::dec(b[nwp::AXES + a]); }
            const int axis = nwp::widest_axis(lo, hi);
            const float4 f = foot[order_in[p0 + idx[cur][j]]];
            float c[nwp::AXES];
            nwp::coords(f.x, f.y, f.z, f.w, w, c);
            const float v = axis == 0 ? c[0] : axis == 1 ? c[1] : axis == 2 ? c[2] : c[3];
            const float vlo = axis == 0 ? lo[0] : axis == 1 ? lo[1] : axis == 2 ? lo[2] : lo[3];
            const float vhi = axis == 0 ? hi[0] : axis == 1 ? hi[1] : axis == 2 ? hi[2] : hi[3];
            const unsigned key = nwp::quantise(v, vlo, vhi);
            comp[j] = s.n > nwp::SORT_MAX ? key : (key << 16) | (unsigned)j;
        }
        __syncthreads();
        // the large segments, one after the other: parted
        for (int j = 0; j < n;) {
            const nwp::Seg s = nwp::seg_at(n, leaf, depth, j);
            j = s.s0 + s.n;
            if (s.n > nwp::SORT_MAX) nwkd_part_segment(idx[cur], idx[cur ^ 1], comp, s.s0, s.n, nwp::cut_rank(s.n, leaf), hist, wsum, pick);
        }
        // every segment sorted by counting
        for (int j = tid; j < n; j += NWP_THREADS) {
            const nwp::Seg s = nwp::seg_at(n, leaf, depth, j);
            if (s.n > nwp::SORT_MAX) continue;
            const int to = s.n > leaf ? s.s0 + nwkd_rank_u32(comp, s.s0, s.n, comp[j]) : j;
            idx[cur ^ 1][to] = idx[cur][j];
        }
        cur ^= 1;
        __syncthreads();
    }
    // every leaf by (nearest face, position)
    for (int j = tid; j < n; j += NWP_THREADS) comp[j] = (unsigned)face[order_in[p0 + idx[cur][j]]];
    __syncthreads();
    for (int j = tid; j < n; j += NWP_THREADS) {
        const int l0 = j / leaf * leaf, l1 = min(l0 + leaf, n);
        const int fj = (int)comp[j];
        int rank = 0;
        for (int t = l0; t < l1; ++t) rank += nwp::face_before((int)comp[t], t, fj, j) ? 1 : 0;
        order_out[p0 + l0 + rank] = order_in[p0 + idx[cur][j]];
    }
}
