// The rules of the balanced k-d work list of the nearest-face query, without HIP: which localizations share a wave.  The device driver
// (nw_partition.h, launched from resort_by_projection in nanowrap.hip) and the host restatement at the end of this file apply the same
// functions, so the two agree element for element; tests/test_partition_core_cpu.py compiles the restatement for the CPU with g++.
// Without a HIP compiler NWP_HD is plain `inline`.
//
// The list is cut from the localizations in the order of their foot-point Morton keys (k_projection_keys):
//   * start segments = the aligned Morton blocks of that key at the coarsest level at which no block holds more than `cap` localizations
//     (start_level); a block that is larger even at level 0 is cut into runs of chunk_len() localizations;
//   * a segment of n > leaf localizations is cut on the coordinate with the widest extent -- foot x, y, z or w x signed height, ties to
//     the lowest axis -- quantised to 16 bits inside the segment's own box: the cut_rank(n) localizations that come first by (key,
//     position) go left.  A segment of at most sort_max localizations is sorted by (key, position) on the way; a larger one is only
//     parted, and both parts keep their order (a selection and a scan instead of a sort: what the device can afford for thousands of
//     localizations).  The left part is a whole number of leaves, so every leaf of a start segment but its last is exactly full and
//     the leaves are the runs of `leaf` positions counted from the segment's start;
//   * at the end every leaf is ordered by (nearest face id, position), so lanes that share a face stay adjacent.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define NWP_HD __host__ __device__ __forceinline__
#else
#define NWP_HD inline
#endif

namespace nwp {

enum { AXES = 4, LEVELS = 11, MAX_DEPTH = 32, SORT_MAX = 1024 };

// a coordinate as the rules see it: non-finite -> 0, and -0 -> +0 (so that the box of a segment does not depend on who reduced it)
NWP_HD float clean(float v) { return (v - v == 0.0f) ? v + 0.0f : 0.0f; }

// floats as unsigned integers of the same order (the device reduces a segment's box with integer min / max)
NWP_HD uint32_t enc(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
NWP_HD float dec(uint32_t e)
{
    const uint32_t b = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// the four coordinates of a localization: its foot point and w x its signed height over the nearest face
NWP_HD void coords(float fx, float fy, float fz, float height, float w, float c[AXES])
{
    c[0] = clean(fx); c[1] = clean(fy); c[2] = clean(fz); c[3] = clean(w * clean(height));
}

// how many localizations of a segment of n go left
NWP_HD int cut_rank(int n, int leaf) { return ((n + leaf - 1) / leaf / 2) * leaf; }

// the segment {first position, length} that holds position j after `depth` cuts of a start segment of n localizations
struct Seg { int s0, n; };
NWP_HD Seg seg_at(int n, int leaf, int depth, int j)
{
    Seg s;
    s.s0 = 0; s.n = n;
    for (int d = 0; d < depth && s.n > leaf; ++d) {
        const int nl = cut_rank(s.n, leaf);
        if (j < s.s0 + nl) s.n = nl;
        else { s.s0 += nl; s.n -= nl; }
    }
    return s;
}

// the axis a segment is cut on: the widest of its box, ties to the lowest
NWP_HD int widest_axis(const float lo[AXES], const float hi[AXES])
{
    int best = 0;
    float e = hi[0] - lo[0];
    for (int a = 1; a < AXES; ++a) {
        const float ea = hi[a] - lo[a];
        if (ea > e) { e = ea; best = a; }
    }
    return best;
}

// 16-bit key of v inside [lo, hi]; a box without extent gives 0 for everyone.  (One subtraction, one division per box, one product:
// nothing a compiler could contract, so host and device round alike.)
NWP_HD uint32_t quantise(float v, float lo, float hi)
{
    const float ext = hi - lo;
    if (!(ext > 0.0f)) return 0u;
    const float scale = 65535.0f / ext;
    if (!(scale - scale == 0.0f)) return 0u;                 // a denormal extent
    const float x = (v - lo) * scale;
    if (!(x < 65535.0f)) return 65535u;
    return x > 0.0f ? (uint32_t)x : 0u;
}

// order inside a leaf: by nearest face id, then by position
NWP_HD bool face_before(int fa, int ja, int fb, int jb) { return fa < fb || (fa == fb && ja < jb); }

// the Morton level (block = key >> 3 level; level 10 is the whole cloud) of the start segments: the coarsest whose largest block fits
NWP_HD int start_level(const int max_block[LEVELS], int cap)
{
    for (int l = LEVELS - 1; l > 0; --l)
        if (max_block[l] <= cap) return l;
    return 0;
}

// a block of m > cap localizations is cut into runs of this many (a whole number of leaves, at most cap; cap is a multiple of leaf)
NWP_HD int chunk_len(int m, int cap, int leaf)
{
    const int k = (m + cap - 1) / cap;
    const int per = (m + k - 1) / k;
    return (per + leaf - 1) / leaf * leaf;
}
// ... and how many start segments a block of m localizations makes
NWP_HD int chunk_count(int m, int cap, int leaf)
{
    if (m <= cap) return 1;
    const int per = chunk_len(m, cap, leaf);
    return (m + per - 1) / per;
}

}  // namespace nwp

// ---- the whole partition on the host, plainly ---------------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>

namespace nwp {

struct HostResult {
    std::vector<int> order;          // new position -> position in the order the partition was given
    std::vector<int> seg_start;      // start segments: first positions, and n at the end
    std::vector<int> leaf_start;     // leaves in list order: first positions, and n at the end
    int level = 0;
};

// key: the foot-point Morton keys, ascending (30 bits); foot: (x, y, z, signed height) per localization; face: nearest face ids
inline HostResult partition_host(int n, const uint32_t *key, const float *foot, const int *face, int leaf, int cap, float w, int sort_max = SORT_MAX)
{
    HostResult r;
    int max_block[LEVELS];
    for (int l = 0; l < LEVELS; ++l) {
        max_block[l] = 0;
        for (int i = 0, b0 = 0; i <= n; ++i)
            if (i == n || (i > 0 && (key[i] >> (3 * l)) != (key[i - 1] >> (3 * l)))) { max_block[l] = std::max(max_block[l], i - b0); b0 = i; }
    }
    r.level = start_level(max_block, cap);
    const int shift = 3 * r.level;
    for (int i = 0, b0 = 0; i <= n; ++i)
        if (i == n || (i > 0 && (key[i] >> shift) != (key[i - 1] >> shift))) {
            const int m = i - b0, per = m > cap ? chunk_len(m, cap, leaf) : m;
            for (int p = b0; p < i; p += per) r.seg_start.push_back(p);
            b0 = i;
        }
    r.seg_start.push_back(n);
    r.order.resize((size_t)n);
    for (int i = 0; i < n; ++i) r.order[(size_t)i] = i;
    std::vector<uint32_t> k16((size_t)n);
    for (size_t s = 0; s + 1 < r.seg_start.size(); ++s) {
        const int p0 = r.seg_start[s], m = r.seg_start[s + 1] - p0;
        int *ord = r.order.data() + p0;                                  // (entries are positions of the given order)
        bool more = true;
        for (int depth = 0; more && depth < MAX_DEPTH; ++depth) {
            more = false;
            for (int j = 0; j < m;) {
                const Seg sg = seg_at(m, leaf, depth, j);
                j = sg.s0 + sg.n;
                if (sg.n <= leaf) continue;
                more = true;
                uint32_t lo[AXES], hi[AXES];
                for (int a = 0; a < AXES; ++a) { lo[a] = 0xffffffffu; hi[a] = 0u; }
                float c[AXES];
                for (int t = sg.s0; t < sg.s0 + sg.n; ++t) {
                    const float *f = foot + 4 * (size_t)ord[t];
                    coords(f[0], f[1], f[2], f[3], w, c);
                    for (int a = 0; a < AXES; ++a) { lo[a] = std::min(lo[a], enc(c[a])); hi[a] = std::max(hi[a], enc(c[a])); }
                }
                float flo[AXES], fhi[AXES];
                for (int a = 0; a < AXES; ++a) { flo[a] = dec(lo[a]); fhi[a] = dec(hi[a]); }
                const int axis = widest_axis(flo, fhi);
                for (int t = sg.s0; t < sg.s0 + sg.n; ++t) {
                    const float *f = foot + 4 * (size_t)ord[t];
                    coords(f[0], f[1], f[2], f[3], w, c);
                    k16[(size_t)ord[t]] = quantise(c[axis], flo[axis], fhi[axis]);
                }
                int *b = ord + sg.s0, *e = b + sg.n;
                if (sg.n <= sort_max) {
                    std::stable_sort(b, e, [&](int x, int y) { return k16[(size_t)x] < k16[(size_t)y]; });
                } else {
                    // the first cut_rank by (key, position) go left; both parts keep their order
                    std::vector<int> by_key(b, e);
                    std::stable_sort(by_key.begin(), by_key.end(), [&](int x, int y) { return k16[(size_t)x] < k16[(size_t)y]; });
                    const int nl = cut_rank(sg.n, leaf);
                    std::vector<char> left((size_t)n, 0);
                    for (int t = 0; t < nl; ++t) left[(size_t)by_key[(size_t)t]] = 1;
                    std::stable_partition(b, e, [&](int x) { return left[(size_t)x] != 0; });
                }
            }
        }
        for (int j = 0; j < m; j += leaf) {
            const int len = std::min(leaf, m - j);
            r.leaf_start.push_back(p0 + j);
            std::stable_sort(ord + j, ord + j + len, [&](int x, int y) { return face[x] < face[y]; });
        }
    }
    r.leaf_start.push_back(n);
    return r;
}

}  // namespace nwp
#endif
