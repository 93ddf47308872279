// The definition of the geodesic graph distance on a mesh (include/nw_geodesic.h), shared by the kernels of nw_geodesic.hip and by
// whoever compiles this header for the CPU (tests/test_geodesic_core_cpu.py builds a shim from it with g++ -ffp-contract=off):
//   - the weight of a mesh edge and of a face diagonal (one level of unfolding about an interior edge), and when a diagonal exists;
//   - which half-edge of a pair computes the diagonal and which lane relaxes which arc;
//   - one relaxation and one label step, with the argument why any schedule of them ends in the same numbers.
// PYME is not in the reference tree and upstream has no such module: this definition is the project's own.
// The squared distance is nw_neighbours_core.h's: included, not copied.  All arithmetic is float64 on the float32 positions.  Nothing
// may be contracted into an fma: compile with -ffp-contract=off.  No HIP header is needed: without a HIP compiler NWK_HD is plain `inline`.
//
// WHAT THIS IS NOT.  D is a distance in a graph: the mesh's edges plus, across every interior edge, the straight segment between the two
// opposite corners where that segment stays inside the two unfolded faces.  Every arc is a real path on the surface, so D is the length of
// a real path: never below the Euclidean distance, and an UPPER BOUND of the polyhedral geodesic, not the geodesic itself (no MMP, no
// heat method).  tests/test_mesh_geodesic_ref.py measures the overestimate on a sphere.
#pragma once
#include "nw_neighbours_core.h"

#define NWT_MAX_N (1ll << 30)       // vertices, sources
#define NWT_MAX_FACES (1ll << 29)   // 3 * faces half-edges are indexed by an int
// How many rounds are launched before the host reads their changed words, and how often a workgroup sweeps its own half-edges again
// within a round while one of its atomics lowered a value.  Both are first choices that nobody has measured: profiles/geodesic.txt is to
// record any sweep of them.  No output depends on either.
#define NWT_BATCH 16
#define NWT_SWEEPS 4
#define NWT_LABEL_NONE 0x7fffffff   // a label before any source reached it

// half-edge h = 3 f + k runs from faces[f][k] to faces[f][(k + 1) % 3]; the corner opposite to it is faces[f][(k + 2) % 3]
NWK_HD long long nwt_next(long long h) { return h - h % 3 + (h + 1) % 3; }
NWK_HD long long nwt_prev(long long h) { return h - h % 3 + (h + 2) % 3; }

// The weight of the edge {u, v}: sqrt((dx dx + dy dy) + dz dz).  nwk_dist2 is bit-symmetric in its two points (the differences are each
// other's negations, exactly), so both half-edges of an edge, and both directions of the arc, carry one double.  A zero-length edge
// weighs +0.0.
NWK_HD double nwt_edge_weight(const float *pu, const float *pv)
{
    return sqrt(nwk_dist2(pu[0], pu[1], pu[2], (double)pv[0], (double)pv[1], (double)pv[2]));
}

// x = ((p - a) . e) / L and y = sqrt(|(p - a) x e|^2) / L: the corner p in the plane of its face, the edge a -> b along the x axis
NWK_HD void nwt_unfold(const float *a, double ex, double ey, double ez, double L, const float *p, double *x, double *y)
{
    const double px = (double)p[0] - (double)a[0], py = (double)p[1] - (double)a[1], pz = (double)p[2] - (double)a[2];
    const double cx = py * ez - pz * ey, cy = pz * ex - px * ez, cz = px * ey - py * ex;
    *x = ((px * ex + py * ey) + pz * ez) / L;
    *y = sqrt((cx * cx + cy * cy) + cz * cz) / L;
}

// The weight of the diagonal c -> d across the interior edge {a, b}, or +inf if there is none.  The caller passes the canonical
// orientation: a is the end with the smaller vertex id, c the corner of the face whose half-edge runs a -> b, d the other face's corner.
// The two faces are unfolded about the edge into one plane, c above the axis and d below it.  The segment c -> d crosses the axis at
// x* = x_c + (x_d - x_c) y_c / (y_c + y_d); it lies inside the two triangles iff both faces have a height (y_c > 0, y_d > 0: a flat face
// has no inside) and 0 < x* < L STRICTLY (at an end of the edge the segment runs through a vertex, and the two edges there are no longer).
NWK_HD double nwt_diagonal_weight(const float *a, const float *b, const float *c, const float *d)
{
    const double ex = (double)b[0] - (double)a[0], ey = (double)b[1] - (double)a[1], ez = (double)b[2] - (double)a[2];
    const double L = sqrt((ex * ex + ey * ey) + ez * ez);
    if (!(L > 0.0)) return INFINITY;
    double xc, yc, xd, yd;
    nwt_unfold(a, ex, ey, ez, L, c, &xc, &yc);
    nwt_unfold(a, ex, ey, ez, L, d, &xd, &yd);
    if (!(yc > 0.0) || !(yd > 0.0)) return INFINITY;
    const double dx = xd - xc, sy = yc + yd;
    const double xs = xc + dx * yc / sy;
    if (!(xs > 0.0 && xs < L)) return INFINITY;
    return sqrt(dx * dx + sy * sy);
}

// Of the two half-edges h and t = twin[h] of an interior edge, the one that runs from the smaller vertex id to the larger computes the
// diagonal, once, and both ends read that double.  (A face that names a vertex twice has u == v on an edge: L = 0, no diagonal; the
// smaller half-edge index then owns it, so that exactly one does.)
NWK_HD bool nwt_owner(int u, int v, long long h, long long t) { return u < v || (u == v && h < t); }

// What k_gd_weights stores for half-edge h.  twin = nullptr: the plain edge graph.
//   we      the edge's weight (every half-edge)
//   wd      the diagonal's weight or +inf; written by the owner into its own slot and into twin[h]'s (wd_valid)
//   other   which arc the lane of h relaxes in a round: < 0 -- the edge (u, v, we); >= 0 -- the diagonal (own corner, other, wd).  A
//           border half-edge and every half-edge of a mesh without a twin table relax their edge (NWT_EDGE_ALONE: the edge has no second
//           lane; without a twin table an interior edge is then relaxed by both its half-edges, which changes nothing); of an interior
//           pair the owner relaxes the edge (NWT_EDGE_OWNER) and the other one the diagonal, so every lane has one arc
#define NWT_EDGE_ALONE (-1)
#define NWT_EDGE_OWNER (-2)
struct nwt_halfedge {
    double we, wd;
    int other;
    bool wd_valid;
};

NWK_HD nwt_halfedge nwt_halfedge_setup(const float *pos, const int *faces, const int *twin, long long h)
{
    nwt_halfedge r;
    const int u = faces[h], v = faces[nwt_next(h)];
    r.we = nwt_edge_weight(pos + 3 * (long long)u, pos + 3 * (long long)v);
    r.wd = INFINITY;
    r.wd_valid = false;
    r.other = NWT_EDGE_ALONE;
    const long long t = twin ? (long long)twin[h] : -1;
    if (t < 0) return r;
    if (nwt_owner(u, v, h, t)) {
        const int c = faces[nwt_prev(h)], d = faces[nwt_prev(t)];
        r.wd = nwt_diagonal_weight(pos + 3 * (long long)u, pos + 3 * (long long)v, pos + 3 * (long long)c, pos + 3 * (long long)d);
        r.wd_valid = true;
        r.other = NWT_EDGE_OWNER;
    } else {
        r.other = faces[nwt_prev(t)];
    }
    return r;
}

// The arc (p, q, w) the lane of half-edge h relaxes, in both directions; false: none (a diagonal that does not exist or is not asked for)
NWK_HD bool nwt_lane_arc(const int *faces, const int *other, const double *we, const double *wd, long long h, bool diagonals, int *p, int *q, double *w)
{
    const int o = other[h];
    if (o < 0) {
        *p = faces[h]; *q = faces[nwt_next(h)]; *w = we[h];
        return true;
    }
    *p = faces[nwt_prev(h)]; *q = o; *w = wd[h];
    return diagonals && *w < INFINITY;
}

// ---- the distance ------------------------------------------------------------------------------------------------------------------------
// D is what is left when, starting from D = +inf everywhere ("nothing known"), these two rules are applied until neither changes a value:
//     D[v] <- min(D[v], d0 of a source at v)                                          (seed)
//     D[v] <- min(D[v], fl(D[u] + w))  for an arc u -> v with D[u] <= d_cap           (relax)
// In the order of information -- +inf at the bottom -- this is the least fixed point of
//     D[v] = min(d0 of v's own sources, fl(D[u] + w) over arcs u -> v with D[u] <= d_cap).
//
// Proof that the result does not depend on the schedule, and is Dijkstra's.  Let W(v) be the minimum, over all walks
// s = v_0 -> v_1 -> ... -> v_k = v from a source, of the value x_k with x_0 = d0(s), x_{i+1} = fl(x_i + w_i), the walk being allowed
// only while x_i <= d_cap (k = 0 included).  (1) Every value a schedule ever stores in D[v] is +inf or such an x_k, by induction over the
// stores: a seed stores an x_0, a relaxation stores fl(D[u] + w) with D[u] an allowed x_i.  So D[v] >= W(v) at all times.  (2) g(x) =
// fl(x + w) with w >= +0.0 is monotone (rounding is) and g(x) >= x (x + w >= x exactly, and x is a double).  Take a walk that attains
// W(v).  When nothing changes any more, D[v_0] <= x_0, and D[v_i] <= x_i <= d_cap gives D[v_{i+1}] <= g(D[v_i]) <= g(x_i) = x_{i+1}: so
// D[v] <= W(v).  Together D = W whatever the order was, and a round of all arcs that lowers nothing is the end.  (3) Because g(x) >= x
// a cycle never lowers a value, so the minimum is attained by a simple walk of at most V - 1 arcs: a round that relaxes every arc whose
// tail changed in the round before makes the vertices of walk length <= k final after k rounds, and round V at the latest lowers
// nothing.  (4) Dijkstra's algorithm with the same rounded additions settles vertices in ascending x and computes the same minimum,
// again because g is monotone and never below its argument.  Values are >= +0.0 or +inf, never nan (-0.0 is not let in), so the unsigned
// 64-bit pattern of a value orders as the value does: the device's minimum is an integer atomic.
//
//
// A source's start value: d0 with -0.0 turned into +0.0 (its bit pattern would be the largest of all)
NWK_HD double nwt_start_value(double d0) { return d0 + 0.0; }

// One direction of one arc: whether it lowers D[v], and to what.
NWK_HD bool nwt_relax(double Du, double w, double d_cap, double Dv, double *cand)
{
    *cand = Du + w;
    return Du <= d_cap && *cand < Dv;
}

// ---- the label ---------------------------------------------------------------------------------------------------------------------------
// S is what is left when, starting from S = NWT_LABEL_NONE everywhere, these rules are applied on the final D until neither changes a value:
//     S[v] <- min(S[v], i)     for source i at v with d0_i == D[v]
//     S[v] <- min(S[v], S[u])  for an arc u -> v that is tight: D[u] <= d_cap and fl(D[u] + w) == D[v]
// i.e. the smallest index of a source from which a walk of tight arcs leads to v.  min over integers commutes, so the order is free.
// This is defined by the rule and not by "the source of some shortest walk": with rounded sums a walk can be shortest without each of
// its arcs being tight as seen from the final D (two different prefixes can round to one value), and the rule is what is computed.
NWK_HD bool nwt_tight(double Du, double w, double d_cap, double Dv) { return Du <= d_cap && Du + w == Dv && Dv < INFINITY; }

// ---- arguments ---------------------------------------------------------------------------------------------------------------------------
// sources: 1 <= n <= 2^30 ids in [0, n_vertices) (n_vertices < 0: only the sign is checked), d0 finite and >= 0 (or no d0: all zeros)
NWK_HD bool nwt_sources_ok(const int *ids, const double *d0, long long n, long long n_vertices)
{
    if (!ids || n < 1 || n > NWT_MAX_N) return false;
    for (long long i = 0; i < n; ++i) {
        if (ids[i] < 0 || (n_vertices >= 0 && ids[i] >= n_vertices)) return false;
        if (d0 && !(d0[i] >= 0.0 && d0[i] < INFINITY)) return false;
    }
    return true;
}

// d_cap: positive, +inf allowed, no nan
NWK_HD bool nwt_cap_ok(double d_cap) { return d_cap > 0.0; }

// twin[0 .. 3 nf): -1 or the half-edge that runs the other way along the same edge, mutually
NWK_HD bool nwt_twins_ok(const int *faces, const int *twin, long long nf)
{
    for (long long h = 0; h < 3 * nf; ++h) {
        const long long t = twin[h];
        if (t == -1) continue;
        if (t < 0 || t >= 3 * nf || t == h || twin[t] != h) return false;
        if (faces[t] != faces[nwt_next(h)] || faces[nwt_next(t)] != faces[h]) return false;
    }
    return true;
}
