"""
Neck removal and short-edge cleanup at block boundaries: ctypes binding of include/nw_surgery.h (the mesh-wide queries, in
libnanowrap_hip.so) and the host surgery that upstream's remove_necks / remove_extra_short_edges (ch_shrinkwrap/_membrane_mesh.pyx:
1201-1239) leave to PYME's TriangleMesh: unsafe_remove_vertices -> repair -> remesh(n_relax=0) -> remove_inner_surfaces.  PYME's code
is not in the reference, so the surgery is this package's own, defined here:

    excise           drop every face with a corner in the vertex set
    make_manifold    until stable: a vertex whose faces form more than one fan joins the deleted set, a face with three border edges goes
    boundary_loops   the border half-edges as ordered loops, in order of each loop's smallest half-edge id
    cap_loop         a loop closed with new vertices only: a fan to the centroid up to FAN_MAX edges, concentric rings above
    repair           all of the above, then dust: closed components of fewer than min_component_faces faces go
    guard_regions    the neck guard: which regions of candidate faces are cut (a disk is a bump; a cut may not leave small islands)
    inner_components remove_inner_surfaces' decision: inverted shells, and shells inside another kept shell (winding numbers)

Every labelling step takes the labeller as a parameter, `label_faces(faces, twin, mask) -> (label, n)`: the device's
(SurgeryContext.label_faces) in a fit, scipy's (scipy_label_faces) in the CPU tests.  Half-edge 3f+k runs faces[f,k] -> faces[f,(k+1)%3].
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nws_abi_version', 'nws_create', 'nws_destroy', 'nws_last_error', 'nws_label_faces', 'nws_component_stats', 'nws_winding',
           'nws_short_edge_vertices']
ABI_VERSION = 1
NWS_OK, NWS_ERR_BADARG, NWS_ERR_HIP, NWS_ERR_NOMEM = 0, -1, -2, -3
ERRORS = {NWS_ERR_BADARG: 'bad argument', NWS_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWS_ERR_NOMEM: 'out of device memory'}
FAN_MAX = 12                  # a loop of up to this many edges is closed by a fan; longer ones get concentric rings first
MAX_VALENCE = 16              # the device remesher's max_valence: no cap leaves a vertex with more neighbours

_L = None


def load():
    """The library's nws_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
        _L = _lib.load_entry_points(SYMBOLS, {
            'nws_abi_version': [], 'nws_create': [i32, ctypes.POINTER(vp)], 'nws_destroy': [vp], 'nws_last_error': [vp],
            'nws_label_faces': [vp, vp, vp, vp, i64, vp, vp],
            'nws_component_stats': [vp, vp, i64, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp],
            'nws_winding': [vp, vp, i64, vp, vp, i64, i32, vp, vp, i64, vp],
            'nws_short_edge_vertices': [vp, vp, i64, vp, i64, f32, vp, vp]}, 'nws_abi_version', ABI_VERSION, 'nw_surgery')
    return _L


_p, _mesh = _lib.ptr, _lib.mesh_arrays


class SurgeryContext(_lib.QueryContext):
    """One nws_ctx: the four mesh-wide queries of the block-boundary surgery on one device."""
    prefix, errors, gpu_only, load = 'nws_', ERRORS, 'neck removal and short-edge cleanup run', staticmethod(load)

    def label_faces(self, faces, twin, mask=None):
        """(label (F,) int32, number of components): edge-connected components of the faces with mask != 0, numbered in order of their
        smallest face id; -1 outside the mask."""
        faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        twin = np.ascontiguousarray(twin, np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        label = np.empty(faces.shape[0], np.int32)
        n = ctypes.c_int32()
        if faces.shape[0] == 0:
            return label, 0
        self.check(self.L.nws_label_faces(self.h, _p(faces), _p(twin), _p(m), faces.shape[0], _p(label), ctypes.byref(n)), 'nws_label_faces')
        return label, int(n.value)

    def component_stats(self, pos, faces, twin, label, n):
        """dict(faces, area, volume, bbox (n,6) float32, border) per component of `label`."""
        pos, faces = _mesh(pos, faces)
        twin = np.ascontiguousarray(twin, np.int32)
        label = np.ascontiguousarray(label, np.int32)
        out = dict(faces=np.zeros(n, np.int64), area=np.zeros(n), volume=np.zeros(n), bbox=np.zeros((n, 6), np.float32), border=np.zeros(n, np.int64))
        if n == 0:
            return out
        self.check(self.L.nws_component_stats(self.h, _p(pos), pos.shape[0], _p(faces), _p(twin), _p(label), faces.shape[0], int(n),
                                              _p(out['faces']), _p(out['area']), _p(out['volume']), _p(out['bbox']), _p(out['border'])),
                   'nws_component_stats')
        return out

    def winding(self, pos, faces, label, n, queries, query_component=None):
        """(Q, n) float64: generalized winding number of each query with respect to each component; exactly 0 for the query's own
        component and for a component whose bounding box does not hold the query."""
        pos, faces = _mesh(pos, faces)
        label = np.ascontiguousarray(label, np.int32)
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 3)
        qc = None if query_component is None else np.ascontiguousarray(query_component, np.int32)
        w = np.zeros((q.shape[0], n), np.float64)
        if w.size == 0:
            return w
        self.check(self.L.nws_winding(self.h, _p(pos), pos.shape[0], _p(faces), _p(label), faces.shape[0], int(n), _p(q), _p(qc), q.shape[0],
                                      _p(w)), 'nws_winding')
        return w

    def short_edge_vertices(self, pos, faces, threshold=0.05):
        """((V,) bool: the vertex is the head of a half-edge shorter than threshold * median, the median (float32))."""
        pos, faces = _mesh(pos, faces)
        flag = np.zeros(pos.shape[0], np.uint8)
        med = np.zeros(1, np.float32)
        self.check(self.L.nws_short_edge_vertices(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0], float(threshold), _p(flag), _p(med)),
                   'nws_short_edge_vertices')
        return flag.astype(bool), med[0]


# ---- labelling and adjacency on the host ------------------------------------------------------------------------------------------
def twins(faces, n_vertices=None):
    """twin[3f+k] of an oriented face array whose directed edges are all distinct (-1 on a border): the sort-based definition."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return np.zeros(0, np.int32)
    nv = int(f.max()) + 1 if n_vertices is None else int(n_vertices)
    o, d = f.ravel(), f[:, [1, 2, 0]].ravel()
    key, rkey = o * nv + d, d * nv + o
    order = np.argsort(key, kind='stable')
    sk = key[order]
    p = np.minimum(np.searchsorted(sk, rkey), sk.size - 1)
    return np.where(sk[p] == rkey, order[p], -1).astype(np.int32)


def _renumber(lab, mask):
    """component ids -> 0..C-1 in order of each component's smallest face id; -1 outside the mask"""
    out = np.full(lab.size, -1, np.int32)
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return out, 0
    uniq, first, inv = np.unique(lab[idx], return_index=True, return_inverse=True)
    rank = np.empty(uniq.size, np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(uniq.size)
    out[idx] = rank[inv.reshape(-1)]
    return out, int(uniq.size)


def scipy_label_faces(faces, twin, mask=None):
    """The labeller's contract (SurgeryContext.label_faces) with scipy.sparse.csgraph: the CPU tests' stand-in for the device."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    twin = np.asarray(twin)
    nf = twin.size // 3
    m = np.ones(nf, bool) if mask is None else np.asarray(mask).astype(bool)
    h = np.flatnonzero(twin >= 0)
    a, b = h // 3, twin[h] // 3
    ok = m[a] & m[b]
    g = coo_matrix((np.ones(int(ok.sum())), (a[ok], b[ok])), shape=(nf, nf))
    _, lab = connected_components(g, directed=False)
    return _renumber(lab, m)


def euler_characteristic(faces):
    """V - E + F of a face set (vertices and edges of its faces)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return 0
    e = np.sort(np.stack([f.ravel(), f[:, [1, 2, 0]].ravel()], 1), 1)
    return int(np.unique(f).size - np.unique(e, axis=0).shape[0] + f.shape[0])


# ---- the surgery -------------------------------------------------------------------------------------------------------------------
def excise(faces, vertex_ids, n_vertices):
    """(F,) bool: the faces with no corner in vertex_ids (unsafe_remove_vertices keeps these)"""
    gone = np.zeros(int(n_vertices), bool)
    gone[np.asarray(vertex_ids, np.int64)] = True
    return ~gone[np.asarray(faces)].any(1)


def make_manifold(faces, n_vertices):
    """(indices of the faces kept, vertices that joined the deleted set).  Repeated until nothing changes: a vertex whose faces form
    more than one fan (a bow-tie left by a deletion) loses all of them, and a face whose three edges are all on the border goes."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.ones(faces.shape[0], bool)
    joined = []
    while True:
        idx = np.flatnonzero(keep)
        f = faces[idx]
        if f.shape[0] == 0:
            break
        tw = twins(f, n_vertices)
        # an open fan of k faces has k corners and k - 1 inner edges at its vertex, a closed one as many of each: corners minus the
        # outgoing half-edges that have a twin = the number of open fans
        corners = np.bincount(f.ravel(), minlength=n_vertices)
        links = np.bincount(f.ravel()[tw >= 0], minlength=n_vertices)
        bad = np.flatnonzero(corners - links > 1)
        drop = (tw.reshape(-1, 3) < 0).all(1)
        if bad.size:
            drop |= np.isin(f, bad).any(1)
            joined.append(bad)
        if not drop.any():
            break
        keep[idx[drop]] = False
    return np.flatnonzero(keep), (np.unique(np.concatenate(joined)) if joined else np.zeros(0, np.int64))


def boundary_loops(faces, twin):
    """[[a_0, a_1, ...]]: every loop of border half-edges, the faces' half-edges running a_k -> a_k+1, in order of each loop's smallest
    half-edge id.  Needs one border fan per vertex (make_manifold)."""
    fl = np.asarray(faces).ravel()
    h = np.flatnonzero(np.asarray(twin) < 0)
    if h.size == 0:
        return []
    origin = fl[h]
    dest = fl[3 * (h // 3) + (h % 3 + 1) % 3]
    out_of = dict(zip(origin.tolist(), h.tolist()))
    if len(out_of) != h.size:
        raise ValueError('boundary_loops: a vertex starts two border half-edges (make_manifold first)')
    dest_of = dict(zip(h.tolist(), dest.tolist()))
    seen, loops = set(), []
    for s in h.tolist():
        if s in seen:
            continue
        loop, e = [], s
        while e not in seen:
            seen.add(e)
            loop.append(int(fl[e]))
            e = out_of[dest_of[e]]
        loops.append(loop)
    return loops


def _strip(P, Q):
    """Triangles between ring P (n vertices) and the ring Q inside it (m <= n), both running with the cap's interior on their left,
    zipped in proportion to their lengths from the diagonal P_0 Q_0.  P's edges appear as P_k -> P_k+1, Q's as Q_t+1 -> Q_t."""
    n, m = len(P), len(Q)
    tris, seen = [], {(0, 0)}
    k = t = 0
    while k < n or t < m:
        ok_p = k < n and ((k + 1) % n, t % m) not in seen or (k + 1, t) == (n, m)
        ok_q = t < m and (k % n, (t + 1) % m) not in seen or (k, t + 1) == (n, m)
        if not ok_q:
            adv_p = True
        elif not ok_p:
            adv_p = False
        else:
            adv_p = (2 * k + 1) * m <= (2 * t + 1) * n
        if adv_p:
            tris.append((P[k % n], P[(k + 1) % n], Q[t % m]))
            k += 1
        else:
            tris.append((Q[(t + 1) % m], Q[t % m], P[k % n]))
            t += 1
        seen.add((k % n, t % m))
    return tris


def cap_loop(pos, loop, first_id):
    """(new vertex positions (K,3) float32, faces (M,3)) closing one loop with new vertices numbered from first_id.  The cap takes the
    loop in reverse, so its faces hold a_k+1 -> a_k and agree with the faces around.  Up to FAN_MAX edges: a fan to the loop's centroid.
    Above: rings of ceil(n/2), ceil(n/4), ... vertices (sampled along the loop, pulled towards the centroid), each strip-joined to the one
    outside it, until a ring of at most FAN_MAX closes with a fan.  Every new edge has a new vertex at one end, and a loop vertex gains
    at most two edges."""
    P = list(reversed(loop))
    n = len(P)
    pl = np.asarray(pos, np.float64)[P]
    c = pl.mean(0)
    sizes = [n]
    while sizes[-1] > FAN_MAX:
        sizes.append((sizes[-1] + 1) // 2)
    levels = len(sizes)                   # ring 0 = the loop, rings 1..levels-1 new, the centroid at level `levels`
    new_pos, rings, nid = [], [P], int(first_id)
    for j in range(1, levels):
        m = sizes[j]
        t = np.arange(m) * (n / m)
        i0 = np.floor(t).astype(np.int64) % n
        fr = (t - np.floor(t))[:, None]
        sample = pl[i0] * (1 - fr) + pl[(i0 + 1) % n] * fr
        new_pos.append(c + (1.0 - j / levels) * (sample - c))
        rings.append(list(range(nid, nid + m)))
        nid += m
    centre = nid
    new_pos.append(c[None, :])
    tris = []
    for j in range(levels - 1):
        tris += _strip(rings[j], rings[j + 1])
    last = rings[-1]
    tris += [(last[k], last[(k + 1) % len(last)], centre) for k in range(len(last))]
    return np.vstack(new_pos).astype(np.float32), np.array(tris, np.int64).reshape(-1, 3)


def repair(pos, faces, label_faces, min_component_faces=32):
    """(vertices, faces, info): make_manifold, cap every border loop, drop dust; vertices no face refers to are dropped and the rest
    renumbered in their order, cap vertices after them.  Positions of the vertices kept are not touched (bit for bit).
    info: faces_dropped, vertices_joined, loops, loop_sizes, new_vertices, dust [(component, faces)], kept_faces (indices into `faces`
    of the faces kept before capping), vertex_map (old id -> new id or -1)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = pos.shape[0]
    kept, joined = make_manifold(faces, nv)
    f = faces[kept]
    loops = boundary_loops(f, twins(f, nv)) if f.shape[0] else []
    new_pos, caps, nid = [], [], nv
    for loop in loops:
        p, t = cap_loop(pos, loop, nid)
        new_pos.append(p)
        caps.append(t)
        nid += p.shape[0]
    allpos = np.vstack([pos] + new_pos) if new_pos else pos
    allf = np.vstack([f] + caps) if caps else f
    dust = []
    if allf.shape[0]:
        lab, nc = label_faces(np.ascontiguousarray(allf, np.int32), twins(allf, nid), None)
        cnt = np.bincount(lab[lab >= 0], minlength=nc)
        small = cnt < int(min_component_faces)
        if small.any():
            dust = [(int(c), int(cnt[c])) for c in np.flatnonzero(small)]
            allf = allf[~small[lab]]
    used = np.zeros(nid, bool)
    used[allf.ravel()] = True
    remap = np.where(used, np.cumsum(used) - 1, -1)
    info = dict(faces_dropped=int(faces.shape[0] - kept.size), vertices_joined=int(joined.size), loops=len(loops),
                loop_sizes=[len(l) for l in loops], new_vertices=int(nid - nv), dust=dust, kept_faces=kept, vertex_map=remap[:nv])
    return np.ascontiguousarray(allpos[used]), np.ascontiguousarray(remap[allf], np.int32), info


# ---- the neck guard ---------------------------------------------------------------------------------------------------------------
def region_topology(faces, twin, label, n):
    """(chi, loops, simple) per region of `label` (-1 = no region): Euler characteristic of its faces, the number of loops of its border
    half-edges (those whose twin is -1 or in another region), and whether every border vertex starts exactly one of them."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lab = np.asarray(label)
    twin = np.asarray(twin)
    sel = np.flatnonzero(lab >= 0)
    chi, loops, simple = np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, bool)
    if sel.size == 0 or n == 0:
        return chi, loops, simple
    L = lab[sel].astype(np.int64)
    fs = f[sel]
    # (vertex ids renumbered among the region faces, so that (region, vertex, vertex) keys stay well inside int64)
    uv, inv = np.unique(fs, return_inverse=True)
    loc = inv.reshape(-1, 3).astype(np.int64)
    nv = np.int64(uv.size)
    L3 = np.repeat(L, 3)
    V = np.bincount(np.unique(L3 * nv + loc.ravel()) // nv, minlength=n)
    e = np.sort(np.stack([loc.ravel(), loc[:, [1, 2, 0]].ravel()], 1), 1)
    E = np.bincount(np.unique((L3 * nv + e[:, 0]) * nv + e[:, 1]) // (nv * nv), minlength=n)
    F = np.bincount(L, minlength=n)
    chi = V - E + F
    h = (3 * sel[:, None] + np.arange(3)).ravel()
    t = twin[h]
    border = (t < 0) | (lab[np.maximum(t, 0) // 3] != L3)
    bh, bl = h[border], L3[border]
    if bh.size == 0:
        return chi, loops, simple
    origin = loc.ravel()[border]
    dest = loc[:, [1, 2, 0]].ravel()[border]
    ko, kd = bl * nv + origin, bl * nv + dest
    uo, cnto = np.unique(ko, return_counts=True)
    simple[np.unique(uo[cnto > 1] // nv)] = False
    order = np.argsort(ko, kind='stable')
    sk = ko[order]
    p = np.minimum(np.searchsorted(sk, kd), sk.size - 1)
    nb = bh.size
    succ = np.where(sk[p] == kd, order[p], np.arange(nb))
    # cycles of the successor map by pointer doubling: every half-edge learns the smallest index on its cycle
    low = np.arange(nb)
    s = succ
    for _ in range(int(np.ceil(np.log2(nb + 1))) + 1):
        low = np.minimum(low, low[s])
        s = s[s]
    loops = np.bincount(bl[low == np.arange(nb)], minlength=n)
    return chi, loops, simple


def guard_regions(faces, twin, label, n, label_faces, max_regions=32, min_piece_faces=200):
    """The neck guard: (accepted regions, skips [(region, reason)], info dict(disks, examined)).  A region that is a disk (Euler
    characteristic 1, one simple border loop) is a bump, not a neck: deleting and capping it gives back the same topology.  The others
    are taken in order of their smallest face id, at most max_regions of them; a region is accepted if every piece of the mesh that
    borders it -- the mesh labelled without it and without the regions accepted before it -- has at least min_piece_faces faces: a cut
    that splits the surface or opens a handle passes, a noise cluster that would leave islands does not."""
    faces = np.asarray(faces).reshape(-1, 3)
    twin = np.asarray(twin)
    label = np.asarray(label)
    chi, loops, simple = region_topology(faces, twin, label, n)
    disk = simple & (chi == 1) & (loops == 1)
    removed = np.zeros(faces.shape[0], bool)
    accepted, skips, examined = [], [], 0
    for r in range(n):
        if disk[r]:
            continue
        if examined >= int(max_regions):
            break
        examined += 1
        inr = label == r
        pl, npieces = label_faces(faces, twin, (~(removed | inr)).astype(np.uint8))
        h = (3 * np.flatnonzero(inr)[:, None] + np.arange(3)).ravel()
        t = twin[h]
        g = t[t >= 0] // 3
        bordering = np.unique(pl[g])
        bordering = bordering[bordering >= 0]
        if bordering.size == 0:
            skips.append((r, 'no piece borders it (a whole component)'))
            continue
        sizes = np.bincount(pl[pl >= 0], minlength=npieces)[bordering]
        if sizes.min() < int(min_piece_faces):
            skips.append((r, 'chi %d, %d loops: would leave a piece of %d faces (< %d)' % (chi[r], loops[r], sizes.min(), min_piece_faces)))
            continue
        accepted.append(r)
        removed |= inr
    return accepted, skips, dict(disks=int(disk.sum()), examined=examined)


# ---- inner surfaces ---------------------------------------------------------------------------------------------------------------
def sample_vertices(faces, label, n, n_samples=16):
    """[(component, vertex ids)]: up to n_samples vertices of each component, at evenly spaced ranks of its sorted vertex ids"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    comp = np.full(int(f.max()) + 1 if f.size else 0, -1, np.int64)
    comp[f.ravel()] = np.repeat(np.asarray(label, np.int64), 3)       # (a vertex belongs to the component of its faces)
    vids = np.flatnonzero(comp >= 0)
    order = np.argsort(comp[vids], kind='stable')
    vids, cv = vids[order], comp[vids][order]
    bounds = np.searchsorted(cv, np.arange(n + 1))
    out = []
    for c in range(n):
        v = vids[bounds[c]:bounds[c + 1]]
        k = min(int(n_samples), v.size)
        out.append((c, v[(np.arange(k) * v.size) // max(k, 1)]))
    return out


def inner_components(volume, samples, winding):
    """remove_inner_surfaces' decision: [(component, reason)].  A component goes if its signed volume is <= 0 (an inverted shell), or
    if more than half of its sample vertices have a winding number >= 0.5 with respect to another component that is kept and positively
    oriented; components are decided in order of decreasing volume (a shell inside another is the smaller of the two).
    samples: [(component, vertex ids)] (sample_vertices); winding(vertex ids, their components) -> (Q, C) winding numbers."""
    volume = np.asarray(volume, np.float64)
    out = [(int(c), 'signed volume %.4g <= 0 (an inverted shell)' % volume[c]) for c in np.flatnonzero(~(volume > 0))]
    positive = [c for c in range(volume.size) if volume[c] > 0]
    if len(positive) < 2:
        return out
    qv = np.concatenate([samples[c][1] for c in positive]).astype(np.int64)
    qc = np.concatenate([np.full(samples[c][1].size, c, np.int32) for c in positive])
    w = winding(qv, qc)
    kept = []
    for c in sorted(positive, key=lambda c: (-volume[c], c)):
        r = np.flatnonzero(qc == c)
        if kept and r.size:
            inside = w[r][:, kept] >= 0.5
            if 2 * int(inside.any(1).sum()) > r.size:
                host = int(kept[int(np.argmax(inside.sum(0)))])
                out.append((int(c), '%d of %d samples inside component %d' % (int(inside.any(1).sum()), r.size, host)))
                continue
        kept.append(c)
    return sorted(out)
