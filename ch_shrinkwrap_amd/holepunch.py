"""
Hole punching at block boundaries: ctypes binding of include/nw_holepunch.h (the point queries, in libnanowrap_hip.so) and the host
half of upstream's punch_holes (ch_shrinkwrap/_membrane_mesh.pyx:1163-1199), which MembraneMesh.punch_holes drives:

    step 1  candidate faces (no localization within eps of the centroid)     nwh_empty_faces   (GPU)
    step 2  pairing of opposite candidates + upstream's index post-processing  nwh_pair_faces    (GPU) + pair_postprocess
    step 3  empty prisms: one flag per pair, then the sequential greedy pass     nwh_prism_empty   (GPU) + prism_greedy
    step 4  two sweeps of min-label propagation                                 connect_candidates
    step 5  Euler characteristic per component                                  component_euler_characteristic
    step 6  plan the punches and cut the tubes                                  plan_punches + apply_punches

Steps 1-5 follow the reference line by line.  Step 6's primitives are PYME's (absent upstream), so the surgery is this package's own:
both patches and their interior vertices go, the two boundary loops are joined by a strip of triangles, no vertex is created.
Half-edge 3f+k of the mirror runs faces[f,k] -> faces[f,(k+1)%3] (trimesh.py): a face's half-edge h = 3f, next(h) = 3f+1, prev(h) = 3f+2.
"""
import ctypes

import numpy as np

from . import _lib
from .trimesh import NEIGHBORSIZE

SYMBOLS = ['nwh_abi_version', 'nwh_create', 'nwh_destroy', 'nwh_last_error', 'nwh_set_points', 'nwh_empty_faces', 'nwh_pair_faces',
           'nwh_prism_empty']
ABI_VERSION = 1
NWH_OK, NWH_ERR_BADARG, NWH_ERR_HIP, NWH_ERR_NONFINITE, NWH_ERR_NOMEM, NWH_ERR_NOPOINTS = 0, -1, -2, -3, -4, -5
ERRORS = {NWH_ERR_BADARG: 'bad argument', NWH_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWH_ERR_NONFINITE: 'non-finite localization',
          NWH_ERR_NOMEM: 'out of device memory', NWH_ERR_NOPOINTS: 'no localizations set'}
COMPONENT_NONE = 1000000          # `self._faces['component'][:] = 1e6` (:1024) in the int32 field

_L = None


def load():
    """The library's nwh_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwh_abi_version': [], 'nwh_create': [i32, ctypes.POINTER(vp)], 'nwh_destroy': [vp], 'nwh_last_error': [vp],
            'nwh_set_points': [vp, vp, i64, f32],
            'nwh_empty_faces': [vp, vp, i64, vp, i64, f32, vp, vp],
            'nwh_pair_faces': [vp, vp, i64, vp, i64, vp, vp, i64, vp],
            'nwh_prism_empty': [vp, vp, i64, vp, i64, vp, vp, vp, i64, f32, vp]}, 'nwh_abi_version', ABI_VERSION, 'nw_holepunch')
    return _L


_p, _mesh = _lib.ptr, _lib.mesh_arrays


class HolePunchContext(_lib.QueryContext):
    """One nwh_ctx: the cell grid of a fit's localizations (set once: they do not move) and the three point queries."""
    prefix, errors, gpu_only, load = 'nwh_', ERRORS, 'hole punching runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_points = 0

    def set_points(self, points, cell_size=0.0):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        self.check(self.L.nwh_set_points(self.h, _p(pts), pts.shape[0], float(cell_size)), 'nwh_set_points')
        self.n_points = pts.shape[0]

    def empty_faces(self, pos, faces, eps, return_dist=False):
        """(F,) bool: no localization within eps of the face centroid (and the nearest distance clipped at eps)."""
        pos, faces = _mesh(pos, faces)
        far = np.empty(faces.shape[0], np.uint8)
        dist = np.empty(faces.shape[0], np.float32) if return_dist else None
        self.check(self.L.nwh_empty_faces(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0], float(eps), _p(far), _p(dist)), 'nwh_empty_faces')
        return (far.astype(bool), dist) if return_dist else far.astype(bool)

    def pair_faces(self, pos, faces, face_normals, cands):
        """(C,) int32: the raw `pairs` array of c_holepunch_pair_candidate_faces (index into cands, or -1)."""
        pos, faces = _mesh(pos, faces)
        fn = np.ascontiguousarray(face_normals, np.float32).reshape(-1, 3)
        cands = np.ascontiguousarray(cands, np.int32)
        pairs = np.full(cands.shape[0], -1, np.int32)
        if cands.shape[0] == 0:
            return pairs
        self.check(self.L.nwh_pair_faces(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0], _p(fn), _p(cands), cands.shape[0], _p(pairs)),
                   'nwh_pair_faces')
        return pairs

    def prism_empty(self, pos, faces, face_normals, cands, pair_idx, eps):
        """(C,) bool: the prism between candidate k and candidate pair_idx[k] holds no localization."""
        pos, faces = _mesh(pos, faces)
        fn = np.ascontiguousarray(face_normals, np.float32).reshape(-1, 3)
        cands = np.ascontiguousarray(cands, np.int32)
        pair_idx = np.ascontiguousarray(pair_idx, np.int32)
        out = np.zeros(cands.shape[0], np.uint8)
        if cands.shape[0] == 0:
            return out.astype(bool)
        if pair_idx.shape != cands.shape:
            raise ValueError('prism_empty: one pair index per candidate')
        self.check(self.L.nwh_prism_empty(self.h, _p(pos), pos.shape[0], _p(faces), faces.shape[0], _p(fn), _p(cands), _p(pair_idx),
                                          cands.shape[0], float(eps), _p(out)), 'nwh_prism_empty')
        return out.astype(bool)


# ---- host steps -------------------------------------------------------------------------------------------------------------------
def pair_postprocess(candidates, pairs):
    """_membrane_mesh.pyx:905-910: candidates that found a pair, and their pair mapped through cumsum(pairs != -1) - 1 -- which sends an
    unpaired j onto the paired entry before it (upstream's quirk, reproduced: it decides which faces step 3 tests)."""
    pair_inds = pairs != -1
    new_inds = np.cumsum(pair_inds) - 1
    return candidates[pair_inds], new_inds[pairs[pair_inds]]


def prism_greedy(candidates, candidate_pair, empty):
    """The sequential pass of _holepunch_empty_prism_candidate_faces (:960-1016) fed by the per-pair emptiness flags."""
    n = len(candidates)
    kept = np.zeros(n, bool)
    disallowed = np.zeros(n, bool)
    where = {}
    for k, f in enumerate(candidates.tolist()):
        where.setdefault(f, []).append(k)
    cand_list, pair_list, empty_list = candidates.tolist(), np.asarray(candidate_pair).tolist(), np.asarray(empty).tolist()
    for i in range(n):
        j = pair_list[i]
        if kept[i] or disallowed[i] or kept[j] or disallowed[j]:
            continue
        if empty_list[i]:
            kept[i] = True
            disallowed[where[cand_list[j]]] = True        # disallowed[candidates == candidates[j]]
    c = candidates[kept]
    cp = candidates[np.asarray(candidate_pair)[kept]]
    return np.hstack([c, cp]), np.hstack([np.arange(len(c), 2 * len(c)), np.arange(len(c))])


def connect_candidates(candidates, twin):
    """_holepunch_connect_candidates (:1018-1054): TWO sweeps of min-label propagation over the face-adjacency graph in candidate order (not a
    full connected-components labelling).  Labels live in a local array (the mirror's face records carry none)."""
    cand = np.asarray(candidates).tolist()
    comp = {}                                             # face -> label; a face that is no candidate has COMPONENT_NONE
    for k, f in enumerate(cand):
        comp[f] = k                                       # (a face listed twice keeps its last index, as the array assignment does)
    members = set(cand)
    tw = twin
    for _ in range(2):
        for c in cand:
            e = (3 * c, 3 * c + 1, 3 * c + 2)             # e0 = face halfedge, e1 = next, e2 = prev
            nb = []
            lab = [comp[c]]
            for h in e:
                t = int(tw[h])
                if t != -1:
                    g = t // 3
                    nb.append(g)
                    lab.append(comp.get(g, COMPONENT_NONE))
                else:
                    nb.append(None)
                    lab.append(COMPONENT_NONE)
            new = min(lab)
            comp[c] = new
            for g in nb:
                # upstream writes here without the twin != -1 guard (:1048-1053 index half-edge -1 on an open border): guarded
                if g is not None and g in members:
                    comp[g] = new
    return np.array([comp[c] for c in cand], dtype=np.int64)


def component_euler_characteristic(candidates, component, faces):
    """_holepunch_component_euler_characteristic (:1056-1080): V - E + F of each component's faces (a face listed twice counts twice in F)."""
    unique_components = np.unique(component)
    chi = np.zeros_like(unique_components)
    for i, c in enumerate(unique_components):
        fv3 = faces[np.asarray(candidates)[component == c]]
        v0, v1, v2 = fv3[:, 0], fv3[:, 1], fv3[:, 2]          # prev(h), h, next(h) vertices of the face's half-edge
        fv = np.hstack([v0, v1, v2])
        F = len(v0)
        V = len(set(fv.ravel().tolist()))
        edges = np.vstack([fv, np.hstack([v1, v2, v0])]).T
        E = len(np.unique(np.sort(edges, axis=1), axis=0))
        chi[i] = V - E + F
    return chi


def patch_boundary(faces, twin, patch):
    """(loop, interior vertices, None) of a patch whose boundary is one simple loop -- the loop as vertices a_0, a_1, ... with the patch's
    half-edges running a_k -> a_k+1 -- or (None, None, reason)."""
    patch = np.unique(np.asarray(patch, np.int64))
    he = (3 * patch[:, None] + np.arange(3)).ravel()
    tw = twin[he]
    if (tw == -1).any():
        return None, None, 'patch reaches an open border of the mesh'
    bnd = he[~np.isin(tw // 3, patch)]
    if bnd.size == 0:
        return None, None, 'patch is a closed surface'
    origin = faces[bnd // 3, bnd % 3]
    dest = faces[bnd // 3, (bnd % 3 + 1) % 3]
    if np.unique(origin).size != origin.size:
        return None, None, 'boundary is not a simple loop (a vertex is on it twice)'
    nxt = dict(zip(origin.tolist(), dest.tolist()))
    loop = [int(origin[0])]
    while True:
        v = nxt.get(loop[-1])
        if v is None:
            return None, None, 'boundary is not closed'
        if v == loop[0]:
            break
        loop.append(v)
        if len(loop) > origin.size:
            return None, None, 'boundary is not closed'
    if len(loop) != origin.size:
        return None, None, 'boundary has %d edges off its first loop (two or more loops)' % (origin.size - len(loop))
    interior = set(faces[patch].ravel().tolist()) - set(loop)
    return loop, interior, None


def _tube(pos, loop_a, loop_b):
    """Triangles joining loop A (a_k -> a_k+1 as in its patch) and loop B, started at their nearest vertex pair and zipped in proportion
    to the loops' lengths.  Each triangle holds one loop edge in its patch's direction, so the strip is oriented like the faces it replaces."""
    # upstream aligns at np.argmin over the flattened (n, 3) array of squared coordinate differences (:738): here the nearest pair of all
    A = np.asarray(loop_a)
    B = np.asarray(loop_b)
    n, m = A.size, B.size
    pa, pb = pos[A].astype(np.float64), pos[B].astype(np.float64)
    d2 = ((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1)
    ka, kb = np.unravel_index(int(np.argmin(d2)), d2.shape)
    A = A[(ka + np.arange(n)) % n]
    Bp = B[(kb - np.arange(m)) % m]                       # B walked against its own direction, from the nearest vertex
    tris, diag = [], [(int(A[0]), int(Bp[0]))]
    seen = {(0, 0)}
    k = t = 0
    while k < n or t < m:
        # (a step may not come back to a vertex pair the strip has joined already -- A wrapped round to a_0 while B still stands where it
        # stood at the start: that diagonal would be an edge of four triangles)
        ok_a = k < n and ((k + 1) % n, t % m) not in seen or (k + 1, t) == (n, m)
        ok_b = t < m and (k % n, (t + 1) % m) not in seen or (k, t + 1) == (n, m)
        if not ok_b:
            adv_a = True
        elif not ok_a:
            adv_a = False
        else:
            adv_a = (2 * k + 1) * m <= (2 * t + 1) * n      # in step with the loops' lengths: no vertex gets a long fan
        if adv_a:
            tris.append((A[k % n], A[(k + 1) % n], Bp[t % m]))
            k += 1
        else:
            tris.append((Bp[(t + 1) % m], Bp[t % m], A[k % n]))
            t += 1
        seen.add((k % n, t % m))
        diag.append((int(A[k % n]), int(Bp[t % m])))
    return np.array(tris, np.int32).reshape(-1, 3), diag[:-1]


def _regions(faces_kept, twin):
    """{face: region id} of the edge-connected regions of a face set (a full connected-components labelling)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    kept = np.unique(np.asarray(faces_kept, np.int64))
    local = {f: k for k, f in enumerate(kept.tolist())}
    tw = twin[(3 * kept[:, None] + np.arange(3)).ravel()]
    g = np.where(tw >= 0, tw // 3, -1)
    src = np.repeat(np.arange(kept.size), 3)
    ok = np.isin(g, kept)
    dst = np.array([local[x] for x in g[ok].tolist()], np.int64)
    n, lab = connected_components(coo_matrix((np.ones(dst.size), (src[ok], dst)), shape=(kept.size, kept.size)), directed=False)
    return dict(zip(kept.tolist(), lab.tolist()))


def _check_patch(faces, twin, patch, punched_vertices):
    """(loop, interior, vertex set, None) of a patch that can be cut out, or (None, None, vertex set, reason)"""
    verts = set(faces[patch].ravel().tolist())
    if verts & punched_vertices:
        return None, None, verts, 'touches a patch punched in this call'
    chi = int(component_euler_characteristic(patch, np.zeros(len(patch), np.int64), faces)[0])
    if chi != 1:
        return None, None, verts, 'region of Euler characteristic %d, not a disk' % chi
    loop, interior, reason = patch_boundary(faces, twin, patch)
    return loop, interior, verts, reason


def plan_punches(pos, faces, twin, candidates, candidate_pairs, component, euler, region_faces=None):
    """_holepunch_update_topology (:1082-1126) as a plan: [(patch, paired patch, tube triangles, interior vertices)], skips [(component, reason)].
    Nothing is changed here; apply_punches performs the plan in one go (the punches share no vertex, so their order does not matter).

    Components are visited in upstream's order, with upstream's tests (chi 0 and chi != 1 skipped, a pair in the same or in a used
    component passed over).  What is cut is the component's REGION: every face of `region_faces` (punch_holes passes step 1's candidates:
    the faces with no localization near) edge-connected to it.  Upstream cuts the component itself (:1111); its two sweeps (:1018-1054)
    and the one-to-one pass of step 3 leave one empty opening as many small components, and one hole would come out as dozens of slivers
    between single triangles, which the next remesh cannot take (vertices beyond the 1-ring table's NEIGHBORSIZE slots)."""
    candidates = np.asarray(candidates)
    candidate_pairs = np.asarray(candidate_pairs)
    component = np.asarray(component)
    unique_components = np.unique(component)
    used = np.zeros(len(unique_components), bool)
    region_of = _regions(np.concatenate([np.asarray(candidates).ravel(), np.asarray([] if region_faces is None else region_faces, np.int64).ravel()]), twin)
    kept = np.array(sorted(region_of), np.int64)
    kept_region = np.array([region_of[f] for f in kept.tolist()], np.int64)
    punched_vertices, punched_regions = set(), set()
    plan, skips = [], []

    def region_patch(faces_c):
        regs = {region_of[f] for f in np.asarray(faces_c).tolist()}
        return frozenset(regs), kept[np.isin(kept_region, list(regs))]

    for i, c in enumerate(unique_components):
        if used[i]:
            continue
        idx = component == c
        if euler[i] == 0:
            skips.append((int(c), 'Euler characteristic 0 (the tube cut is disabled upstream)'))
        elif euler[i] == 1:
            regs_a, pa = region_patch(candidates[idx])
            if regs_a & punched_regions:
                used[i] = True                             # (its faces went with a region punched in this call)
                continue
            loop_a, in_a, va, reason = _check_patch(faces, twin, pa, punched_vertices)
            if reason is not None:
                skips.append((int(c), reason))
                used[i] = True
                continue
            tried = set()
            for pair_idx in candidate_pairs[idx]:
                if component[pair_idx] == c:
                    continue
                pci = int(np.argmax(unique_components == component[pair_idx]))
                if used[pci]:
                    continue
                regs_b, pb = region_patch(candidates[component == component[pair_idx]])
                if regs_b == regs_a or regs_b in tried:
                    continue
                tried.add(regs_b)
                # upstream punches the first pair it meets and stops (:1106-1121); a pair that cannot be cut here is skipped and the next
                # pair of the component is tried instead
                loop_b, in_b, vb, reason = _check_patch(faces, twin, pb, punched_vertices)
                reason = reason and 'paired patch: ' + reason
                if reason is None and va & vb:
                    reason = 'the two patches share a vertex'           # (upstream would join the loops regardless, :731-814)
                if reason is None:
                    tris, diag = _tube(pos, loop_a, loop_b)
                    if len({(min(a, b), max(a, b)) for a, b in diag}) != len(diag):
                        reason = 'no strip joins the two loops without repeating an edge'
                if reason is None:
                    loop_v = np.array(loop_a + loop_b)
                    touching = np.isin(faces, loop_v).any(1)
                    near = faces[touching]
                    nv = np.int64(pos.shape[0])
                    e = np.sort(np.concatenate([near[:, [0, 1]], near[:, [1, 2]], near[:, [2, 0]]]), 1).astype(np.int64)
                    existing = set((e[:, 0] * nv + e[:, 1]).tolist())
                    if any(min(a, b) * int(nv) + max(a, b) in existing for a, b in diag):
                        reason = 'a tube edge would duplicate an edge of the mesh'
                if reason is None:
                    # the mirror's 1-ring table has NEIGHBORSIZE slots: a loop vertex may not end up with more neighbours than that
                    rest = near[~np.isin(np.flatnonzero(touching), np.concatenate([pa, pb]))]
                    after = np.vstack([rest, tris])
                    nbrs = {}
                    for a, b in np.concatenate([after[:, [0, 1]], after[:, [1, 2]], after[:, [2, 0]]]).tolist():
                        nbrs.setdefault(a, set()).add(b)
                        nbrs.setdefault(b, set()).add(a)
                    if max(len(nbrs[x]) for x in loop_v.tolist()) > NEIGHBORSIZE:
                        reason = 'a boundary vertex would get more than %d neighbours' % NEIGHBORSIZE
                if reason is not None:
                    skips.append((int(c), reason))
                    continue
                plan.append((pa, pb, tris, in_a | in_b))
                punched_vertices |= va | vb
                punched_regions |= regs_a | regs_b
                used[pci] = True
                break
        else:
            skips.append((int(c), 'Euler characteristic %d' % int(euler[i])))   # (upstream prints "I don't know what to do with this")
        used[i] = True
    return plan, skips


def apply_punches(vertices, faces, plan):
    """(vertices, faces) with every planned patch removed, its interior vertices dropped and the tubes added; no vertex is created."""
    if not plan:
        return vertices, faces
    gone = np.concatenate([np.concatenate([pa, pb]) for pa, pb, _, _ in plan])
    keep_f = np.ones(faces.shape[0], bool)
    keep_f[gone] = False
    new_faces = np.vstack([faces[keep_f]] + [t for _, _, t, _ in plan])
    keep_v = np.ones(vertices.shape[0], bool)
    for _, _, _, interior in plan:
        keep_v[list(interior)] = False
    remap = np.cumsum(keep_v) - 1
    if not keep_v[new_faces].all():
        raise RuntimeError('hole punch: a removed vertex is still referenced')          # (a patch interior is only the patch's)
    return np.ascontiguousarray(vertices[keep_v]), np.ascontiguousarray(remap[new_faces], np.int32)
