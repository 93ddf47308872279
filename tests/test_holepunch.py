"""CPU tests of hole punching: the surgery (step 6), the skip paths, steps 4-5 against a line-for-line restatement of upstream's
_membrane_mesh.pyx:1018-1080, the hook surface of MembraneMesh / ShrinkwrapMembrane and the C-ABI's argument checks (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from ch_shrinkwrap_amd import holepunch as H
from ch_shrinkwrap_amd.membrane_mesh import MembraneMesh, ShrinkwrapMembrane
from ch_shrinkwrap_amd.trimesh import icosphere, TriMesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pancake(nsub=3, radius=100.0, flat=0.3):
    v, f = icosphere(nsub, radius)
    v = v.copy()
    v[:, 2] *= flat
    return v, f


def disk(v, f, top, r):
    c = v[f].mean(1)
    return np.flatnonzero(((c[:, 2] > 0) == top) & (np.hypot(c[:, 0], c[:, 1]) < r)).astype('i4')


def euler(v, f):
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    return v.shape[0] - e.shape[0] + f.shape[0]


def closed_oriented(f):
    """every directed edge exactly once, and its reverse present"""
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    rkey = e[:, 1] * (1 << 32) + e[:, 0]
    return np.unique(key).size == key.size and np.isin(rkey, key).all()


def kept_pair_lists(top, bot):
    """(candidates, candidate_pairs) as step 3 hands them on: hstack([c, cp]) with crossed indices"""
    n = min(len(top), len(bot))
    c, cp = top[:n], bot[:n]
    return np.hstack([c, cp]), np.hstack([np.arange(n, 2 * n), np.arange(n)])


# ---- step 6: the surgery ----------------------------------------------------------------------------------------------------------
def test_surgery_on_a_pancake_opens_one_oriented_hole():
    v, f = pancake()
    m = MembraneMesh(v, f)
    top, bot = disk(v, f, True, 35.0), disk(v, f, False, 35.0)
    cands, pairs = kept_pair_lists(top, bot)
    comp = m._holepunch_connect_candidates(cands)
    chi = m._holepunch_component_euler_characteristic(cands, comp)
    assert list(chi) == [1, 1]
    holes, skips = m._holepunch_update_topology(cands, pairs, comp, chi)
    assert holes == 1 and skips == []
    nv, nf = np.asarray(m.vertices), np.asarray(m.faces)
    assert closed_oriented(nf)
    assert euler(nv, nf) == euler(v, f) - 2
    # no new vertices: every vertex is one of the input's, bit for bit; the patches' interior vertices are gone
    old = {tuple(p) for p in v.tolist()}
    assert all(tuple(p) in old for p in nv.tolist())
    interior = set(f[np.concatenate([top, bot])].ravel().tolist())
    for patch in (top, bot):
        loop, inner, reason = H.patch_boundary(f, TriMesh(v, f)._halfedges['twin'], patch)
        interior -= set(loop)
    assert nv.shape[0] == v.shape[0] - len(interior)
    kept_pos = {tuple(p) for p in nv.tolist()}
    assert not any(tuple(v[i]) in kept_pos for i in interior)
    # none of the patch faces is left (compared by corner positions)
    tri = lambda P, F: {tuple(sorted(map(tuple, P[t].tolist()))) for t in F}
    assert not (tri(v, f[np.concatenate([top, bot])]) & tri(nv, nf))
    # the mesh is a valid mirror again (half-edge records rebuilt, twins everywhere)
    assert (m._halfedges['twin'] != -1).all()


def _unchanged(m, v, f):
    return np.array_equal(np.asarray(m.vertices), v) and np.array_equal(np.asarray(m.faces), f)


def test_patches_that_share_a_vertex_are_skipped():
    v, f = pancake()
    m = MembraneMesh(v, f)
    # two faces of one fan that share only their apex vertex
    top = disk(v, f, True, 200.0)
    apex = np.bincount(f[top].ravel()).argmax()
    fan = [int(t) for t in top if apex in f[t]]
    a = fan[0]
    b = next(t for t in fan[1:] if len(set(f[a]) & set(f[t])) == 1)
    cands, pairs = np.array([a, b], 'i4'), np.array([1, 0])
    comp = m._holepunch_connect_candidates(cands)
    chi = m._holepunch_component_euler_characteristic(cands, comp)
    assert len(set(comp.tolist())) == 2 and list(chi) == [1, 1]
    holes, skips = m._holepunch_update_topology(cands, pairs, comp, chi)
    assert holes == 0 and len(skips) == 1 and 'share a vertex' in skips[0][1]
    assert _unchanged(m, v, f)


def _annulus(v, f, top):
    c = v[f].mean(1)
    rr = np.hypot(c[:, 0], c[:, 1])
    return np.flatnonzero(((c[:, 2] > 0) == top) & (rr > 30.0) & (rr < 60.0)).astype('i4')


def test_a_patch_with_more_than_one_boundary_loop_is_skipped():
    v, f = pancake()
    m = MembraneMesh(v, f)
    ring, centre = _annulus(v, f, True), disk(v, f, True, 15.0)          # an annulus (chi 0) and a disk (chi 1) under one label: chi 1, three loops
    other = disk(v, f, False, 35.0)
    cands = np.hstack([ring, centre, other]).astype('i4')
    comp = np.hstack([np.zeros(len(ring) + len(centre), np.int64), np.ones(len(other), np.int64)])
    pairs = np.hstack([np.full(len(ring) + len(centre), len(ring) + len(centre)), np.zeros(len(other), np.int64)])
    chi = m._holepunch_component_euler_characteristic(cands, comp)
    assert list(chi) == [1, 1]
    holes, skips = m._holepunch_update_topology(cands, pairs, comp, chi)
    assert holes == 0 and len(skips) == 1 and 'loop' in skips[0][1]
    assert _unchanged(m, v, f)


def test_a_component_of_euler_characteristic_zero_is_skipped():
    v, f = pancake()
    m = MembraneMesh(v, f)
    cands = _annulus(v, f, True)
    comp = np.zeros(len(cands), np.int64)           # (one label by hand: the two sweeps may leave an annulus under several)
    chi = m._holepunch_component_euler_characteristic(cands, comp)
    assert list(chi) == [0]
    holes, skips = m._holepunch_update_topology(cands, np.zeros(len(cands), np.int64), comp, chi)
    assert holes == 0 and skips == [(int(np.unique(comp)[0]), 'Euler characteristic 0 (the tube cut is disabled upstream)')]
    assert _unchanged(m, v, f)


def test_a_split_opening_is_cut_as_one_region():
    """upstream's labelling may leave one empty opening under several components: the surgery cuts the whole edge-connected region once"""
    v, f = pancake()
    m = MembraneMesh(v, f)
    top, bot = disk(v, f, True, 35.0), disk(v, f, False, 35.0)
    west = v[f[top]].mean(1)[:, 0] < 0                                # the top disk as two half-disks under two labels
    top = np.concatenate([top[west], top[~west]])
    cands = np.hstack([top, bot]).astype('i4')
    comp = np.hstack([np.zeros(west.sum()), np.ones((~west).sum()), np.full(len(bot), 2)]).astype(np.int64)
    pairs = np.hstack([np.full(len(top), len(top)), np.zeros(len(bot))]).astype(np.int64)
    chi = m._holepunch_component_euler_characteristic(cands, comp)
    assert list(chi) == [1, 1, 1]
    holes, skips = m._holepunch_update_topology(cands, pairs, comp, chi)
    assert holes == 1
    nv, nf = np.asarray(m.vertices), np.asarray(m.faces)
    assert closed_oriented(nf) and euler(nv, nf) == euler(v, f) - 2
    tri = lambda P, F: {tuple(sorted(map(tuple, P[t].tolist()))) for t in F}
    assert not (tri(v, f[cands]) & tri(nv, nf))                      # both halves of the top disk went


def test_a_pair_that_cannot_be_cut_passes_on_to_the_next_pair():
    """upstream's update loop takes a component's pairs in turn (:1106-1121): a pair skipped here does not end the component"""
    v, f = pancake()
    m = MembraneMesh(v, f)
    top, bot = disk(v, f, True, 35.0), disk(v, f, False, 35.0)
    tv = set(f[top].ravel().tolist())
    edge_nb = set((TriMesh(v, f)._halfedges['twin'][(3 * top[:, None] + np.arange(3)).ravel()] // 3).tolist())
    other = next(int(t) for t in range(f.shape[0]) if t not in set(top.tolist()) and t not in edge_nb and len(set(f[t]) & tv) == 1)
    cands = np.hstack([top, [other], bot]).astype('i4')
    comp = np.hstack([np.zeros(len(top)), [1], np.full(len(bot), 2)]).astype(np.int64)
    pairs = np.hstack([[len(top)], np.full(len(top) - 1, len(top) + 1), [0], np.zeros(len(bot))]).astype(np.int64)
    chi = m._holepunch_component_euler_characteristic(cands, comp)
    assert list(chi) == [1, 1, 1]
    holes, skips = m._holepunch_update_topology(cands, pairs, comp, chi)
    assert holes == 1
    assert (0, 'the two patches share a vertex') in skips
    assert closed_oriented(np.asarray(m.faces))


# ---- steps 4-5 against the restatement ----------------------------------------------------------------------------------------------
def restated_connect(candidates, face_halfedge, he_next, he_prev, he_twin, he_face, n_faces):
    """_membrane_mesh.pyx:1018-1054, line for line, on a local label array; the writes get the twin != -1 guard the reads have"""
    component = np.full(n_faces, 1000000, np.int32)
    component[candidates] = range(len(candidates))
    for _ in range(2):
        for c in candidates:
            e0 = face_halfedge[c]
            e1 = he_next[e0]
            e2 = he_prev[e0]
            c0, c1, c2 = 1e6, 1e6, 1e6
            if he_twin[e0] != -1:
                c0 = component[he_face[he_twin[e0]]]
            if he_twin[e1] != -1:
                c1 = component[he_face[he_twin[e1]]]
            if he_twin[e2] != -1:
                c2 = component[he_face[he_twin[e2]]]
            new_component = np.min([component[c], c0, c1, c2])
            component[c] = new_component
            if he_twin[e0] != -1 and he_face[he_twin[e0]] in candidates:
                component[he_face[he_twin[e0]]] = new_component
            if he_twin[e1] != -1 and he_face[he_twin[e1]] in candidates:
                component[he_face[he_twin[e1]]] = new_component
            if he_twin[e2] != -1 and he_face[he_twin[e2]] in candidates:
                component[he_face[he_twin[e2]]] = new_component
    return component[candidates]


def restated_euler(candidates, component, face_halfedge, he_prev, he_next, he_vertex):
    """_membrane_mesh.pyx:1056-1080, line for line"""
    unique_components = np.unique(component)
    chi = np.zeros_like(unique_components)
    for i, c in enumerate(unique_components):
        he = face_halfedge[candidates[component == c]]
        v0 = he_vertex[he_prev[he]]
        v1 = he_vertex[he]
        v2 = he_vertex[he_next[he]]
        fv = np.hstack([v0, v1, v2])
        F = len(he)
        V = len(set(fv.ravel()))
        edges = np.vstack([fv, np.hstack([v1, v2, v0])]).T
        sorted_edges = np.sort(edges, axis=1)
        E = len(np.unique(sorted_edges, axis=0))
        chi[i] = V - E + F
    return chi


def _records(m):
    he = m._halfedges
    return m._faces['halfedge'], he['next'], he['prev'], he['twin'], he['face'], he['vertex']


def strip(k=12):
    """an open strip of 2k triangles whose dual graph is a path: t_2i = (a_i, b_i, a_i+1), t_2i+1 = (b_i, b_i+1, a_i+1)"""
    a = np.stack([np.arange(k + 1), np.zeros(k + 1), np.zeros(k + 1)], 1)
    b = np.stack([np.arange(k + 1), np.ones(k + 1), np.zeros(k + 1)], 1)
    v = np.vstack([a, b]).astype('f4')
    A, B = np.arange(k + 1), np.arange(k + 1) + k + 1
    f = []
    for i in range(k):
        f.append((A[i], B[i], A[i + 1]))
        f.append((B[i], B[i + 1], A[i + 1]))
    return v, np.array(f, 'i4')


@pytest.mark.parametrize('case', ['pancake_pairs', 'self_pair', 'strip_split'])
def test_components_and_euler_characteristic_match_the_restatement(case):
    if case == 'strip_split':
        v, f = strip(12)
        m = MembraneMesh(v, f)
        chain = np.arange(f.shape[0], dtype='i4')                     # faces of the strip in path order
        cands = np.hstack([chain[-1:], chain[:-1]]).astype('i4')        # the last one first: its label 0 has to travel the whole path
    else:
        v, f = pancake()
        m = MembraneMesh(v, f)
        top, bot = disk(v, f, True, 45.0), disk(v, f, False, 45.0)
        if case == 'pancake_pairs':
            rng = np.random.default_rng(3)
            cands, _ = kept_pair_lists(rng.permutation(top), rng.permutation(bot))
        else:
            cands = np.hstack([top[:5], top[:1], top[5:9]]).astype('i4')    # a face listed twice (step 3's self-pair)
    fh, nx, pv, tw, fc, vx = _records(m)
    ref = restated_connect(cands, fh, nx, pv, tw, fc, f.shape[0])
    got = m._holepunch_connect_candidates(cands)
    assert np.array_equal(got, ref)
    assert np.array_equal(m._holepunch_component_euler_characteristic(cands, got), restated_euler(cands, ref, fh, pv, nx, vx))
    if case == 'strip_split':
        # the strip is ONE edge-connected patch, yet the two sweeps leave it under two labels: upstream's labelling, not a full one
        assert len(np.unique(got)) == 2
    if case == 'self_pair':
        assert 2 in m._holepunch_component_euler_characteristic(cands, got).tolist() or len(np.unique(got)) > 1


def test_pair_postprocess_maps_an_unpaired_partner_onto_the_previous_paired_entry():
    cands = np.array([10, 11, 12, 13, 14], 'i4')
    pairs = np.array([2, 4, -1, -1, -1], 'i4')                          # 0 -> 2 (unpaired), 1 -> 4 (unpaired)
    c, p = H.pair_postprocess(cands, pairs)
    assert c.tolist() == [10, 11] and p.tolist() == [1, 1]              # cumsum([1,1,0,0,0]) - 1 = [0,1,1,1,1]


def test_prism_greedy_is_the_sequential_pass():
    cands = np.array([5, 6, 7, 8], 'i4')
    pair = np.array([2, 2, 3, 0])
    empty = np.array([True, True, True, False])
    c, p = H.prism_greedy(cands, pair, empty)
    # 0 keeps (7 disallowed); 1 -> 2 is disallowed; 2 is disallowed; 3 -> 0 is kept already
    assert c.tolist() == [5, 7] and p.tolist() == [1, 0]


# ---- the hook surface -----------------------------------------------------------------------------------------------------------------
class _StubCG(object):
    def refresh_normals(self):
        pass


def _boundary(m, calls):
    m.cg = _StubCG()
    m.punch_holes = lambda pts, eps: calls.append(eps)
    plan = MembraneMesh._BlockPlan(m, 10, np.full((4, 3), 10.0), 5.0)
    assert plan.punch and not plan.remesh
    m._block_boundary(np.zeros((4, 3), 'f4'), 5, plan)


def test_no_hole_puncher_means_no_punching_and_device_means_punch_holes():
    v, f = pancake(2)
    calls = []
    m = MembraneMesh(v, f, remesh_frequency=0, delaunay_remesh_frequency=5, delaunay_eps=50.0)
    assert m.hole_puncher is None
    _boundary(m, calls)
    assert calls == [] and m.punch_log == []
    m = MembraneMesh(v, f, remesh_frequency=0, delaunay_remesh_frequency=5, delaunay_eps=50.0, hole_puncher='device')
    _boundary(m, calls)
    assert calls == [50.0]
    seen = []
    m = MembraneMesh(v, f, remesh_frequency=0, delaunay_remesh_frequency=5, delaunay_eps=50.0, hole_puncher=lambda mesh, p, e: seen.append(e))
    m.cg = _StubCG()
    m._block_boundary(np.zeros((4, 3), 'f4'), 5, MembraneMesh._BlockPlan(m, 10, np.full((4, 3), 10.0), 5.0))
    assert seen == [50.0]


def test_unknown_hole_puncher_is_refused():
    v, f = pancake(2)
    with pytest.raises(ValueError):
        MembraneMesh(v, f, hole_puncher='gpu')
    with pytest.raises(ValueError):
        ShrinkwrapMembrane(hole_puncher='builtin')
    assert ShrinkwrapMembrane().hole_puncher is None
    assert ShrinkwrapMembrane(hole_puncher='device').hole_puncher == 'device'


# ---- the C-ABI ----------------------------------------------------------------------------------------------------------------------
def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_holepunch.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwh_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_binding_matches_its_header():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    assert sorted(H.SYMBOLS) == _declared()
    L = H.load()
    assert L.nwh_abi_version() == H.ABI_VERSION == 1


def test_holepunch_binding_checks_its_arguments_before_it_touches_a_gpu():
    """Bad sizes, NULL pointers, indices outside their arrays and a non-positive eps are refused with NWH_ERR_BADARG -- without a GPU as
    well; with valid arguments and no GPU the context cannot be made (NWH_ERR_HIP): there is no CPU fallback."""
    L = H.load()
    v, f = pancake(1)
    pos = np.ascontiguousarray(v, np.float32)
    faces = np.ascontiguousarray(f, np.int32)
    fn = np.zeros((f.shape[0], 3), np.float32)
    far = np.zeros(f.shape[0], np.uint8)
    cands = np.arange(4, dtype=np.int32)
    out = np.zeros(4, np.int32)
    P = lambda a: a.ctypes.data
    BAD = H.NWH_ERR_BADARG
    assert L.nwh_set_points(None, None, 10, 0.0) == BAD
    assert L.nwh_set_points(None, P(pos), 0, 0.0) == BAD
    assert L.nwh_set_points(None, P(pos), 10, float('nan')) == BAD
    assert L.nwh_empty_faces(None, P(pos), pos.shape[0], P(faces), faces.shape[0], 0.0, P(far), None) == BAD          # eps <= 0
    assert L.nwh_empty_faces(None, P(pos), pos.shape[0], None, faces.shape[0], 10.0, P(far), None) == BAD
    assert L.nwh_empty_faces(None, P(pos), 2, P(faces), faces.shape[0], 10.0, P(far), None) == BAD                  # a face index >= n_vertices
    bad_pos = pos.copy()
    bad_pos[3, 1] = np.nan
    assert L.nwh_empty_faces(None, P(bad_pos), pos.shape[0], P(faces), faces.shape[0], 10.0, P(far), None) == BAD
    bad_c = cands.copy()
    bad_c[2] = faces.shape[0]
    assert L.nwh_pair_faces(None, P(pos), pos.shape[0], P(faces), faces.shape[0], P(fn), P(bad_c), 4, P(out)) == BAD
    assert L.nwh_pair_faces(None, P(pos), pos.shape[0], P(faces), faces.shape[0], None, P(cands), 4, P(out)) == BAD
    pidx = np.array([1, 0, 3, 4], np.int32)                                                                             # 4 is outside [0, 4)
    assert L.nwh_prism_empty(None, P(pos), pos.shape[0], P(faces), faces.shape[0], P(fn), P(cands), P(pidx), 4, 10.0, P(far)) == BAD
    assert L.nwh_create(-1, ctypes.byref(ctypes.c_void_p())) == BAD
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        assert L.nwh_create(0, ctypes.byref(h)) == H.NWH_ERR_HIP and h.value is None
        with pytest.raises(RuntimeError):
            H.HolePunchContext(0)
        with pytest.raises(RuntimeError):
            MembraneMesh(v, f)._holepunch_find_candidate_faces(np.zeros((10, 3), 'f4'), 10.0)
