"""CPU tests of the neck / short-edge surgery (ch_shrinkwrap_amd/surgery.py): excise, make-manifold, capping and dust on cut spheres, the
neck guard's region decisions with scipy's labeller standing in for the device's, the hook surface of MembraneMesh / ShrinkwrapMembrane
and the C-ABI's argument checks (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

from ch_shrinkwrap_amd import surgery as S
from ch_shrinkwrap_amd.membrane_mesh import MembraneMesh, ShrinkwrapMembrane
from ch_shrinkwrap_amd.trimesh import icosphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = S.scipy_label_faces


def closed_oriented(f):
    """every directed edge exactly once, and its reverse present (every directed edge has exactly one twin)"""
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    rkey = e[:, 1] * (1 << 32) + e[:, 0]
    return np.unique(key).size == key.size and np.isin(rkey, key).all()


def one_fan_per_vertex(f, nv):
    tw = S.twins(f, nv)
    corners = np.bincount(f.ravel(), minlength=nv)
    links = np.bincount(f.ravel()[tw >= 0], minlength=nv)
    return bool((corners == links).all())          # closed fans only, and one each (a closed fan has as many corners as inner edges)


def signed_volumes(v, f):
    lab, n = LABEL(f, S.twins(f, v.shape[0]))
    p = v.astype(np.float64)[f]
    t = np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])) / 6.0
    return np.bincount(lab, weights=t, minlength=n)


def max_valence(f, nv):
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    return int(np.bincount(e.ravel(), minlength=nv).max())


def cut_and_repair(v, f, deleted):
    """excise + repair; checks every invariant the issue lists and returns (vertices, faces, info)"""
    keep1 = S.excise(f, deleted, v.shape[0])
    f1 = f[keep1]
    nv, nf, info = S.repair(v, f1, LABEL, min_component_faces=1)
    assert closed_oriented(nf)
    assert one_fan_per_vertex(nf, nv.shape[0])
    assert (signed_volumes(nv, nf) > 0).all()
    assert max_valence(nf, nv.shape[0]) <= S.MAX_VALENCE
    # vertices kept are bit-identical; cap vertices come after them
    vm = info['vertex_map']
    old = np.flatnonzero(vm >= 0)
    assert np.array_equal(nv[vm[old]].view(np.uint32), v[old].view(np.uint32))
    assert nv.shape[0] == old.size + info['new_vertices']
    # chi after = chi before - chi(removed) + loops
    kept = np.flatnonzero(keep1)[info['kept_faces']]
    removed = np.ones(f.shape[0], bool)
    removed[kept] = False
    assert S.euler_characteristic(nf) == S.euler_characteristic(f) - S.euler_characteristic(f[removed]) + info['loops']
    return nv, nf, info


def sphere(nsub=3, r=10.0):
    v, f = icosphere(nsub, r)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


# ---- excise / make manifold / cap ---------------------------------------------------------------------------------------------------
def test_a_band_cut_out_of_a_sphere_gives_two_closed_spheres():
    v, f = sphere()
    nv, nf, info = cut_and_repair(v, f, np.flatnonzero(np.abs(v[:, 2]) < 2.0))
    assert info['loops'] == 2
    lab, n = LABEL(nf, S.twins(nf, nv.shape[0]))
    assert n == 2 and S.euler_characteristic(nf) == 4


def test_a_disk_cut_out_of_a_sphere_is_capped_back_to_a_sphere():
    v, f = sphere()
    nv, nf, info = cut_and_repair(v, f, np.flatnonzero(v[:, 2] > 8.0))
    assert info['loops'] == 1 and S.euler_characteristic(nf) == 2


def test_a_short_loop_is_closed_by_one_fan():
    v, f = sphere()
    nv, nf, info = cut_and_repair(v, f, [0])
    assert info['loops'] == 1 and info['loop_sizes'] == [5] and info['new_vertices'] == 1
    assert nf.shape[0] == f.shape[0] and S.euler_characteristic(nf) == 2


def ordered_ring(f, x):
    """the 1-ring of vertex x in fan order"""
    nxt = {}
    for t in f[(f == x).any(1)].tolist():
        k = t.index(x)
        nxt[t[(k + 1) % 3]] = t[(k + 2) % 3]
    ring = [next(iter(nxt))]
    while len(ring) < len(nxt):
        ring.append(nxt[ring[-1]])
    return ring


def test_a_bow_tie_left_by_a_deletion_is_made_manifold():
    v, f = sphere(2)
    x = int(np.flatnonzero(np.bincount(f.ravel()) == 6)[0])
    ring = ordered_ring(f, x)
    a, b = ring[0], ring[3]                                              # two opposite neighbours of x
    f1 = f[S.excise(f, [a, b], v.shape[0])]
    tw = S.twins(f1, v.shape[0])
    corners = np.bincount(f1.ravel(), minlength=v.shape[0])
    links = np.bincount(f1.ravel()[tw >= 0], minlength=v.shape[0])
    assert corners[x] - links[x] == 2                                    # x keeps two fans that meet only at it
    kept, joined = S.make_manifold(f1, v.shape[0])
    assert x in joined.tolist()
    nv, nf, info = cut_and_repair(v, f, [a, b])
    assert info['vertices_joined'] >= 1 and info['vertex_map'][x] == -1
    assert S.euler_characteristic(nf) == 2


def test_a_long_loop_is_capped_by_concentric_rings():
    v, f = sphere(4)
    nv, nf, info = cut_and_repair(v, f, np.flatnonzero(v[:, 2] > 7.5))
    assert info['loops'] == 1 and info['loop_sizes'][0] >= 40            # ~55 edges: three rings and a fan
    assert info['new_vertices'] > 1 + info['loop_sizes'][0] // 2
    assert S.euler_characteristic(nf) == 2
    # every loop vertex gained at most two edges
    loop = [i for i in range(v.shape[0]) if info['vertex_map'][i] >= 0 and v[i, 2] > 6.0]
    nbr = lambda F, x: set(np.unique(F[(F == x).any(1)]).tolist()) - {x}
    vm = info['vertex_map']
    f1 = f[S.excise(f, np.flatnonzero(v[:, 2] > 7.5), v.shape[0])]
    for x in loop:
        if (f1 == x).any() and not (f == x).sum() == (f1 == x).sum():    # a loop vertex (it lost faces)
            before = {vm[y] for y in nbr(f1, x)}
            assert len(nbr(nf, vm[x]) - before) <= 2


def test_small_closed_components_are_dropped_as_dust():
    v, f = sphere(3)
    nv, nf, info = S.repair(v, f[S.excise(f, np.flatnonzero(np.abs(v[:, 2] - 7.0) < 1.5), v.shape[0])], LABEL, min_component_faces=200)
    assert len(info['dust']) == 1 and info['dust'][0][1] < 200
    lab, n = LABEL(nf, S.twins(nf, nv.shape[0]))
    assert n == 1 and closed_oriented(nf)


# ---- the neck guard ---------------------------------------------------------------------------------------------------------------
def regions_of(v, f, cand):
    c = np.zeros(v.shape[0], bool)
    c[cand] = True
    tw = S.twins(f, v.shape[0])
    lab, n = LABEL(f, tw, c[f].any(1).astype(np.uint8))
    return tw, lab, n


def test_region_topology_tells_a_disk_from_a_band():
    v, f = sphere()
    for cand, chi, loops in ((np.abs(v[:, 2]) < 1.5, 0, 2), (v[:, 2] > 8.0, 1, 1)):
        tw, lab, n = regions_of(v, f, np.flatnonzero(cand))
        c, l, simple = S.region_topology(f, tw, lab, n)
        assert n == 1 and c[0] == chi and l[0] == loops and simple[0]


def test_the_guard_accepts_a_band_skips_a_disk_and_rejects_an_annulus_round_a_small_island():
    v, f = sphere()
    z = v[:, 2]
    band = np.flatnonzero(np.abs(z) < 1.5)
    disk = np.flatnonzero(z < -8.0)
    annulus = np.flatnonzero((z > 5.0) & (z < 8.0))                   # the cap above z = 8 is an island of < 200 faces
    tw, lab, n = regions_of(v, f, np.concatenate([band, disk, annulus]))
    assert n == 3
    acc, skips, info = S.guard_regions(f, tw, lab, n, LABEL)
    which = lambda cand: int(lab[np.flatnonzero(np.isin(f, cand).any(1))[0]])
    assert acc == [which(band)]
    assert info['disks'] == 1 and info['examined'] == 2
    assert [r for r, _ in skips] == [which(annulus)] and 'piece of' in skips[0][1]


def test_the_guard_examines_at_most_max_regions():
    v, f = sphere()
    z = v[:, 2]
    tw, lab, n = regions_of(v, f, np.flatnonzero((np.abs(z) < 1.0) | (np.abs(z - 5.0) < 0.8)))
    acc, skips, info = S.guard_regions(f, tw, lab, n, LABEL, max_regions=1)
    assert info['examined'] == 1 and len(acc) + len(skips) == 1


def test_inner_components_decides_by_volume_and_winding():
    samples = [(0, np.arange(4)), (1, np.arange(4, 8)), (2, np.arange(8, 12))]
    vol = np.array([10.0, 1.0, -1.0])

    def winding(qv, qc):
        w = np.zeros((qv.size, 3))
        w[qc == 1, 0] = 1.0                          # component 1 lies inside component 0
        return w
    out = S.inner_components(vol, samples, winding)
    assert [c for c, _ in out] == [1, 2]
    assert 'inverted' in dict(out)[2] and 'inside component 0' in dict(out)[1]


# ---- hooks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['neck_remover', 'edge_cleaner'])
def test_hooks_accept_device_none_and_callables_and_refuse_other_strings(name):
    v, f = sphere(1)
    for ok in ('device', None, lambda *a: None):
        m = MembraneMesh(v, f, **{name: ok})
        assert getattr(m, name) is ok or getattr(m, name) == ok
    with pytest.raises(ValueError):
        MembraneMesh(v, f, **{name: 'gpu'})
    m = MembraneMesh(v, f)
    assert getattr(m, name) is None
    with pytest.raises(ValueError):
        setattr(m, name, 'builtin')
    with pytest.raises(ValueError):
        ShrinkwrapMembrane(**{name: 'gpu'})


def test_shrinkwrap_membrane_passes_the_hooks_to_the_mesh(monkeypatch):
    v, f = sphere(1)

    class Surf(object):
        vertices, faces = v, f
    monkeypatch.setattr(MembraneMesh, 'shrink_wrap', lambda self, *a, **k: None)
    pts = dict(x=np.zeros(10), y=np.zeros(10), z=np.zeros(10))
    mod = ShrinkwrapMembrane(neck_remover='device', edge_cleaner='device')
    mesh = mod.execute(dict(surf=Surf(), filtered_localizations=pts))
    assert mesh.neck_remover == 'device' and mesh.edge_cleaner == 'device' and mesh.neck_guard is True
    mesh = ShrinkwrapMembrane().execute(dict(surf=Surf(), filtered_localizations=pts))
    assert mesh.neck_remover is None and mesh.edge_cleaner is None


def test_no_neck_remover_leaves_the_mesh_alone_and_logs_as_before(monkeypatch):
    v, f = sphere(2)
    m = MembraneMesh(v, f, remesh_frequency=5, neck_first_iter=1)
    monkeypatch.setattr(MembraneMesh, 'neck_vertices', lambda self, lo, hi: np.arange(5))
    plan = MembraneMesh._BlockPlan(m, 10, np.full((4, 3), 10.0), -1)

    class CG(object):
        def refresh_normals(self):
            pass
    m.cg = CG()
    m._block_boundary(np.zeros((4, 3), 'f4'), 5, plan)
    assert m.neck_log == [dict(iteration=5, candidates=5)] and m.edge_log == []
    assert np.array_equal(m.faces, f)


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------------
def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_surgery.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nws_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_binding_matches_its_header():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    assert sorted(S.SYMBOLS) == _declared()
    L = S.load()
    assert L.nws_abi_version() == S.ABI_VERSION == 1
    for k in build.KERNEL_BUDGETS:
        if k.startswith('k_ws_'):
            assert build.kernel_resources(build.OBJ_SURGERY)[k]['scratch'] == 0, k


def test_surgery_binding_checks_its_arguments_before_it_touches_a_gpu():
    """Bad sizes, NULL pointers and indices outside their arrays are refused with NWS_ERR_BADARG -- without a GPU as well; with valid
    arguments and no GPU the context cannot be made (NWS_ERR_HIP): there is no CPU fallback."""
    L = S.load()
    v, f = sphere(1)
    tw = S.twins(f, v.shape[0])
    lab = np.zeros(f.shape[0], np.int32)
    out = np.zeros(f.shape[0], np.int32)
    n = ctypes.c_int32()
    P = lambda a: a.ctypes.data
    BAD = S.NWS_ERR_BADARG
    nf, nv = f.shape[0], v.shape[0]
    assert L.nws_label_faces(None, P(f), None, None, nf, P(out), ctypes.byref(n)) == BAD
    assert L.nws_label_faces(None, P(f), P(tw), None, 0, P(out), ctypes.byref(n)) == BAD
    badtw = tw.copy()
    badtw[5] = 3 * nf
    assert L.nws_label_faces(None, P(f), P(badtw), None, nf, P(out), ctypes.byref(n)) == BAD
    assert L.nws_label_faces(None, P(f), P(tw), None, nf, P(out), ctypes.byref(n)) == BAD          # no ctx
    badf = f.copy()
    badf[0, 0] = nv
    d = np.zeros(1)
    assert L.nws_component_stats(None, P(v), nv, P(badf), P(tw), P(lab), nf, 1, None, P(d), None, None, None) == BAD
    badlab = lab.copy()
    badlab[3] = 1
    assert L.nws_component_stats(None, P(v), nv, P(f), P(tw), P(badlab), nf, 1, None, P(d), None, None, None) == BAD
    q = np.zeros((2, 3), np.float32)
    w = np.zeros(2)
    qc = np.array([0, 1], np.int32)
    assert L.nws_winding(None, P(v), nv, P(f), P(lab), nf, 1, P(q), P(qc), 2, P(w)) == BAD               # query component 1 of 1
    assert L.nws_winding(None, P(v), nv, P(f), P(lab), nf, 1, None, None, 2, P(w)) == BAD
    flag = np.zeros(nv, np.uint8)
    assert L.nws_short_edge_vertices(None, P(v), nv, P(f), nf, -0.5, P(flag), None) == BAD
    assert L.nws_short_edge_vertices(None, P(v), nv, P(f), nf, float('nan'), P(flag), None) == BAD
    assert L.nws_short_edge_vertices(None, P(v), 2, P(f), nf, 0.05, P(flag), None) == BAD
    assert L.nws_create(-1, ctypes.byref(ctypes.c_void_p())) == BAD
    assert L.nws_create(0, None) == BAD
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        assert L.nws_create(0, ctypes.byref(h)) == S.NWS_ERR_HIP and h.value is None
        with pytest.raises(RuntimeError):
            S.SurgeryContext(0)
        with pytest.raises(RuntimeError):
            MembraneMesh(v, f).remove_extra_short_edges()
