"""GPU tests of include/nw_surgery.h and of the surgery that uses it: the labeller against scipy, component statistics and winding numbers
against float64 NumPy restatements, the short-edge selection against np.median, remove_inner_surfaces, remove_necks on synthetic necks,
and recipe fits with neck_remover='device'."""
import numpy as np
import pytest

from ch_shrinkwrap_amd import surgery as S
from ch_shrinkwrap_amd.membrane_mesh import MembraneMesh, ShrinkwrapMembrane
from ch_shrinkwrap_amd.trimesh import icosphere, TriMesh
from ch_shrinkwrap_amd import synth
from ch_shrinkwrap_amd.evaluation import fit_quality

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope='module')
def ctx():
    c = S.SurgeryContext(0)
    yield c
    c.close()


def components(v, f):
    lab, n = S.scipy_label_faces(f, S.twins(f, v.shape[0]))
    return lab, n


def closed_oriented(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    rkey = e[:, 1] * (1 << 32) + e[:, 0]
    return np.unique(key).size == key.size and np.isin(rkey, key).all()


def genera(v, f):
    """genus of every component of a closed mesh"""
    lab, n = components(v, f)
    return [(2 - S.euler_characteristic(f[lab == c])) // 2 for c in range(n)]


def sphere(nsub, r, centre=(0, 0, 0)):
    v, f = icosphere(nsub, r)
    return (v.astype(np.float64) + np.asarray(centre)).astype(F32), np.ascontiguousarray(f, np.int32)


def join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += v.shape[0]
    return np.vstack(vs).astype(F32), np.vstack(fs).astype(np.int32)


# ---- labelling ------------------------------------------------------------------------------------------------------------------------
def tube(n_ring=8, n_seg=20000, r=5.0, step=1.0):
    """an open tube of n_seg segments: a long thin component (its face-graph diameter is ~2 n_seg)"""
    a = 2 * np.pi * np.arange(n_ring) / n_ring
    v = np.stack([np.repeat(np.arange(n_seg + 1) * step, n_ring), np.tile(r * np.cos(a), n_seg + 1), np.tile(r * np.sin(a), n_seg + 1)], 1)
    i = np.arange(n_seg)[:, None] * n_ring
    j = np.arange(n_ring)[None, :]
    p0, p1, p2, p3 = i + j, i + (j + 1) % n_ring, i + n_ring + j, i + n_ring + (j + 1) % n_ring
    f = np.concatenate([np.stack([p0, p1, p3], -1).reshape(-1, 3), np.stack([p0, p3, p2], -1).reshape(-1, 3)])
    return v.astype(F32), f.astype(np.int32)


@pytest.mark.parametrize('case', ['c5', 'c5_masked', 'tube'])
def test_labels_equal_scipy_in_min_face_id_order(ctx, case):
    if case == 'tube':
        v, f = tube()
        mask = None
    else:
        cfg = synth.make_config('c5', scale=0.02)
        v, f = cfg['vertices'], np.ascontiguousarray(cfg['faces'], np.int32)
        mask = None if case == 'c5' else (np.random.default_rng(3).random(f.shape[0]) < 0.7).astype(np.uint8)
    tw = S.twins(f, v.shape[0])
    got, n = ctx.label_faces(f, tw, mask)
    ref, nr = S.scipy_label_faces(f, tw, mask)
    print('%s: %d faces, %d components' % (case, f.shape[0], n))
    assert n == nr and np.array_equal(got, ref)
    if case == 'c5':
        assert n == 8
    if case == 'tube':
        assert n == 1
    again, _ = ctx.label_faces(f, tw, mask)
    assert again.tobytes() == got.tobytes()


# ---- statistics and winding numbers --------------------------------------------------------------------------------------------------
def restated_stats(v, f, tw, lab, n):
    p = v.astype(np.float64)[f]
    cr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area = 0.5 * np.sqrt((cr * cr).sum(1))
    vol = np.einsum('ij,ij->i', p[:, 0], np.cross(p[:, 1], p[:, 2])) / 6.0
    sel = lab >= 0
    bl = np.repeat(lab, 3)
    border = (tw < 0) | (lab[np.maximum(tw, 0) // 3] != bl)
    return dict(faces=np.bincount(lab[sel], minlength=n), area=np.bincount(lab[sel], weights=area[sel], minlength=n),
                volume=np.bincount(lab[sel], weights=vol[sel], minlength=n),
                border=np.bincount(bl[(bl >= 0) & border], minlength=n))


def restated_winding(v, f, q):
    p = v.astype(np.float64)[f][None] - q.astype(np.float64)[:, None, None, :]
    a, b, c = p[:, :, 0], p[:, :, 1], p[:, :, 2]
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    det = np.einsum('qfi,qfi->qf', a, np.cross(b, c))
    dot = lambda x, y: np.einsum('qfi,qfi->qf', x, y)
    den = la * lb * lc + dot(a, b) * lc + dot(a, c) * lb + dot(b, c) * la
    return (np.arctan2(det, den) / (2 * np.pi)).sum(1)


def test_component_stats_match_float64_numpy(ctx):
    v, f = join(sphere(3, 2.0), sphere(2, 1.0, (5, 0, 0)), sphere(2, 1.5, (0, 6, 1)))
    f = f.copy()
    f[-5:] = f[-5:, ::-1]                                        # some faces flipped: borders between labels, a smaller volume
    tw = S.twins(f, v.shape[0])
    lab, n = ctx.label_faces(f, tw)
    got = ctx.component_stats(v, f, tw, lab, n)
    ref = restated_stats(v, f, tw, lab, n)
    for k in ('faces', 'border'):
        assert np.array_equal(got[k], ref[k]), k
    for k in ('area', 'volume'):
        print(k, got[k], np.abs(got[k] - ref[k]).max())
        assert np.abs(got[k] - ref[k]).max() <= 1e-9, k
    for c in range(n):
        vv = v[np.unique(f[lab == c])]
        assert np.array_equal(got['bbox'][c], np.concatenate([vv.min(0), vv.max(0)]))
    again = ctx.component_stats(v, f, tw, lab, n)
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    # on a bigger mesh: relative agreement
    cfg = synth.make_config('c5', scale=0.02)
    v2, f2 = cfg['vertices'], np.ascontiguousarray(cfg['faces'], np.int32)
    tw2 = S.twins(f2, v2.shape[0])
    lab2, n2 = ctx.label_faces(f2, tw2)
    got2, ref2 = ctx.component_stats(v2, f2, tw2, lab2, n2), restated_stats(v2, f2, tw2, lab2, n2)
    assert np.allclose(got2['area'], ref2['area'], rtol=1e-10) and np.allclose(got2['volume'], ref2['volume'], rtol=1e-10)


def test_winding_numbers_match_the_restatement_and_are_one_inside(ctx):
    vs, fs = sphere(3, 2.0)
    vi, fi = sphere(2, 1.0, (6, 0, 0))
    v, f = join((vs, fs), (vi, fi[:, ::-1]))                      # a sphere and an inverted sphere
    tw = S.twins(f, v.shape[0])
    lab, n = ctx.label_faces(f, tw)
    rng = np.random.default_rng(0)
    inside = (rng.normal(size=(64, 3)) * 0.4).astype(F32)
    outside = (rng.normal(size=(64, 3)) * 0.1 + [0, 0, 1.9]).astype(F32) * F32(1.08)
    near_inv = rng.normal(size=(32, 3))
    near_inv = (near_inv / np.linalg.norm(near_inv, axis=1)[:, None] * rng.uniform(0, 0.9, (32, 1)) + [6, 0, 0]).astype(F32)
    q = np.vstack([inside, outside, near_inv, [[0.5, 0.5, 0.5]]]).astype(F32)
    out_of_box = np.linalg.norm(outside.astype(np.float64), axis=1) > 2.0
    w = ctx.winding(v, f, lab, n, q)
    ref0 = restated_winding(vs, fs, q)
    ref1 = restated_winding(vi, fi[:, ::-1], q)
    # pairs outside a component's box are exactly 0
    inbox1 = (q >= vi.min(0)).all(1) & (q <= vi.max(0)).all(1)
    assert (w[~inbox1, 1] == 0).all()
    assert np.abs(w[inbox1, 1] - ref1[inbox1]).max() <= 1e-9
    inbox0 = (q >= vs.min(0)).all(1) & (q <= vs.max(0)).all(1)
    assert np.abs(w[inbox0, 0] - ref0[inbox0]).max() <= 1e-9
    assert np.abs(w[:64, 0] - 1).max() <= 1e-6
    assert np.abs(w[64:128][out_of_box, 0]).max() <= 1e-6
    assert np.abs(w[128:160, 1] + 1).max() <= 1e-6                # inside the inverted sphere: -1
    # the query's own component is skipped
    w2 = ctx.winding(v, f, lab, n, q, np.zeros(q.shape[0], np.int32))
    assert (w2[:, 0] == 0).all() and np.array_equal(w2[:, 1], w[:, 1])
    assert ctx.winding(v, f, lab, n, q).tobytes() == w.tobytes()


# ---- short edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nsub', [3, 4])
def test_short_edge_selection_equals_numpy(ctx, nsub):
    v, f = sphere(nsub, 100.0)
    v = v.copy()
    rng = np.random.default_rng(nsub)
    v += rng.normal(scale=0.3, size=v.shape).astype(F32)
    # planted short edges: a few vertices moved next to a neighbour
    for i in rng.choice(v.shape[0], 12, replace=False):
        j = f[(f == i).any(1)][0]
        j = int(j[j != i][0])
        v[i] = v[j] + F32(0.01) * (v[i] - v[j])
    m = TriMesh(v, f)
    el = m._edge_lengths()
    thr = 0.05 * np.median(el)
    assert thr.dtype == np.float32
    ref = np.zeros(v.shape[0], bool)
    ref[f[:, [1, 2, 0]].ravel()[el < thr]] = True                   # head of half-edge 3f+k = faces[f, (k+1) % 3]
    flags, med = ctx.short_edge_vertices(v, f, 0.05)
    print('%d half-edges: median %r, %d flagged' % (el.size, med, ref.sum()))
    assert med == np.median(el) and med.dtype == np.float32
    assert ref.sum() >= 12 and np.array_equal(flags, ref)
    # an odd count: the middle element
    f_odd = f[:-1]
    el_odd = TriMesh(v, f_odd)._edge_lengths()
    assert el_odd.size % 2 == 1
    assert ctx.short_edge_vertices(v, f_odd, 0.05)[1] == np.median(el_odd)


def test_remove_extra_short_edges_removes_planted_short_edges():
    v, f = sphere(3, 100.0)
    v = v.copy()
    v[7] = v[f[(f == 7).any(1)][0][f[(f == 7).any(1)][0] != 7][0]] + F32(0.01)
    m = MembraneMesh(v, f)
    verts = m.remove_extra_short_edges()
    assert verts.size >= 1 and m.edge_log[-1]['vertices'] == verts.size
    nv, nf = np.asarray(m.vertices), np.asarray(m.faces)
    assert closed_oriented(nf) and genera(nv, nf) == [0]
    assert (TriMesh(nv, nf)._edge_lengths() >= 0.05 * np.median(TriMesh(nv, nf)._edge_lengths())).all()
    nothing = MembraneMesh(*sphere(3, 100.0))
    assert nothing.remove_extra_short_edges().size == 0 and np.array_equal(nothing.faces, sphere(3, 100.0)[1])


# ---- inner surfaces --------------------------------------------------------------------------------------------------------------------
def test_remove_inner_surfaces():
    outer, inner = sphere(3, 100.0), sphere(2, 40.0, (10, 0, 0))
    m = MembraneMesh(*join(outer, inner))
    removed = m.remove_inner_surfaces()
    assert [c for c, _ in removed] == [1] and 'inside component 0' in removed[0][1]
    assert np.array_equal(np.asarray(m.faces), outer[1]) and np.array_equal(np.asarray(m.vertices), outer[0])
    # two disjoint spheres both stay
    two = join(sphere(3, 50.0), sphere(3, 50.0, (200, 0, 0)))
    m = MembraneMesh(*two)
    assert m.remove_inner_surfaces() == [] and np.array_equal(np.asarray(m.faces), two[1])
    # a shell with an inverted cavity: the cavity goes
    m = MembraneMesh(*join(outer, (inner[0], np.ascontiguousarray(inner[1][:, ::-1]))))
    removed = m.remove_inner_surfaces()
    assert [c for c, _ in removed] == [1] and 'inverted' in removed[0][1]
    assert np.asarray(m.faces).shape[0] == outer[1].shape[0]


# ---- remove_necks ---------------------------------------------------------------------------------------------------------------------
def dumbbell_sdf(p, r=60.0, x0=90.0, waist=12.0, k=10.0):
    p = np.asarray(p, 'f8')
    lobes = np.minimum(synth.sdf_sphere(p, r, (-x0, 0, 0)), synth.sdf_sphere(p, r, (x0, 0, 0)))
    return synth.smooth_min(lobes, synth.sdf_capsule(p, (-x0, 0, 0), (x0, 0, 0), waist), k)


def dumbbell(cell=4.0):
    return synth.isosurface_mesh(dumbbell_sdf, (-170, -80, -80), (170, 80, 80), cell)


def test_remove_necks_cuts_an_hourglass_into_two_spheres():
    v, f = dumbbell()
    m = MembraneMesh(v, f, neck_remover='device')
    K = m.curvature_gaussian.copy()
    waist = np.abs(v[:, 0]) < 4.0
    print('dumbbell: %d vertices; K at the waist %.2e .. %.2e, on the lobes' % (v.shape[0], K[waist].min(), K[waist].max()),
          np.percentile(K[np.abs(v[:, 0]) > 60], [1, 50, 99]))
    lo = -1.5e-3
    assert (K[waist] < lo).all()
    verts = m.remove_necks(lo, 1.0)
    assert waist.sum() > 0 and np.isin(np.flatnonzero(waist), verts).all()
    rec = m.neck_log[-1]
    print('neck log:', rec)
    assert rec['cut'] == 1 and rec['components_before'] == 1 and rec['components_after'] == 2
    nv, nf = np.asarray(m.vertices), np.asarray(m.faces)
    assert closed_oriented(nf) and genera(nv, nf) == [0, 0]
    off = np.abs(v[:, 0]) > 45.0
    rows = lambda a: {r.tobytes() for r in np.ascontiguousarray(a, F32)}
    assert rows(v[off]) <= rows(nv)
    # with the device remesher each piece stays a sphere of radius ~60 around its centre
    m2 = MembraneMesh(v, f, neck_remover='device', remesher='device')
    m2.remove_necks(lo, 1.0)
    v2, f2 = np.asarray(m2.vertices), np.asarray(m2.faces)
    lab, n = components(v2, f2)
    assert n == 2 and closed_oriented(f2)
    for c in range(n):
        pv = v2[np.unique(f2[lab == c])].astype(np.float64)
        centre = np.array([np.sign(pv[:, 0].mean()) * 90.0, 0, 0])
        d = np.linalg.norm(pv - centre, axis=1)
        print('piece %d: %d vertices, distance from its centre %.1f .. %.1f' % (c, pv.shape[0], d.min(), d.max()))
        assert np.abs(np.median(d) - 60.0) < 3.0 and d.max() < 70.0


def pinched_torus_sdf(p, R=60.0, r=20.0, pinch=13.0, width=0.25):
    p = np.asarray(p, 'f8')
    th = np.arctan2(p[:, 1], p[:, 0])
    rr = r - pinch * np.exp(-(th / width) ** 2)
    return np.hypot(np.hypot(p[:, 0], p[:, 1]) - R, p[:, 2]) - rr


def test_remove_necks_opens_the_handle_of_a_pinched_torus():
    v, f = synth.isosurface_mesh(pinched_torus_sdf, (-90, -90, -30), (90, 90, 30), 2.5)
    assert genera(v, f) == [1]
    m = MembraneMesh(v, f, neck_remover='device')
    K = m.curvature_gaussian.copy()
    pinch = (np.abs(np.arctan2(v[:, 1], v[:, 0])) < 0.05)
    print('torus: %d vertices; K at the pinch %.2e .. %.2e; elsewhere min %.2e' % (v.shape[0], K[pinch].min(), K[pinch].max(), K[~pinch].min()))
    m.remove_necks(-4e-3, 1.0)
    rec = m.neck_log[-1]
    print('neck log:', rec)
    nv, nf = np.asarray(m.vertices), np.asarray(m.faces)
    assert rec['cut'] >= 1 and closed_oriented(nf)
    assert genera(nv, nf) == [0]


def noisy_sphere(seed=1):
    v, f = sphere(4, 100.0)
    rng = np.random.default_rng(seed)
    v = (v.astype(np.float64) * (1 + rng.normal(scale=0.004, size=(v.shape[0], 1)))).astype(F32)
    return v, f


def test_the_guard_cuts_nothing_on_a_noisy_sphere_and_no_guard_does():
    v, f = noisy_sphere()
    m = MembraneMesh(v, f, neck_remover='device')
    verts = m.remove_necks(-1e-4, 1e-2)
    rec = m.neck_log[-1]
    print('noisy sphere: %d candidates, log %s' % (len(verts), {k: rec[k] for k in ('regions', 'disks', 'examined', 'cut')}))
    assert len(verts) > 100 and rec['cut'] == 0
    assert np.asarray(m.vertices).tobytes() == v.tobytes() and np.asarray(m.faces).tobytes() == f.tobytes()
    m = MembraneMesh(v, f, neck_remover='device', neck_guard=False)
    m.remove_necks(-1e-4, 1e-2)
    nf = np.asarray(m.faces)
    assert nf.shape != f.shape or not np.array_equal(nf, f)
    assert closed_oriented(nf)


# ---- recipe fits ------------------------------------------------------------------------------------------------------------------------
def two_vesicles(seed=4):
    rng = np.random.default_rng(seed)
    pts = []
    for cx in (-200.0, 200.0):
        d = rng.normal(size=(60000, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts.append(d * 150.0 + [cx, 0, 0] + rng.normal(scale=10.0, size=d.shape))
    pts = np.vstack(pts).astype(F32)
    sdf = lambda p: synth.smooth_min(np.minimum(synth.sdf_sphere(p, 175.0, (-200, 0, 0)), synth.sdf_sphere(p, 175.0, (200, 0, 0))),
                                     synth.sdf_capsule(p, (-200, 0, 0), (200, 0, 0), 15.0), 10.0)
    v, f = synth.isosurface_mesh(sdf, (-400, -200, -200), (400, 200, 200), 10.0)
    truth = []
    for cx in (-200.0, 200.0):
        d = rng.normal(size=(40000, 3))
        truth.append(d / np.linalg.norm(d, axis=1)[:, None] * 150.0 + [cx, 0, 0])
    return pts, v, f, np.vstack(truth).astype(F32)


def fit(pts, v, f, minimum_edge_length=5.0, **kw):
    class Surf(object):
        pass
    s = Surf()
    s.vertices, s.faces = v, f
    src = dict(x=pts[:, 0].astype('f8'), y=pts[:, 1].astype('f8'), z=pts[:, 2].astype('f8'),
               error_x=np.full(len(pts), 10.0), error_y=np.full(len(pts), 10.0), error_z=np.full(len(pts), 10.0))
    return ShrinkwrapMembrane(remesher='device', minimum_edge_length=minimum_edge_length, **kw).execute(dict(surf=s, filtered_localizations=src))


def test_recipe_fit_separates_two_vesicles_wrapped_by_one_surface():
    pts, v, f, truth = two_vesicles()
    plain = fit(pts, v, f)
    a = fit(pts, v, f, neck_remover='device')
    b = fit(pts, v, f, neck_remover='device')
    n_plain = components(np.asarray(plain.vertices), np.asarray(plain.faces))[1]
    na, fa = np.asarray(a.vertices), np.asarray(a.faces)
    print('neck log:', [(r['iteration'], r['candidates'], r['regions'], r['disks'], r['cut'], r['components_after']) for r in a.neck_log])
    qa, qp = fit_quality(a, truth), fit_quality(plain, truth)
    print('components: plain %d, with neck removal %d; mse_rms %.2f vs %.2f nm' % (n_plain, components(na, fa)[1], qa['mse_rms'], qp['mse_rms']))
    assert n_plain == 1
    assert components(na, fa)[1] == 2 and closed_oriented(fa)
    assert qa['mse_rms'] < qp['mse_rms']
    assert np.array_equal(na, np.asarray(b.vertices)) and np.array_equal(fa, np.asarray(b.faces))


def test_recipe_fit_on_c4_cuts_nothing_with_the_defaults():
    """examples/fit_network.py 0.2: the recipe's thresholds (-1e-3 / 1e-2, neck_first_iter 9) select thousands of vertices of noise"""
    scale = 0.2
    cfg = synth.make_config('c4', scale=scale)
    pts, v, f = cfg['points'], cfg['vertices'], np.ascontiguousarray(cfg['faces'], np.int32)
    mel = max(5.0, 2.5 / np.sqrt(scale))
    plain = fit(pts, v, f, mel)
    a = fit(pts, v, f, mel, neck_remover='device')
    print('c4 at scale %g: %d vertices; neck log:' % (scale, v.shape[0]),
          [(r['iteration'], r['candidates'], r['regions'], r['disks'], r['examined'], r['cut']) for r in a.neck_log])
    assert max(r['candidates'] for r in a.neck_log) > 1000
    assert all(r['cut'] == 0 for r in a.neck_log)
    assert np.array_equal(np.asarray(a.vertices), np.asarray(plain.vertices)) and np.array_equal(np.asarray(a.faces), np.asarray(plain.faces))
    assert sorted(genera(np.asarray(a.vertices), np.asarray(a.faces))) == sorted(genera(np.asarray(plain.vertices), np.asarray(plain.faces)))


# ---- off the origin and degenerate inputs --------------------------------------------------------------------------------------------
OFFSETS = {'origin': (0.0, 0.0, 0.0), 'offset_4e4': (4e4, 3e4, 1e3), 'offset_2e5': (2e5, -1.5e5, 1e5)}


def _shifted(v, offset):
    return (np.asarray(v, np.float64) + np.asarray(OFFSETS[offset])).astype(F32)


def exact_volumes(v, f, lab, n):
    """6 x signed volume per component as exact integers: every float32 coordinate is an integer multiple of 2^-s"""
    vv = np.asarray(v, np.float64)
    nz = vv[vv != 0]
    s = int(max(0, (23 - (np.frexp(np.abs(nz))[1] - 1)).max())) if nz.size else 0
    q = np.ldexp(vv, s).astype(object)
    q = np.vectorize(int, otypes=[object])(q)
    p0, p1, p2 = q[f[:, 0]], q[f[:, 1]], q[f[:, 2]]
    det = (p0[:, 0] * (p1[:, 1] * p2[:, 2] - p1[:, 2] * p2[:, 1]) + p0[:, 1] * (p1[:, 2] * p2[:, 0] - p1[:, 0] * p2[:, 2])
           + p0[:, 2] * (p1[:, 0] * p2[:, 1] - p1[:, 1] * p2[:, 0]))
    out = []
    for c in range(n):
        out.append(sum(det[lab == c].tolist()))
    return out, 3 * s


def documented_volume_bound(v, f, lab, n):
    """what include/nw_surgery.h promises: n_c 2^-k / 2 (+ |o|_1 n_c 2^-k' / 12) of the fixed point, plus the rounding of the float64 terms"""
    vv = np.asarray(v, np.float64)
    o = ((vv.min(0) + vv.max(0)) * 0.5).astype(F32).astype(np.float64)
    M = max(np.abs(vv - o).max(), 1e-30)
    scale = lambda bound: 2.0 ** np.floor(62.0 - np.log2(bound * max(f.shape[0], 1)))
    sv, sn = scale(M ** 3), scale(12.0 * M * M)
    q = vv[f] - o
    term = (np.abs(q[:, 0]) * (np.abs(q[:, 1, [1, 2, 0]] * q[:, 2, [2, 0, 1]]) + np.abs(q[:, 1, [2, 0, 1]] * q[:, 2, [1, 2, 0]]))).sum(1) / 6.0
    cross = np.abs(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])).sum(1)
    f64 = 8 * np.finfo(np.float64).eps * (term + np.abs(o).sum() * cross / 6.0)
    nc = np.bincount(lab[lab >= 0], minlength=n)
    return nc * (0.5 / sv + np.abs(o).sum() * 0.5 / sn / 6.0) + np.bincount(lab[lab >= 0], weights=f64[lab >= 0], minlength=n)


def shell_scene():
    """a small positively oriented shell outside a large mesh, a small inverted shell inside it, and the large mesh"""
    big = sphere(5, 500.0)
    small = sphere(1, 2.0, (520.0, 0.0, 0.0))
    cavity = sphere(1, 2.0, (100.0, 0.0, 0.0))
    return join(big, small, (cavity[0], np.ascontiguousarray(cavity[1][:, ::-1])))


@pytest.mark.parametrize('offset', list(OFFSETS))
def test_component_stats_off_the_origin_against_exact_arithmetic(ctx, offset):
    v0, f = shell_scene()
    v = _shifted(v0, offset)
    tw = S.twins(f, v.shape[0])
    lab, n = ctx.label_faces(f, tw)
    assert n == 3
    got = ctx.component_stats(v, f, tw, lab, n)
    ref = restated_stats(v, f, tw, lab, n)
    p = v.astype(np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    ref_area = np.bincount(lab, weights=area, minlength=n)
    six, e = exact_volumes(v, f, lab, n)
    ref_vol = np.array([float(x) / 6.0 / 2.0 ** e for x in six])   # (the quotient rounded once)
    bound = documented_volume_bound(v, f, lab, n)
    err = np.abs(got['volume'] - ref_vol)
    print('%s: volumes %s; error %s; documented bound %s; area error %s'
          % (offset, got['volume'], err, bound, np.abs(got['area'] - ref_area)))
    assert np.array_equal(got['faces'], ref['faces']) and np.array_equal(got['border'], ref['border'])
    assert (err <= bound).all()
    # area: n_c 2^-k / 2 with 2^k = 2^62 / (n_faces 6 M^2), plus float64 rounding of the terms
    vv = v.astype(np.float64)
    M = np.abs(vv - ((vv.min(0) + vv.max(0)) * 0.5).astype(F32)).max()
    s_area = 2.0 ** np.floor(62.0 - np.log2(6.0 * M * M * f.shape[0]))
    area_bound = np.bincount(lab, minlength=n) * 0.5 / s_area + 1e-14 * ref_area
    print('  area error %s, documented bound %s' % (np.abs(got['area'] - ref_area), area_bound))
    assert (np.abs(got['area'] - ref_area) <= area_bound).all()
    assert got['volume'][1] > 0 > got['volume'][2]                  # the signs remove_inner_surfaces decides on
    for c in range(n):
        vv = v[np.unique(f[lab == c])]
        assert np.array_equal(got['bbox'][c], np.concatenate([vv.min(0), vv.max(0)]))


def test_remove_inner_surfaces_decides_the_same_off_the_origin():
    v0, f = shell_scene()
    decided = {}
    for offset in OFFSETS:
        m = MembraneMesh(_shifted(v0, offset), f)
        decided[offset] = (m.remove_inner_surfaces(), np.asarray(m.faces).copy())
    print({k: r for k, (r, _) in decided.items()})
    assert [c for c, _ in decided['origin'][0]] == [2] and 'inverted' in decided['origin'][0][0][1]
    kind = lambda removed: [(c, 'inverted' in r, 'inside' in r) for c, r in removed]
    for offset in OFFSETS:
        assert kind(decided[offset][0]) == kind(decided['origin'][0]), offset
        assert np.array_equal(decided[offset][1], decided['origin'][1]), offset


def _short_edge_reference(v, f, threshold):
    el = TriMesh(v, f)._edge_lengths()
    med = np.median(el)
    thr = F32(threshold) * med
    ref = np.zeros(v.shape[0], bool)
    ref[f[:, [1, 2, 0]].ravel()[el < thr]] = True
    return ref, med


def _grid(n=6, h=2.0):
    xx, yy = np.meshgrid(np.arange(n, dtype='f4') * F32(h), np.arange(n, dtype='f4') * F32(h), indexing='ij')
    v = np.stack([xx.ravel(), yy.ravel(), np.zeros(n * n, 'f4')], 1)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 0).astype(np.int32)


def _short_edge_case(case):
    if case in OFFSETS:
        v, f = sphere(3, 100.0)
        v = v + np.random.default_rng(5).normal(scale=0.3, size=v.shape).astype(F32)
        return _shifted(v, case), f
    if case == 'one_face':
        return np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], F32), np.array([[0, 1, 2]], np.int32)
    if case == 'two_faces':
        return np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [3, 5, 1]], F32), np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    if case == 'ties':
        return _grid()                                               # two lengths, each many times: the median is a tie
    if case == 'zero_length':
        v, f = _grid()
        v = v.copy()
        v[7] = v[8]                                                  # duplicated positions: edges of length exactly 0
        v[20] = v[14]
        return v, f
    raise KeyError(case)


@pytest.mark.parametrize('case', list(OFFSETS) + ['one_face', 'two_faces', 'ties', 'zero_length'])
def test_short_edge_selection_equals_numpy_on_edge_cases(ctx, case):
    v, f = _short_edge_case(case)
    for threshold in (0.05, 0.0, 0.75, 1e30):
        ref, med = _short_edge_reference(v, f, threshold)
        flags, got_med = ctx.short_edge_vertices(v, f, threshold)
        assert got_med == med and got_med.dtype == np.float32, (case, threshold)
        assert np.array_equal(flags, ref), (case, threshold)
        if threshold == 0.0:
            assert not flags.any()
        if threshold == 1e30:
            assert np.array_equal(flags, np.isin(np.arange(v.shape[0]), f))     # every head of a half-edge
    if case == 'zero_length':
        assert _short_edge_reference(v, f, 0.05)[0][[7, 8, 14, 20]].sum() >= 2


@pytest.mark.parametrize('case', ['single_face', 'empty_mask', 'twins_excluded'])
def test_labels_equal_scipy_on_degenerate_masks(ctx, case):
    if case == 'single_face':
        f = np.array([[0, 1, 2]], np.int32)
        tw, mask = S.twins(f, 3), None
    else:
        v, f = sphere(2, 10.0)
        tw = S.twins(f, v.shape[0])
        if case == 'empty_mask':
            mask = np.zeros(f.shape[0], np.uint8)
        else:
            # include a face set, exclude every twin face of it (those not themselves included): the included faces touch only excluded ones
            inc = np.zeros(f.shape[0], bool)
            for g in range(f.shape[0]):
                if not inc[np.maximum(tw[3 * g: 3 * g + 3], 0) // 3].any():
                    inc[g] = True
            mask = inc.astype(np.uint8)
    got, n = ctx.label_faces(f, tw, mask)
    ref, nr = S.scipy_label_faces(f, tw, mask)
    assert n == nr and np.array_equal(got, ref)
    if case == 'single_face':
        assert n == 1 and got.tolist() == [0]
    if case == 'empty_mask':
        assert n == 0 and (got == -1).all()
    if case == 'twins_excluded':
        assert n == int(mask.sum()) > 1                               # every included face is a component of its own
