"""
The NumPy restatement of the point-to-mesh distance (tests/mesh_distance_ref.py) against ground truth that does not come from it: a
box's closed-form signed distance, an apex whose nearest faces look away from the query, a concave edge and vertex, a sphere.  The
compiled core (tests/test_distance_core_cpu.py) and the device (tests/test_hip_distance.py) are then compared with the restatement
bit for bit, so what is settled here holds for them.
"""
import numpy as np

import mesh_distance_ref as R
from ch_shrinkwrap_amd.trimesh import icosphere


def test_cube_equals_the_box_distance():
    v, f = R.cube()
    tw = R.twins(f)
    assert (tw >= 0).all()
    p = np.random.default_rng(0).uniform(-2.5, 2.5, (2000, 3))
    out = R.distance(p, v, f, tw)
    truth = R.box_sdf(p)
    err = np.abs(out['dist'] - truth).max()
    wrong = int((np.sign(out['dist']) != np.sign(truth)).sum())
    print('cube: max error %.3g, %d wrong signs, %d inside' % (err, wrong, int((truth < 0).sum())))
    assert (truth < 0).sum() > 50 and (truth > 0).sum() > 1000
    assert err <= 1e-12 and wrong == 0


def test_spike_needs_the_pseudonormal():
    """400 queries level with a sharp apex: all are nearest to the apex and all are outside; the nearest face's own normal says
    'inside' for a good share of them, the angle-weighted pseudonormal for none."""
    v, f = R.spike()
    tw = R.twins(f)
    q = R.spike_queries(400)
    out = R.distance(q, v, f, tw)
    # nearest to the apex, whichever corner of the face it is -- or, within 48 degrees of a base corner's direction (3 r cos > 2 at
    # r = 1), to a point of the edge that runs down to that corner, at most 1 / 101 of the way along
    apex = out['feature'] == 4 + np.argmax(f[out['face']] == 3, axis=1)
    assert apex.sum() > 60 and (out['feature'][~apex] >= 1).all() and (out['feature'][~apex] <= 3).all()
    assert np.array_equal(out['closest'][apex], np.tile([0.0, 0.0, 10.0], (apex.sum(), 1)))
    assert np.abs(out['closest'] - [0.0, 0.0, 10.0]).max() <= 0.1
    assert (out['dist'] > 0).all()
    assert np.allclose(out['dist'][apex], np.sqrt(9.0 + 0.2 ** 2), rtol=1e-14) and out['dist'].max() <= np.sqrt(9.04) * (1 + 1e-14)
    vd = v.astype(np.float64)
    fn = np.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]])
    shortcut = ((q - out['closest']) * fn[out['face']]).sum(1) < 0
    print('spike: the closest face\'s own normal gives %d of %d negative' % (int(shortcut.sum()), len(q)))
    assert shortcut.sum() == 114                               # the shortcut this test is there to catch does fail here (the input is fixed)


def test_l_prism_signs_beside_the_concave_edge_and_vertex():
    v, f = R.l_prism()
    tw = R.twins(f)
    assert (tw >= 0).all() and len(f) == 20
    vd = v.astype(np.float64)
    assert np.isclose((vd[f[:, 0]] * np.cross(vd[f[:, 1]], vd[f[:, 2]])).sum() / 6.0, 3.0)        # closed, outward, volume 3
    # inside, nearest to the concave edge x = y = 1: the point is nearer to it than to any wall
    t = np.linspace(0.05, 0.3, 6)
    inner = np.stack([1.0 - t, 1.0 - t * 0.8, np.full(6, 0.5)], 1)
    # outside, in the notch and above the top, beside the concave vertex (1, 1, 1): nearest to one of the two top edges that meet in it
    # (a saddle vertex is nearest to no point off the line above it) -- and on that line
    outer = np.concatenate([np.stack([1.0 + t, 1.0 + 0.7 * t, 1.0 + 0.5 * t], 1), np.stack([np.ones(6), np.ones(6), 1.0 + t], 1)])
    # inside, just under the concave vertex, and outside in the notch beside the edge
    mixed = np.array([[0.95, 0.97, 0.96], [1.1, 1.2, 0.5], [1.02, 1.01, 0.99]])
    oi, oo, om = (R.distance(p, v, f, tw) for p in (inner, outer, mixed))
    assert ((oi['feature'] >= 1) & (oi['feature'] <= 3)).all() and np.allclose(oi['closest'][:, :2], 1.0)
    assert (oi['dist'] < 0).all()
    assert (oo['feature'][:6] >= 1).all() and (oo['feature'][:6] <= 3).all() and np.array_equal(oo['closest'][6:], np.ones((6, 3)))
    assert np.abs(oo["closest"] - 1.0).max() <= 0.31 and (oo['dist'] > 0).all()
    assert ((om['dist'] < 0) == R.l_prism_inside(mixed)).all()
    # and everywhere: the sign is the solid's, and outside the distance is the smaller of the two boxes'
    p = np.random.default_rng(1).uniform(-0.5, 2.5, (1500, 3)) * [1, 1, 0.8] - [0, 0, 0.4]
    out = R.distance(p, v, f, tw)
    inside = R.l_prism_inside(p)
    assert inside.sum() > 100 and (~inside).sum() > 100
    assert ((out['dist'] < 0) == inside).all()
    boxes = np.minimum(R.box_sdf(p - [1.0, 0.5, 0.5] , np.array([1.0, 0.5, 0.5])), R.box_sdf(p - [0.5, 1.0, 0.5], np.array([0.5, 1.0, 0.5])))
    assert np.abs(out['dist'] - boxes)[~inside].max() <= 1e-12


def test_icosphere_sign_is_the_spheres():
    radius = 50.0
    v, f = icosphere(2, radius)
    tw = R.twins(f)
    vd = v.astype(np.float64)
    n = np.cross(vd[f[:, 1]] - vd[f[:, 0]], vd[f[:, 2]] - vd[f[:, 0]])
    inscribed = ((vd[f[:, 0]] * n).sum(1) / np.linalg.norm(n, axis=1)).min()
    sagitta = radius - inscribed
    rng = np.random.default_rng(2)
    d = rng.normal(size=(1500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = rng.uniform(0.0, 2.0 * radius, 1500)
    p = d * r[:, None]
    out = R.distance(p, v, f, tw)
    clear = np.abs(r - radius) > sagitta * (1 + 1e-6)
    assert clear.sum() > 1000 and (r < radius)[clear].sum() > 300
    assert (np.sign(out['dist'][clear]) == np.sign(r - radius)[clear]).all()
    # and the distance is the sphere's to within the sagitta
    assert np.abs(np.abs(out['dist']) - np.abs(r - radius)).max() <= sagitta * (1 + 1e-6)


def test_inputs_reach_what_they_are_named_for():
    # all seven feature codes, each where it is meant to be
    v, f, q, code = R.triangle_region_queries()
    tw = R.twins(f)
    assert (tw == -1).all()
    taken = {}
    out = R.distance(q, v, f, tw, taken=taken)
    assert (out['feature'] == code).all()
    assert sorted(set(out['feature'].tolist())) == [0, 1, 2, 3, 4, 5, 6]
    assert (out['d2'][-6:] == 0).all()                                                  # on the edges and at the vertices
    assert not np.signbit(out['dist'][out['d2'] == 0]).any()                            # a distance of 0 is +0.0
    assert taken.get('border_edge', 0) >= 3 and taken.get('border', 0) >= 3 and 'closed' not in taken
    # the border branch of the fan walk, both ways: a rim vertex of the open disk whose closest face is in the middle of its fan
    v, f = R.disk()
    tw = R.twins(f)
    a = 2.0 * np.pi * np.arange(8) / 8
    rim = np.stack([2.5 * np.cos(a), 2.5 * np.sin(a), np.full(8, 0.4)], 1)
    taken = {}
    out = R.distance(rim, v, f, tw, taken=taken)
    assert (out['feature'] >= 4).all() and taken.get('border', 0) == 8 and 'closed' not in taken
    assert (out['dist'] > 0).all()
    N = out['normal']
    assert np.allclose(N[:, :2], 0.0) and (N[:, 2] > 0).all()
    # every rim vertex has three faces: the sum of their angles at it is below pi, and all three were visited whichever face came first
    assert len(set(np.round(N[:, 2], 5).tolist())) == 1
    below = R.distance(rim * [1, 1, -1], v, f, tw)
    assert (below['dist'] < 0).all() and np.array_equal(np.abs(below['dist']), out['dist'])
    # closed fans and zero-area faces
    taken = {}
    v, f = R.cube()
    R.distance(np.array([[2.0, 2.0, 2.0], [-3.0, 2.0, -2.0]]), v, f, R.twins(f), taken=taken)
    assert taken.get('closed', 0) == 2
    v, f = R.degenerate_faces()
    out = R.distance(np.array([[2.5, 0.5, 0.0], [4.0, -1.0, 0.0], [2.0, 2.0, 2.5], [0.2, 0.2, 1.0]]), v, f)
    assert out['face'].tolist() == [1, 2, 3, 0] and out['feature'].tolist()[:3] == [1 + 1, 1 + 1, 4] and out['feature'][3] == 0


def test_a_capped_fan_sets_the_flag():
    """a vertex with more than FAN_CAP faces around it"""
    n = R.FAN_CAP + 40
    a = 2.0 * np.pi * np.arange(n) / n
    v = np.array([[0.0, 0.0, 1.0]] + [[np.cos(t), np.sin(t), 0.0] for t in a], np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    taken = {}
    out = R.distance(np.array([[0.0, 0.0, 3.0], [2.0, 0.0, 0.0]]), v, f, R.twins(f), taken=taken)
    assert out['feature'][0] & R.CAPPED and (out['feature'][0] & 7) == 4 and taken.get('capped') == 1
    assert not out['feature'][1] & R.CAPPED and out['dist'][0] == 2.0
