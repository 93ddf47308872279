"""CPU test: the NumPy restatement of the DBSCAN query (tests/dbscan_ref.py) against scikit-learn where the two definitions agree, against
closed forms on integer lattices where d2 is an exact integer, under permutation of the cloud, on the two-vesicle scene that the device
test uses end to end, and against three one-line mutations of itself."""
import functools

import numpy as np
import pytest

import dbscan_ref as R


def random_cloud(n, seed, box=60.0):
    return np.random.default_rng(seed).uniform(0.0, box, (n, 3)).astype(np.float32)


def clumps(seed):
    """three gaussian clumps and a uniform background"""
    rng = np.random.default_rng(seed)
    parts = [rng.normal(c, 3.0, (150, 3)) for c in ((0, 0, 0), (30, 5, 0), (10, 40, 20))] + [rng.uniform(-20, 60, (200, 3))]
    return np.concatenate(parts).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(seed=0):
    P, src = R.two_vesicles(seed)
    return P, src, R.dbscan(P, 25.0, 10)


# ---- scikit-learn ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,eps,min_points', [('random', 6.0, 4), ('clumps', 4.0, 8), ('clumps', 7.0, 5), ('vesicles', 25.0, 10)])
def test_against_scikit_learn(name, eps, min_points):
    cluster = pytest.importorskip('sklearn.cluster')
    P = {'random': lambda: random_cloud(700, 1), 'clumps': lambda: clumps(2), 'vesicles': lambda: scene()[0]}[name]()
    # scikit-learn compares a rooted distance with eps: no pair may sit at the threshold
    assert R.min_margin(P, eps) > 1e-9
    ref = R.dbscan(P, eps, min_points) if name != 'vesicles' else scene()[2]
    sk = cluster.DBSCAN(eps=eps, min_samples=min_points, algorithm='brute').fit(P.astype(np.float64))
    core = np.zeros(len(P), bool)
    core[sk.core_sample_indices_] = True
    assert np.array_equal(np.nonzero(ref['core'])[0], np.sort(sk.core_sample_indices_))
    assert R.partition(ref['labels'], core) == R.partition(sk.labels_, core)          # the core points' partition, up to renumbering
    assert np.array_equal(ref['labels'] < 0, sk.labels_ < 0)                           # the noise set
    P64 = P.astype(np.float64)
    border = np.nonzero(~core & (ref['labels'] >= 0))[0]
    assert len(border) > 0
    for i in border:                                              # a border point's label is the label of some core point near it
        near_core = np.nonzero((R.d2_rows(P64, np.array([i]))[0] <= eps * eps) & core)[0]
        assert sk.labels_[i] in set(sk.labels_[near_core]) and ref['labels'][i] in set(ref['labels'][near_core])
        assert ref['anchor'][i] in near_core


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
def test_the_seven_cubed_lattice():
    P = R.lattice(7)
    r = R.dbscan(P, 1.0, 7, count_cap=100)
    on_edge = ((P == 0) | (P == 6)).sum(1)                        # how many coordinates sit on the boundary
    assert np.array_equal(r['n_eps'], 7 - on_edge)                # interior 7, face 6, edge 5, corner 4
    assert np.array_equal(r['count'], r['n_eps']) and np.array_equal(r['core'], on_edge == 0)
    assert r['n_clusters'] == 1 and r['n_core'][0] == 125 and r['sizes'][0] == 125 + 150
    # the border: the points with one coordinate on the boundary and the other two strictly inside (the neighbour across is interior)
    inner = ((P >= 2) & (P <= 4)).sum(1)
    border = (on_edge == 1) & (((P >= 1) & (P <= 5)).sum(1) == 2)
    assert border.sum() == 150 and np.array_equal(~r['core'] & (r['labels'] == 0), border) and inner.max() == 3
    assert np.array_equal(r['labels'] < 0, ~r['core'] & ~border)
    assert r['info'] == dict(n_core=125, n_border=150, n_noise=343 - 275, n_clusters=1)
    assert r['first'][0] == 1 + 7 + 49
    m = r['labels'] == 0
    assert r['bbox'][0].tolist() == P[m].min(0).tolist() + P[m].max(0).tolist()


def test_a_chain_at_exactly_eps_and_one_ulp_beside_it():
    P = R.chain(40, 1.0)
    r = R.dbscan(P, 1.0, 2)
    assert r['n_clusters'] == 1 and r['core'].all() and (r['labels'] == 0).all() and r['sizes'][0] == 40
    assert np.array_equal(r['count'], np.full(40, 2)) and np.array_equal(R.dbscan(P, 1.0, 2, 10)['count'], [2] + [3] * 38 + [2])
    wide = R.dbscan(R.chain(3, 1.0, wider=True), 1.0, 2)                                # the same chain one float32 ulp wider
    assert wide['n_clusters'] == 0 and (wide['labels'] == -1).all() and not wide['core'].any() and np.array_equal(wide['count'], [1, 1, 1])
    below = R.dbscan(P, np.nextafter(1.0, 0.0), 2)                                      # eps one float64 ulp below the step
    assert below['n_clusters'] == 0 and (below['labels'] == -1).all() and below['info']['n_noise'] == 40


def test_duplicates_count():
    P = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    r = R.dbscan(P, 0.5, 300, count_cap=1000)
    assert (r['n_eps'] == 300).all() and r['core'].all() and r['n_clusters'] == 1 and r['first'][0] == 0
    assert not R.dbscan(P, 0.5, 301)['core'].any()


def test_a_bridge_joins_nothing_and_goes_to_the_nearer_core():
    P = R.bridge()
    b = len(P) - 1
    r = R.dbscan(P, 2.0, 10)
    # at eps = 2 a point of a 3^3 lattice has at least 11 points near it (a corner), the bridge has 3: itself and one core on each side
    assert r['n_eps'][b] == 3 and not r['core'][b] and r['core'][:b].all()
    assert r['n_clusters'] == 2 and R.partition(r['labels'], r['core']) == {frozenset(range(27)), frozenset(range(27, 54))}
    i0, i1 = 1 * 9 + 1 * 3 + 2, 27 + 1 * 9 + 1 * 3 + 0           # (2, 1, 1) and (6, 1, 1)
    assert P[i0].tolist() == [2, 1, 1] and P[i1].tolist() == [6, 1, 1]
    assert r['anchor'][b] == i0 and r['labels'][b] == 0          # an exact tie: the smaller index
    Q = P.copy()
    Q[b, 0] = 4.25                                               # nearer to the second lattice: only its core is near
    assert R.dbscan(Q, 2.0, 10)['anchor'][b] == i1
    Q = np.concatenate([P[27:54], P[:27], P[b:]])                # the lattices swapped: the tie goes to the other one
    r2 = R.dbscan(Q, 2.0, 10)
    assert r2['anchor'][b] == 1 * 9 + 1 * 3 + 0 and Q[r2['anchor'][b]].tolist() == [6, 1, 1]
    # a nearer core with a larger index wins over a farther one with a smaller index
    Q = P.copy()
    Q[b] = [4.0, 1.0, 1.0]
    Q[i0, 0] = 2.0
    Q[i1, 0] = 5.5
    r3 = R.dbscan(Q, 2.0, 10)
    assert r3['core'][i0] and r3['core'][i1] and not r3['core'][b] and r3['anchor'][b] == i1


def test_count_cap_below_at_and_above():
    P = R.lattice(7)
    full = R.dbscan(P, 1.0, 3, count_cap=1000)['n_eps']
    for cap in (3, 5, 7, 8, 343, 1 << 30):
        r = R.dbscan(P, 1.0, 3, count_cap=cap)
        assert np.array_equal(r['count'], np.minimum(full, cap)) and r['core'].all()


# ---- invariance -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [3, 4])
def test_a_permuted_cloud_gives_the_permuted_answer(seed):
    P = clumps(seed)
    perm = np.random.default_rng(seed + 10).permutation(len(P))
    a, b = R.dbscan(P, 5.0, 6, 50), R.dbscan(P[perm], 5.0, 6, 50)
    assert np.array_equal(b['count'], a['count'][perm]) and np.array_equal(b['core'], a['core'][perm])
    back = np.argsort(perm)                                       # original index -> position in the permuted cloud
    assert R.partition(a['labels'], a['core']) == set(frozenset(perm[list(s)]) for s in R.partition(b['labels'], b['core']))
    assert np.array_equal(a['labels'] < 0, (b['labels'] < 0)[back])
    # a border point's anchor is as near in both (only an exact tie may pick another index)
    for r_, Q in ((a, P), (b, P[perm])):
        for c in range(r_['n_clusters']):                         # numbering follows the smallest index
            assert r_['first'][c] == np.nonzero((r_['labels'] == c) & r_['core'])[0].min()
        assert np.all(np.diff(r_['first']) > 0)
    ia = np.nonzero(~a['core'] & (a['anchor'] >= 0))[0]
    P64 = P.astype(np.float64)
    da = ((P64[ia] - P64[a['anchor'][ia]]) ** 2).sum(1)
    db = ((P64[ia] - P64[perm[b['anchor'][back[ia]]]]) ** 2).sum(1)
    assert np.array_equal(da, db)


# ---- the scene used end to end --------------------------------------------------------------------------------------------------------
def test_the_two_vesicle_scene():
    P, src, r = scene()
    assert len(P) == 3300 and r['n_clusters'] == 2
    for c in range(2):
        spheres = set(src[(r['labels'] == c) & (src < 2)].tolist())
        assert len(spheres) == 1                                  # one sphere only, apart from background
    assert ((r['labels'] < 0) & (src < 2)).sum() <= 2
    assert 1500 <= r['sizes'].min() and r['sizes'].max() <= 1600 and r['info']['n_core'] >= 2900


# ---- mutations ------------------------------------------------------------------------------------------------------------------------
def test_three_mutations_turn_an_assertion_red():
    P = R.chain(40, 1.0)
    assert R.dbscan(P, 1.0, 2)['n_clusters'] == 1 and R.dbscan(P, 1.0, 2, mutate='strict')['n_clusters'] == 0             # < for <=
    Q = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    assert R.dbscan(Q, 0.5, 300)['core'].all() and not R.dbscan(Q, 0.5, 300, mutate='no_self')['core'].any()              # the self point
    B = R.bridge()
    b = len(B) - 1
    B[b, 0] = 4.3                                                # 1.7 from (6, 1, 1), whose index is the larger one,
    B[1 * 9 + 1 * 3 + 2, 0] = 2.5                                # and 1.8 from what was (2, 1, 1)
    good, bad = R.dbscan(B, 2.0, 10), R.dbscan(B, 2.0, 10, mutate='border_index')
    assert not good['core'][b] and good['anchor'][b] == 27 + 1 * 9 + 1 * 3 + 0 and bad['anchor'][b] == 1 * 9 + 1 * 3 + 2  # nearest, not smallest
