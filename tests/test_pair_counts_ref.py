"""
The NumPy restatement of the pair-count query (tests/pair_counts_ref.py) tied to ground truth, without a GPU: closed forms on the integer
lattice and on duplicates, scipy's cKDTree.count_neighbors on random and clustered clouds, the identities the definition implies, the
normalisation of Ripley's K against the known distance distribution of a uniform cube, and three one-line mutations that are caught.
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import pair_counts_ref as R


def tree_counts(A, B, radii):
    """#{ (i, j) : |a_i - b_j| <= r } for every r, by scipy, on the float64 images of the float32 clouds"""
    return np.asarray(cKDTree(R.cloud32(A).astype(np.float64)).count_neighbors(cKDTree(R.cloud32(B).astype(np.float64)), np.asarray(radii, np.float64)), np.int64)


def test_the_integer_lattice_in_closed_form():
    """7^3 lattice: 2 * 3 * 6 * 49 = 1764 ordered pairs at distance 1, 2 * 3 * 36 * 7 * 2 = 3024 at sqrt(2) (d2 = 2 <= 2.25), then
    d2 = 3 (4 * 216 * 2 = 1728) and d2 = 4 (2 * 3 * 5 * 49 = 1470) up to r = 2: 3198.  A pair at exactly an edge belongs to the bin the
    edge closes; with the first edge one ulp below 1 the 1764 move up."""
    P = R.lattice(7)
    r = R.pair_counts(P, [1.0, 1.5, 2.0])
    assert r['hist'].tolist() == [1764, 3024, 3198] and r['cumulative'].tolist() == [1764, 4788, 7986]
    assert (tree_counts(P, P, [1.0, 1.5, 2.0]) - 343).tolist() == r['cumulative'].tolist()              # scipy counts the 343 self pairs
    below = R.pair_counts(P, [float(np.nextafter(1.0, 0.0)), 1.5, 2.0])
    assert below['hist'].tolist() == [0, 4788, 3198]
    corner, centre = 0, 3 * 49 + 3 * 7 + 3
    assert r['local'][corner].tolist() == [3, 3, 1 + 3] and r['local'][centre].tolist() == [6, 12, 8 + 6]
    assert np.array_equal(r['local'].sum(0, dtype=np.uint64), r['hist'])


def test_duplicates():
    dup = np.tile(np.array([[3.0, -2.0, 7.5]], np.float32), (300, 1))
    r = R.pair_counts(dup, [0.0, 1.0])
    assert r['hist'].tolist() == [300 * 299, 0] and (r['local'][:, 0] == 299).all()
    two = np.concatenate([dup[:5], dup[:3] + np.float32(1.0)])
    r = R.pair_counts(two, [0.0, 2.0])
    assert r['hist'].tolist() == [5 * 4 + 3 * 2, 2 * 15]


@pytest.mark.parametrize('name', ['random', 'clustered', 'cross'])
def test_equal_to_ckdtree_count_neighbors(name):
    rng = np.random.default_rng(3)
    radii = [0.7, 1.9, 3.3, 5.1, 8.7]
    if name == 'random':
        A, B = rng.uniform(0.0, 40.0, (1500, 3)).astype(np.float32), None
    elif name == 'clustered':
        A, B = R.clustered(1500, 4), None
    else:
        A, B = rng.uniform(-30.0, 90.0, (400, 3)).astype(np.float32), R.clustered(1200, 5)
    assert R.min_edge_margin(A, radii, B) > 1e-9                 # scipy roots or squares in its own way: no pair may sit on an edge
    r = R.pair_counts(A, radii, other=B)
    want = tree_counts(A, A if B is None else B, radii) - (len(A) if B is None else 0)
    assert r['cumulative'].tolist() == want.tolist()
    assert np.array_equal(np.diff(np.concatenate([[0], want])), r['hist'].astype(np.int64))


def test_identities():
    rng = np.random.default_rng(6)
    A = R.clustered(700, 7)
    radii = [0.0, 1.0, 2.5, 4.0, 9.0]
    auto = R.pair_counts(A, radii)
    perm = rng.permutation(len(A))                                # a permutation: hist is equal, local is permuted
    shuf = R.pair_counts(A[perm], radii)
    assert np.array_equal(shuf['hist'], auto['hist']) and np.array_equal(shuf['local'], auto['local'][perm])
    cross = R.pair_counts(A, radii, other=A)                      # auto against cross: the n self pairs come back, in bin 0
    extra = np.zeros(len(radii), np.uint64)
    extra[0] = len(A)
    assert np.array_equal(cross['hist'], auto['hist'] + extra)
    assert np.array_equal(cross['local'][:, 1:], auto['local'][:, 1:]) and np.array_equal(cross['local'][:, 0], auto['local'][:, 0] + 1)
    B = rng.uniform(-10.0, 60.0, (300, 3)).astype(np.float32)     # cross mode is symmetric in its total (d2 is bit-symmetric)
    ab, ba = R.pair_counts(A, radii, other=B), R.pair_counts(B, radii, other=A)
    assert np.array_equal(ab['hist'], ba['hist']) and ab['local'].shape == (700, 5) and ba['local'].shape == (300, 5)
    assert (auto['hist'] % np.uint64(2) == 0).all()               # every unordered pair twice
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [-1.0], [np.nan], list(np.arange(65.0)), [1e-200, 2e-200]):
        with pytest.raises(ValueError):
            R.pair_counts(A[:10], bad)


def ripley_host(P, radii, V):
    """pairs.ripley's arithmetic on the restatement's integers (the device is not needed to check the formula)"""
    c = R.pair_counts(P, radii)
    n = len(P)
    K = V * c['cumulative'].astype(np.float64) / (n * (n - 1.0))
    L = np.cbrt(3.0 * K / (4.0 * np.pi))
    return K, L, L - np.asarray(radii), c


def test_ripley_on_a_uniform_cube_and_on_a_clustered_scene():
    """Uniform points in a cube of side S: the distance of two of them has the density 4 pi t^2 - 6 pi t^3 + 8 t^4 - t^5 (t = r / S <= 1;
    the classical cube line picking), so without edge correction E[K(r)] = S^3 (4/3 pi t^3 - 3/2 pi t^4 + 8/5 t^5 - 1/6 t^6): below the
    ball's 4/3 pi r^3 by the border's share.  The count of unordered pairs is close to Poisson, so K is within 6 / sqrt(cumulative / 2)
    of that, relatively; 6 standard deviations, five radii: the bracket fails by chance less than once in 10^8 seeds.
    Clustered scene: 80 % of the points sit in three Gaussian blobs of sigma 2.5, a third each.  Two points of one blob differ by
    N(0, 2 sigma^2) an axis, so d^2 / 12.5 is chi-squared with 3 degrees: P(d <= 5) = P(chi2_3 <= 2) = 0.4276.  The share of ordered
    pairs within 5 is at least 3 (0.8 / 3)^2 0.4276 = 0.091 in expectation; the bracket asks for half of it, K(5) > 0.045 V, against the
    4/3 pi 125 = 524 of a uniform scene in a window of some 10^5: H(5) is far above 0."""
    S, n = 40.0, 3000
    P = np.random.default_rng(12).uniform(0.0, S, (n, 3)).astype(np.float32)
    radii = np.array([1.5, 3.0, 4.0, 6.0, 8.0])
    K, L, H, c = ripley_host(P, radii, S ** 3)
    t = radii / S
    want = S ** 3 * (4.0 / 3.0 * np.pi * t ** 3 - 1.5 * np.pi * t ** 4 + 1.6 * t ** 5 - t ** 6 / 6.0)
    assert (np.abs(K / want - 1.0) < 6.0 / np.sqrt(c['cumulative'].astype(np.float64) / 2.0)).all(), (K / want, c['cumulative'])
    assert (K < 4.0 / 3.0 * np.pi * radii ** 3 * 1.02).all() and (H < 0.02 * radii).all() and (H > -0.12 * radii).all()     # no edge correction: biased low
    Q = R.clustered(2500, 13)
    V = float(np.prod(Q.max(0).astype(np.float64) - Q.min(0).astype(np.float64)))
    K, L, H, c = ripley_host(Q, [5.0], V)
    assert K[0] > 0.045 * V and K[0] > 20.0 * 524.0 and H[0] > 5.0


@pytest.mark.parametrize('mutation, radii', [('closed_left', [1.0, 1.5, 2.0]), ('keep_self', [0.0, 1.0]), ('unordered', [1.0, 1.5, 2.0])])
def test_each_mutation_is_caught(mutation, radii):
    """one line of the definition broken on purpose: the lattice's closed form notices every one"""
    P = R.lattice(7)
    good, bad = R.pair_counts(P, radii), R.pair_counts(P, radii, mutate=mutation)
    assert not np.array_equal(good['hist'], bad['hist'])
    if mutation == 'closed_left':
        assert bad['hist'].tolist() == [0, 4788, 1728]            # the pairs at exactly 1 and exactly 2 have moved up
    elif mutation == 'keep_self':
        assert bad['hist'].tolist() == [343, 1764] and good['hist'].tolist() == [0, 1764]
    else:
        assert (bad['hist'] * np.uint64(2) == good['hist']).all()
