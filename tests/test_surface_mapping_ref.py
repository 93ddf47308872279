"""
The restatement of the localization mapping (tests/surface_mapping_ref.py) tied to closed forms that do not come from it: exact weights
on a right triangle with exact centroid and on mesh_distance_ref.cube(), the band's closed edge, conservation, independence of the
cloud's order and of chunking, the +-scale value columns, the vertex areas, and two physical cases on a sphere.  Then three one-line
mutations of the definition, each caught by one of these checks.  No GPU and no compiled code.
"""
import functools

import numpy as np
import pytest

import mesh_distance_ref as D
import surface_mapping_ref as M
from ch_shrinkwrap_amd.trimesh import icosphere

W = M.W_ONE


def one(point, band=10.0, mutation=None, mesh=None):
    v, f = mesh or M.right_triangle()
    return M.map_cloud(np.array([point], np.float64), v, f, band, mutation=mutation)


# ---- exact weights ----------------------------------------------------------------------------------------------------------------------
def test_a_point_over_a_vertex_gives_it_everything():
    assert one([-1.0, -1.0, 1.0])['weights'].tolist() == [[W, 0, 0]]
    assert one([5.0, -1.0, -2.0])['weights'].tolist() == [[0, W, 0]]
    assert one([-0.5, 4.0, 0.0])['weights'].tolist() == [[0, 0, W]]
    v, f = D.cube()
    r = one([2.0, 2.0, 2.0], mesh=(v, f))                                  # beyond corner 7 = (1, 1, 1)
    face = int(r['face'][0])
    assert sorted(r['weights'][0].tolist()) == [0, 0, W] and f[face][int(np.argmax(r['weights'][0]))] == 7
    assert face == min(i for i in range(len(f)) if 7 in f[i])               # the smallest id among the equally near faces
    assert r['mass'][7] == W and r['mass'].sum() == W and r['count'][face] == 1 and r['count'].sum() == 1


def test_a_point_over_an_edge_midpoint_gives_each_end_half():
    assert one([1.5, -1.0, 0.5])['weights'].tolist() == [[W // 2, W // 2, 0]]        # edge 0: a -> b
    assert one([2.0, 2.0, 1.0])['weights'].tolist() == [[0, W // 2, W // 2]]         # edge 1: b -> c, midpoint (1.5, 1.5, 0)
    assert one([-2.0, 1.5, 0.0])['weights'].tolist() == [[W // 2, 0, W // 2]]        # edge 2: c -> a
    assert one([0.75, -1.0, 0.0])['weights'].tolist() == [[3 * W // 4, W // 4, 0]]   # a quarter of the way from a to b
    v, f = D.cube()
    r = one([0.0, 2.0, 2.0], mesh=(v, f))                                  # the edge from (-1, 1, 1) to (1, 1, 1): vertices 6 and 7
    assert r['mass'][6] == W // 2 and r['mass'][7] == W // 2


def test_a_point_over_the_centroid_gives_thirds_and_the_last_corner_the_rest():
    r = one([1.0, 1.0, 5.0])
    assert r['weights'].tolist() == [[349525, 349525, 349526]] and r['distance'][0] == 5.0
    assert one([1.0, 1.0, -5.0])['weights'].tolist() == [[349525, 349525, 349526]]
    # barycentric in general: q = (0.75, 1.5, 0) = 0.25 a + 0.25 b + 0.5 c
    assert one([0.75, 1.5, 2.0])['weights'].tolist() == [[W // 4, W // 4, W // 2]]


def test_a_face_at_exactly_the_band_is_in_band_and_one_ulp_below_is_not():
    for point in ([1.0, 1.0, 0.1], [-1.0, -1.0, 1.0], [1.5, -0.3, 0.2]):
        d = float(one(point)['distance'][0])
        assert 0 < d < 2
        at = one(point, band=d)
        assert at['n_in_band'] == 1 and at['face'][0] == 0 and at['mass'].sum() == W
        below = one(point, band=np.nextafter(d, 0.0))
        assert below['n_in_band'] == 0 and below['face'][0] == -1 and not below['weights'].any() and np.isinf(below['distance'][0])
        assert np.isnan(below['closest']).all() and not below['mass'].any() and not below['count'].any()


# ---- the accumulators -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cube_case():
    v, f = D.cube()
    pts = M.cloud_around(v, 700, 5, spread=1.6)
    rng = np.random.default_rng(2)
    vals = np.stack([rng.uniform(-900.0, 5000.0, len(pts)), rng.integers(0, 2, len(pts)).astype(np.float64), np.zeros(len(pts))], 1)
    scales = np.array([8192.0, 1.0, 1.0])
    return v, f, pts, vals, scales, M.map_cloud(pts, v, f, 0.6, vals, scales)


def test_conservation_of_mass_and_counts():
    v, f, pts, vals, scales, r = cube_case()
    assert 100 < r['n_in_band'] < len(pts)
    assert int(r['mass'].sum()) == r['n_in_band'] * W and int(r['count'].sum()) == r['n_in_band']
    assert (r['weights'][r['in_band']].sum(1) == W).all() and (r['weights'] >= 0).all()
    # the mean of a column that is 1 everywhere it counts: the flags' sum against the mass
    total = M.column_sums(r['sum_hi'], r['sum_lo'])
    assert not total[:, 2].any() and (total[:, 1] >= 0).all() and (total[:, 1] <= r['mass'].astype(object) * M.Q_ONE).all()


def test_the_order_of_the_cloud_and_chunking_do_not_show():
    v, f, pts, vals, scales, r = cube_case()
    perm = np.random.default_rng(9).permutation(len(pts))
    M.same_accumulators(M.map_cloud(pts[perm], v, f, 0.6, vals[perm], scales), r)
    acc = None
    for s, e in ((0, 1), (1, 300), (300, len(pts))):
        acc = M.map_cloud(pts[s:e], v, f, 0.6, vals[s:e], scales, onto=acc)
    M.same_accumulators(acc, r)


def test_a_column_at_plus_and_minus_its_scale():
    v, f, pts, _, _, base = cube_case()
    vals = np.stack([np.full(len(pts), 64.0), np.full(len(pts), -64.0)], 1)
    r = M.map_cloud(pts, v, f, 0.6, vals, np.array([64.0, 64.0]))
    total = M.column_sums(r['sum_hi'], r['sum_lo'])
    expect = r['mass'].astype(object) * M.Q_ONE
    assert (total[:, 0] == expect).all() and (total[:, 1] == -expect).all() and expect.any()
    assert (r['sum_hi'][:, 1] <= 0).all() and (r['sum_hi'][:, 1] < 0).any()          # the arithmetic shift at work
    _, _, _, means = M.densities(r['mass'], M.vertex_areas(v, f), r['sum_hi'], r['sum_lo'], [64.0, 64.0])
    seen = r['mass'] > 0
    assert (means[seen, 0] == 64.0).all() and (means[seen, 1] == -64.0).all() and np.isnan(means[~seen]).all()


def test_values_beyond_the_scale_count_only_in_band():
    v, f, pts, _, _, base = cube_case()
    far, near = int(np.flatnonzero(~base['in_band'])[0]), int(np.flatnonzero(base['in_band'])[0])
    vals = np.ones((len(pts), 1))
    vals[far] = 1.5
    M.same_accumulators(M.map_cloud(pts, v, f, 0.6, vals, [1.0]), M.map_cloud(pts, v, f, 0.6, np.ones((len(pts), 1)), [1.0]))
    vals[far] = np.nan
    M.map_cloud(pts, v, f, 0.6, vals, [1.0])
    vals[near] = 1.5
    with pytest.raises(M.MappingRangeError):
        M.map_cloud(pts, v, f, 0.6, vals, [1.0])
    vals[near] = np.inf
    with pytest.raises(M.MappingNonFiniteError):
        M.map_cloud(pts, v, f, 0.6, vals, [1.0])
    # ties go to even: 2^-31 and 3 2^-31 of the scale are halves of a unit
    q, _, _ = M.quantise(np.array([2.0 ** -31, 3 * 2.0 ** -31, -2.0 ** -31, 1.0, -1.0]), 1.0)
    assert q.tolist() == [0, 2, 0, M.Q_ONE, -M.Q_ONE]


def test_vertex_areas_add_up_to_the_mesh_area():
    """Every face's floor(A_f 2^20) goes to its three corners, so sum(area3) / 3 = sum_f floor(A_f 2^20): it is short of 2^20 times the
    mesh area by less than 1 a face, beside the rounding of A_f itself (a cross product, a dot product and a root in float64: a few
    ulp, 1e-14 relative is generous).  Bound: 0 <= area - sum(area3) / (3 2^20) <= F 2^-20 + 1e-14 area."""
    for (v, f), area in ((D.cube(), 24.0), (M.right_triangle(), 4.5)):
        a3 = M.vertex_areas(v, f)
        total = int(a3.astype(object).sum())
        assert total % 3 == 0
        assert -1e-14 * area <= area - total / 3 / W <= len(f) * 2.0 ** -20 + 1e-14 * area
    assert M.vertex_areas(*M.right_triangle()).tolist() == [4718592] * 3            # 4.5 2^20, exact
    assert M.vertex_areas(*D.degenerate_faces()).tolist() == [W // 2] * 3 + [0] * 4   # faces without area add nothing


# ---- physical cases ---------------------------------------------------------------------------------------------------------------------
R, N_DENSE = 100.0, 8000


@functools.lru_cache(maxsize=None)
def sphere_case(kind):
    v, f = icosphere(2, R)
    pts = M.sphere_points(10000, R, 21, jitter=2.0) if kind == 'uniform' else M.two_density_points(N_DENSE, R, 31, jitter=2.0)
    return v, f, pts, M.map_cloud(pts, v, f, 30.0), M.vertex_areas(v, f)


def test_a_uniform_sphere_has_the_density_n_over_area():
    v, f, pts, r, a3 = sphere_case('uniform')
    assert r['n_in_band'] == len(pts)
    n, area, density, _ = M.densities(r['mass'], a3)
    mesh_area = float(M.face_areas_q(v, f).sum()) / W
    assert abs(area.sum() - mesh_area) < 1e-9 * mesh_area and 0.97 * 4 * np.pi * R * R < mesh_area < 4 * np.pi * R * R
    # the area-weighted mean of the density is N / area: sum(density area) = sum(n) = N
    assert abs((density * area).sum() / area.sum() - len(pts) / mesh_area) < 1e-9 * len(pts) / mesh_area
    # per vertex: about 10000 / 162 = 62 localizations each, Poisson: every vertex within 6 sigma of the mean (6 / sqrt(62) = 0.76),
    # beside the 12 five-valent vertices' smaller share, which the area accounts for
    assert (np.abs(density / (len(pts) / mesh_area) - 1.0) < 0.76).all()


def test_a_hemisphere_four_times_as_dense_is_recovered_as_such():
    """The density over the vertices with z > 0.2 R against that over z < -0.2 R (the belt between them mixes the two sides through
    the weights and is left out).  The caps hold 0.8 of their hemispheres' localizations, about 6400 and 1600, both Poisson; the
    ratio's relative standard deviation is sqrt(1/6400 + 1/1600) = 0.028.  Bracket: five of them, 14 %, plus 1 % for the faces that
    straddle a cap's edge (they move mass both ways at one density): 4 (1 - 0.15) < ratio < 4 (1 + 0.15)."""
    v, f, pts, r, a3 = sphere_case('two')
    assert r['n_in_band'] == len(pts) == N_DENSE + N_DENSE // 4
    up, low = v[:, 2] > 0.2 * R, v[:, 2] < -0.2 * R
    m, a = r['mass'].astype(np.float64), a3.astype(np.float64)
    ratio = (m[up].sum() / a[up].sum()) / (m[low].sum() / a[low].sum())
    assert 4 * 0.85 < ratio < 4 * 1.15


# ---- mutations --------------------------------------------------------------------------------------------------------------------------
def battery(mutation):
    """the names of the checks above that a mutated definition fails"""
    failed = []
    v, f = M.right_triangle()
    r = one([1.0, 1.0, 5.0], mutation=mutation)
    if r['weights'].tolist() != [[349525, 349525, 349526]] or int(r['mass'].sum()) != W:
        failed.append('centroid')
    d = float(one([1.0, 1.0, 0.1])['distance'][0])
    if one([1.0, 1.0, 0.1], band=d, mutation=mutation)['n_in_band'] != 1:
        failed.append('band')
    cv, cf, pts, _, _, _ = cube_case()
    vals = np.stack([np.full(len(pts), 64.0), np.full(len(pts), -64.0)], 1)
    r = M.map_cloud(pts, cv, cf, 0.6, vals, np.array([64.0, 64.0]), mutation=mutation)
    total, expect = M.column_sums(r['sum_hi'], r['sum_lo']), r['mass'].astype(object) * M.Q_ONE
    if not ((total[:, 0] == expect).all() and (total[:, 1] == -expect).all()):
        failed.append('minus scale')
    if int(r['mass'].sum()) != r['n_in_band'] * W:
        failed.append('conservation')
    return failed


def test_three_one_line_mutations_are_caught():
    assert battery(None) == []
    assert 'centroid' in battery('wc_not_rest') and 'conservation' in battery('wc_not_rest')
    assert battery('logical_shift') == ['minus scale']
    assert battery('strict_band') == ['band']
    assert set(M.MUTATIONS) == {'wc_not_rest', 'logical_shift', 'strict_band'}
