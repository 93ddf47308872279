"""
Localizations mapped onto a mesh, restated in NumPy with Python integers: what ch_shrinkwrap_amd/csrc/nw_mapping_core.h defines, by
brute force.  The closest face, point and feature of every localization come from mesh_distance_ref.distance (every face against every
point, no grid); the weights are computed in the header's written order in float64 (NumPy rounds every product and every sum, as the
header does when it is compiled with -ffp-contract=off); the accumulators are integers added with np.add.at.

    weights        W (n,3) of closest points on features of faces
    quantise       q = rint(x / scale * 2^30) and the two error masks
    vertex_areas   area3 (V,)
    map_cloud      the per-localization record and the accumulators of a cloud, onto fresh accumulators or a previous call's
    densities      the divisions

MUTATIONS names three one-line changes to the definition that tests/test_surface_mapping_ref.py shows its checks catch.
tests/test_surface_mapping_ref.py ties this file to closed forms that do not come from it.
"""
import numpy as np

import mesh_distance_ref as D

W_ONE = 1 << 20
Q_ONE = 1 << 30
MUTATIONS = ('wc_not_rest', 'logical_shift', 'strict_band')


def _edge_weight(q, v, w):
    d = w - v
    dd = D._dot(d, d)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(dd > 0.0, D._dot(q - v, d) / dd, 0.0)
    t = np.where(~(t > 0.0), 0.0, np.where(t >= 1.0, 1.0, t))
    return np.floor(t * float(W_ONE)).astype(np.int64)


def weights(closest, a, b, c, feature, mutation=None):
    """W (n,3) int64 for closest points (n,3) on features (n,) of the faces with float64 corners a, b, c (n,3)"""
    q = np.asarray(closest, np.float64).reshape(-1, 3)
    feature = np.asarray(feature).ravel()
    n = len(q)
    W = np.zeros((n, 3), np.int64)
    corner = (a, b, c)
    for k in range(3):
        W[feature == 4 + k, k] = W_ONE
        m = feature == 1 + k
        if m.any():
            w1 = _edge_weight(q[m], corner[k][m], corner[(k + 1) % 3][m])
            W[m, (k + 1) % 3] = w1
            W[m, k] = W_ONE - w1
    m = feature == 0
    if m.any():
        qa, A, B, C = q[m], a[m], b[m], c[m]
        nrm = D._cross(B - A, C - A)
        e0 = D._dot(D._cross(B - A, qa - A), nrm)
        e1 = D._dot(D._cross(C - B, qa - B), nrm)
        e2 = D._dot(D._cross(A - C, qa - C), nrm)
        e0, e1, e2 = (np.where(e < 0.0, 0.0, e) for e in (e0, e1, e2))
        S = (e0 + e1) + e2
        ok = S > 0.0
        with np.errstate(divide='ignore', invalid='ignore'):
            wa = np.where(ok, np.floor(np.where(ok, e1 / S, 0.0) * float(W_ONE)), float(W_ONE)).astype(np.int64)
            wb = np.where(ok, np.floor(np.where(ok, e2 / S, 0.0) * float(W_ONE)), 0.0).astype(np.int64)
        wb = np.minimum(wb, W_ONE - wa)
        if mutation == 'wc_not_rest':                             # W_c from its own edge function and not "the rest"
            with np.errstate(divide='ignore', invalid='ignore'):
                wc = np.where(ok, np.floor(np.where(ok, e0 / S, 0.0) * float(W_ONE)), 0.0).astype(np.int64)
        else:
            wc = W_ONE - wa - wb
        W[m] = np.stack([wa, wb, wc], 1)
    return W


def quantise(x, scale):
    """(q int64, non-finite mask, out-of-range mask) of values x against a power-of-two scale; q is 0 where either mask holds"""
    x = np.asarray(x, np.float64)
    nonfinite = ~np.isfinite(x)
    with np.errstate(over='ignore', invalid='ignore'):
        r = np.rint(np.where(nonfinite, 0.0, x) / scale * float(Q_ONE))
    bad = ~nonfinite & ~(np.abs(r) <= float(Q_ONE))
    return np.where(nonfinite | bad, 0.0, r).astype(np.int64), nonfinite, bad


def limbs(P, mutation=None):
    """(lo uint64 in [0, 2^32), hi int64) of int64 products: P = hi 2^32 + lo, the shift arithmetic"""
    P = np.asarray(P, np.int64)
    lo = (P.view(np.uint64) & np.uint64(0xFFFFFFFF))
    if mutation == 'logical_shift':
        hi = (P.view(np.uint64) >> np.uint64(32)).view(np.int64)
    else:
        hi = P >> 32
    return lo, hi


def face_areas_q(vertices, faces):
    """floor(A_f 2^20) per face, A_f = 0.5 sqrt(n.n), as int64"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = D._cross(b - a, c - a)
    A = 0.5 * np.sqrt(D._dot(n, n))
    assert (A < 2.0 ** 40).all()
    return np.floor(A * float(W_ONE)).astype(np.int64)


def vertex_areas(vertices, faces):
    """area3 (V,) uint64"""
    f = np.asarray(faces).reshape(-1, 3)
    aq = face_areas_q(vertices, f)
    out = np.zeros(len(np.asarray(vertices).reshape(-1, 3)), np.int64)
    for k in range(3):
        np.add.at(out, f[:, k], aq)
    return out.astype(np.uint64)


class MappingRangeError(ValueError):
    pass


class MappingNonFiniteError(ValueError):
    pass


def map_cloud(points, vertices, faces, band, values=None, scales=None, onto=None, mutation=None):
    """dict(face, weights, distance, closest, in_band; mass (V,) uint64, count (F,) int32, sum_hi (V,C) int64, sum_lo (V,C) uint64,
    n_in_band).  values (n,C) with scales (C,); onto: a previous result whose accumulators this cloud is added to."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    f = np.asarray(faces).reshape(-1, 3)
    n, V, F = len(p), len(v), len(f)
    r = D.distance(p, v32, f)
    dist = np.sqrt(r['d2'])
    in_band = (dist < band) if mutation == 'strict_band' else (dist <= band)
    face = np.where(in_band, r['face'], -1).astype(np.int32)
    fa = r['face']
    W = weights(r['closest'], v[f[fa, 0]], v[f[fa, 1]], v[f[fa, 2]], r['feature'], mutation)
    W[~in_band] = 0
    vals = np.zeros((n, 0)) if values is None else np.asarray(values, np.float64).reshape(n, -1)
    C = vals.shape[1]
    sc = np.zeros(0) if C == 0 else np.asarray(scales, np.float64).ravel()
    assert sc.size == C
    if onto is None:
        mass, count = np.zeros(V, np.uint64), np.zeros(F, np.int32)
        sum_hi, sum_lo = np.zeros((V, C), np.int64), np.zeros((V, C), np.uint64)
    else:
        mass, count, sum_hi, sum_lo = (onto[k].copy() for k in ('mass', 'count', 'sum_hi', 'sum_lo'))
        assert sum_hi.shape == (V, C)
    rows = np.flatnonzero(in_band)
    np.add.at(count, fa[rows], 1)
    for k in range(3):
        np.add.at(mass, f[fa[rows], k], W[rows, k].astype(np.uint64))
    for c in range(C):
        q, nonfinite, bad = quantise(vals[rows, c], sc[c])
        if nonfinite.any():
            raise MappingNonFiniteError('a value of an in-band localization is not finite')
        if bad.any():
            raise MappingRangeError('a value of an in-band localization is larger than its scale')
        for k in range(3):
            lo, hi = limbs(W[rows, k] * q, mutation)
            np.add.at(sum_lo[:, c], f[fa[rows], k], lo)
            np.add.at(sum_hi[:, c], f[fa[rows], k], hi)
    closest = np.where(in_band[:, None], r['closest'], np.nan)
    return dict(face=face, weights=W.astype(np.int32), distance=np.where(in_band, dist, np.inf), closest=closest, in_band=in_band,
                mass=mass, count=count, sum_hi=sum_hi, sum_lo=sum_lo, n_in_band=int(in_band.sum()), scales=sc)


def column_sums(sum_hi, sum_lo):
    """sum_hi 2^32 + sum_lo as an object array of Python integers"""
    return np.asarray(sum_hi).astype(object) * (1 << 32) + np.asarray(sum_lo).astype(object)


def densities(mass, area3, sum_hi=None, sum_lo=None, scales=()):
    """(n, area, density, means (V,C)): n = mass / 2^20, area = area3 / (3 2^20), density = 3 mass / area3 (NaN where area3 = 0),
    mean_c = (sum_hi 2^32 + sum_lo) / mass * scale_c / 2^30 (NaN where mass = 0)"""
    m, a = np.asarray(mass).astype(np.float64), np.asarray(area3).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        density = np.where(a > 0, 3.0 * m / a, np.nan)
        means = None
        if sum_hi is not None and np.asarray(sum_hi).shape[1]:
            s = column_sums(sum_hi, sum_lo).astype(np.float64)
            means = np.where(m[:, None] > 0, s / m[:, None] * (np.asarray(scales, np.float64)[None, :] / float(Q_ONE)), np.nan)
    return m / W_ONE, a / (3.0 * W_ONE), density, means


def same_accumulators(x, y):
    for k in ('mass', 'count', 'sum_hi', 'sum_lo'):
        assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), k


def same_as_restatement(mine, ref):
    """the equalities every implementation owes the restatement: the per-localization record bit for bit, the accumulators exactly"""
    assert np.array_equal(mine['face'], ref['face'])
    assert np.array_equal(mine['weights'], ref['weights'])
    assert np.array_equal(D.bits(mine['distance']), D.bits(ref['distance']))
    near = ref['in_band']
    assert np.array_equal(D.bits(mine['closest'][near]), D.bits(ref['closest'][near])) and np.isnan(mine['closest'][~near]).all()
    assert (mine['weights'][near].sum(1) == W_ONE).all() and (mine['weights'] >= 0).all() and not mine['weights'][~near].any()
    if 'mass' in mine:
        same_accumulators(mine, ref)


# ---- the inputs the tests of the restatement, of the compiled core and of the device share ---------------------------------------------
def right_triangle():
    """corners (0,0,0), (3,0,0), (0,3,0): the centroid (1,1,0) and the edge midpoints are exact"""
    return np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0]], np.float32), np.array([[0, 1, 2]], np.int32)


def sphere_points(n, radius, seed, jitter=0.0):
    """n points uniform on a sphere, each moved along its radius by a normal deviate of `jitter`"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u * (radius + jitter * rng.normal(size=(n, 1)))


def two_density_points(n_dense, radius, seed, jitter=0.0):
    """a sphere whose hemisphere z > 0 carries n_dense points and whose other one a quarter of that"""
    a = sphere_points(2 * n_dense, radius, seed, jitter)
    a = a[a[:, 2] > 0][:n_dense]
    b = sphere_points(2 * n_dense, radius, seed + 1, jitter)
    b = b[b[:, 2] < 0][:n_dense // 4]
    return np.vstack([a, b])


def cloud_around(v, n, seed, spread=1.4):
    """localizations in and around a mesh's box, some of them at its vertices"""
    return D.around(v, n, seed, spread)
