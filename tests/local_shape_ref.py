"""
The local-shape query of include/nw_structure.h restated in NumPy: brute force over all pairs in row blocks, no grid, int64 moments, the
covariance and the Jacobi iteration in csrc/nw_structure_core.h's order.  tests/test_local_shape_ref.py ties it to closed forms, to
np.linalg.eigvalsh and to the radial direction of a sphere shell; the compiled core and the device are asked for its arrays bit for bit.

    r2        = r * r in float64;  R = the smallest power of two >= r;  s = 2^18 / R;  step = R / 2^18
    d2(i, j)  = (ex*ex + ey*ey) + ez*ez in float64, e = (double)cloud_j - (double)query_i   (NumPy multiplies and adds separately: no fma)
    N(i)      = { j : d2(i, j) <= r2 }; auto mode is cross mode with the cloud as its own queries
    u         = rint(e * s) per axis (np.rint: ties to even), an int64
    moments   = (n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz), int64
    m_a       = S_a / n,  C_ab = S_ab / n - m_a m_b  in float64
    Jacobi    : SWEEPS sweeps of rotations (0,1), (0,2), (1,2); a rotation is skipped where a_pq == 0
    order     : descending by three strict exchanges (0,1), (1,2), (0,1); eigenvalues scaled (l * step) * step
    signs     : the component of largest magnitude positive (the first on a tie); with a viewpoint the normal faces it

`mutate` breaks one rule on purpose (the tests show that they notice): 'open_ball' leaves a point at exactly r out (< for <=), 'no_rint'
truncates e * s, 'order' runs the rotations as (0,2), (0,1), (1,2).
"""
import numpy as np

SWEEPS = 5
MAX_R = 2.0 ** 40
Q_ONE = 2.0 ** 18
FLAG_VALID, FLAG_EMPTY, FLAG_FEW, FLAG_POINT, FLAG_TURNED = 1, 2, 4, 8, 16
# Median and maximum angle (degrees) between the normal and the radial direction, up to sign, measured on this restatement for the three
# noisy sphere shells of tests/test_local_shape_ref.py (radius 100, sigma 3); the tests assert ANGLE_FACTOR x these.  (A prototype with
# other seeds saw medians 2.5-3.2 and maxima 6.3-9.4: context, not the bound.)
SHELL_ANGLES = {'2000_r50': (1.2198, 4.4307), '2000_r35': (1.7506, 6.0479), '20000_r20': (1.6492, 5.6535)}
ANGLE_FACTOR = 1.5


def cloud32(points):
    return np.ascontiguousarray(points, np.float32).reshape(-1, 3)


def scale(r):
    """-> (r2, R, s, step), checked as nwf_radius checks"""
    r = float(r)
    if not (r > 0.0 and r <= MAX_R):
        raise ValueError('radius')
    r2 = r * r
    if not (r2 > 0.0 and np.isfinite(r2)):
        raise ValueError('radius')
    f, e = np.frexp(r)
    R = r if f == 0.5 else float(np.ldexp(1.0, e))
    return r2, R, Q_ONE / R, R / Q_ONE


def moments(points, radius, other=None, mutate=None):
    """(n_queries, 10) int64.  other = None: auto mode on `points`; else the queries `points` against the cloud `other`."""
    r2, _, s, _ = scale(radius)
    Q = cloud32(points).astype(np.float64)
    P = Q if other is None else cloud32(other).astype(np.float64)
    out = np.zeros((len(Q), 10), np.int64)
    block = max(1, 200000 // max(len(P), 1))
    for a in range(0, len(Q), block):
        e = P[None, :, :] - Q[a:a + block, None, :]
        d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        near = d2 < r2 if mutate == 'open_ball' else d2 <= r2
        es = np.where(near[..., None], e * s, 0.0)
        u = (np.trunc(es) if mutate == 'no_rint' else np.rint(es)).astype(np.int64)
        ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
        rows = out[a:a + block]
        rows[:, 0] = near.sum(1)
        rows[:, 1], rows[:, 2], rows[:, 3] = ux.sum(1), uy.sum(1), uz.sum(1)
        rows[:, 4], rows[:, 5], rows[:, 6] = (ux * ux).sum(1), (ux * uy).sum(1), (ux * uz).sum(1)
        rows[:, 7], rows[:, 8], rows[:, 9] = (uy * uy).sum(1), (uy * uz).sum(1), (uz * uz).sum(1)
    return out


def covariance(M):
    """the six elements (a00, a01, a02, a11, a12, a22) of C, float64 arrays; rows with n = 0 are nan"""
    M = np.asarray(M, np.int64).reshape(-1, 10)
    with np.errstate(all='ignore'):
        dn = M[:, 0].astype(np.float64)
        mx, my, mz = M[:, 1].astype(np.float64) / dn, M[:, 2].astype(np.float64) / dn, M[:, 3].astype(np.float64) / dn
        f = lambda k: M[:, k].astype(np.float64) / dn
        return [f(4) - mx * mx, f(5) - mx * my, f(6) - mx * mz, f(7) - my * my, f(8) - my * mz, f(9) - mz * mz]


def _rotate(A, V, p, q):
    """one rotation of nwf_rotate on arrays: A = dict of the six elements keyed (i, j) with i <= j, V = dict keyed (row, column)"""
    r = 3 - p - q
    key = lambda i, j: (min(i, j), max(i, j))
    app, aqq, apq, arp, arq = A[(p, p)], A[(q, q)], A[(p, q)], A[key(r, p)], A[key(r, q)]
    skip = apq == 0.0
    theta = (aqq - app) / (2.0 * apq)
    sgn = np.where(theta >= 0.0, 1.0, -1.0)
    t = sgn / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    tapq = t * apq
    keep = lambda old, new: np.where(skip, old, new)
    A[(p, p)], A[(q, q)], A[(p, q)] = keep(app, app - tapq), keep(aqq, aqq + tapq), keep(apq, 0.0)
    A[key(r, p)], A[key(r, q)] = keep(arp, c * arp - s * arq), keep(arq, s * arp + c * arq)
    for k in range(3):
        vp, vq = V[(k, p)], V[(k, q)]
        V[(k, p)], V[(k, q)] = keep(vp, c * vp - s * vq), keep(vq, s * vp + c * vq)


def jacobi(C, sweeps=SWEEPS, mutate=None):
    """-> (A, V) after `sweeps` sweeps: A the dict of the six elements, V the dict of the nine (row, column)"""
    n = len(C[0])
    A = {(0, 0): C[0].copy(), (0, 1): C[1].copy(), (0, 2): C[2].copy(), (1, 1): C[3].copy(), (1, 2): C[4].copy(), (2, 2): C[5].copy()}
    V = {(i, j): np.full(n, 1.0 if i == j else 0.0) for i in range(3) for j in range(3)}
    order = [(0, 2), (0, 1), (1, 2)] if mutate == 'order' else [(0, 1), (0, 2), (1, 2)]
    with np.errstate(all='ignore'):
        for _ in range(sweeps):
            for p, q in order:
                _rotate(A, V, p, q)
    return A, V


def off_diagonal(A):
    """the largest off-diagonal magnitude relative to the largest diagonal magnitude, over all rows (rows of zeros aside)"""
    off = np.maximum(np.maximum(np.abs(A[(0, 1)]), np.abs(A[(0, 2)])), np.abs(A[(1, 2)]))
    top = np.maximum(np.maximum(np.abs(A[(0, 0)]), np.abs(A[(1, 1)])), np.abs(A[(2, 2)]))
    ok = top > 0
    return float((off[ok] / top[ok]).max()) if ok.any() else 0.0


def shape(M, radius, queries=None, viewpoint=None, mutate=None):
    """nwf_shape on every row of the moments -> dict(eigenvalues (nq,3), vectors (nq,3,3): rows axis, mid, normal; flags (nq,) uint8).
    `queries` (the float32 positions) is needed with a viewpoint only."""
    M = np.asarray(M, np.int64).reshape(-1, 10)
    _, _, _, step = scale(radius)
    A, V = jacobi(covariance(M), mutate=mutate)
    lam = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
    vec = [[V[(0, j)], V[(1, j)], V[(2, j)]] for j in range(3)]              # vec[j] = column j

    def exchange(a, b):
        swap = lam[b] > lam[a]
        lam[a], lam[b] = np.where(swap, lam[b], lam[a]), np.where(swap, lam[a], lam[b])
        for k in range(3):
            vec[a][k], vec[b][k] = np.where(swap, vec[b][k], vec[a][k]), np.where(swap, vec[a][k], vec[b][k])
    exchange(0, 1)
    exchange(1, 2)
    exchange(0, 1)
    lam = [(l * step) * step for l in lam]
    for j in range(3):
        big = vec[j][0]
        big = np.where(np.abs(vec[j][1]) > np.abs(big), vec[j][1], big)
        big = np.where(np.abs(vec[j][2]) > np.abs(big), vec[j][2], big)
        flip = big < 0.0
        vec[j] = [np.where(flip, -v, v) for v in vec[j]]
    n = M[:, 0]
    flags = np.zeros(len(M), np.uint8)
    if viewpoint is not None:
        w = np.asarray(viewpoint, np.float64).reshape(1, 3) - cloud32(queries).astype(np.float64)
        with np.errstate(all='ignore'):
            turn = ((vec[2][0] * w[:, 0] + vec[2][1] * w[:, 1]) + vec[2][2] * w[:, 2] < 0.0) & (n > 0)
        vec[2] = [np.where(turn, -v, v) for v in vec[2]]
        flags[turn] |= FLAG_TURNED
    lam = np.stack(lam, 1)
    vec = np.stack([np.stack(v, 1) for v in vec], 1)
    empty = n == 0
    lam[empty] = np.nan
    vec[empty] = 0.0
    flags[empty] |= FLAG_EMPTY
    flags[(n > 0) & (n < 3)] |= FLAG_FEW
    with np.errstate(invalid='ignore'):
        full = (n >= 3) & (lam[:, 0] > 0.0)
    flags[full] |= FLAG_VALID
    flags[(n >= 3) & ~full] |= FLAG_POINT
    return dict(eigenvalues=lam, vectors=vec, flags=flags)


def features(M, lam, flags, radius):
    """structure.py's features, restated: float64 from the integers and the eigenvalues, max(lambda, 0), nan where not valid"""
    _, _, _, step = scale(radius)
    M = np.asarray(M, np.int64).reshape(-1, 10)
    valid = (flags & FLAG_VALID) != 0
    with np.errstate(all='ignore'):
        l = np.maximum(lam, 0.0)
        l0, l1, l2 = l[:, 0], l[:, 1], l[:, 2]
        dn = M[:, 0].astype(np.float64)
        m = M[:, 1:4].astype(np.float64) / dn[:, None]
        out = dict(linearity=(l0 - l1) / l0, planarity=(l1 - l2) / l0, scattering=l2 / l0, surface_variation=l2 / (l0 + l1 + l2),
                   centroid_offset=np.sqrt((m * m).sum(1)) * step)
    for k in out:
        out[k] = np.where(valid, out[k], np.nan)
    out['valid'] = valid
    return out


def local_shape(points, radius, other=None, viewpoint=None, mutate=None):
    """the whole query -> dict(moments, n, eigenvalues, vectors, axis, normal, flags, valid and the features)"""
    M = moments(points, radius, other, mutate)
    out = shape(M, radius, points, viewpoint, mutate)
    out.update(features(M, out['eigenvalues'], out['flags'], radius))
    out.update(moments=M, n=M[:, 0].copy(), axis=out['vectors'][:, 0], normal=out['vectors'][:, 2])
    return out


def same_as_restatement(mine, ref):
    """every integer and every bit"""
    assert mine['moments'].dtype == np.int64 and np.array_equal(mine['moments'], ref['moments'])
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    assert mine['eigenvalues'].shape == ref['eigenvalues'].shape and np.array_equal(bits(mine['eigenvalues']), bits(ref['eigenvalues']))
    assert mine['vectors'].shape == ref['vectors'].shape and np.array_equal(bits(mine['vectors']), bits(ref['vectors']))
    assert mine['flags'].dtype == np.uint8 and np.array_equal(mine['flags'], ref['flags'])


# ---- clouds ---------------------------------------------------------------------------------------------------------------------------------
def lattice(k, step=1.0):
    """the k^3 integer lattice, scaled"""
    g = np.arange(k, dtype=np.float64) * step
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


def shell(n, seed, radius=100.0, sigma=3.0, centre=(0.0, 0.0, 0.0)):
    """a noisy sphere shell: uniform directions, radius + N(0, sigma)"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return (np.asarray(centre) + u * (radius + rng.normal(0.0, sigma, (n, 1)))).astype(np.float32)


def mixed(n, seed, offset=0.0):
    """a sheet, a tubule and a blob with a uniform background: every shape class in one cloud"""
    rng = np.random.default_rng(seed)
    k = n // 4
    sheet = np.c_[rng.uniform(0, 60, k), rng.uniform(0, 60, k), rng.normal(10.0, 0.5, k)]
    t = rng.uniform(0, 60, k)
    tube = np.c_[t, 0.5 * t + rng.normal(0, 0.6, k), 40.0 - 0.3 * t + rng.normal(0, 0.6, k)]
    blob = rng.normal((30.0, 30.0, 40.0), 3.0, (k, 3))
    back = rng.uniform(-5.0, 65.0, (n - 3 * k, 3))
    return (np.concatenate([sheet, tube, blob, back]) + offset).astype(np.float32)
