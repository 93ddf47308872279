"""
NumPy restatement of ch_shrinkwrap_amd/csrc/nw_poisson_core.h: the yardstick the screened Poisson grid solver is compared with, bit for
bit (tests/test_poisson_core_cpu.py for the header under g++, tests/test_hip_poisson.py for the kernels), and that is itself checked
against dense solves, closed forms and the true surfaces of simulated clouds (tests/test_screened_poisson_ref.py).

Arrays of a level are indexed [z, y, x] with n = 2^level nodes an axis; node i of an axis sits at lo + (i + 1/2) h_l.  Every float64
expression below is written in the order the header states, one rounding per operation; the integers are exact.

    quantise_normals   n / |n| in float64 (or as given with use_lengths), rint(. 2^12) per axis; zero length: not used
    axis_weights       u = (p - lo) / h_l - 1/2, i0 = floor(u), q = rint((u - i0) 128): 128 - q on i0 and q on i0 + 1, both clamped
    splat              W and V[3] of a level as int64 sums
    occupancy          the number of distinct home nodes clamp(floor(u + 1/2)) of a level
    depth_used         the global depth rule of samplespernode and fulldepth
    system             rhs and diag of a level
    relax / residual   red-black Gauss-Seidel sweeps in place, even colour first; max |rhs - (diag chi - sum of neighbours)|
    prolong            0.75 / 0.25 axis by axis, x then y then z, the neighbour clamped at the border
    field              M, E, F = rint(chi / E 2^31) + 2^31 as uint64, thr = floor(sum W F / sum W) from two 16-bit limbs
    solve              the driver: everything above from the samples to (F, thr), keeping every level's arrays
"""
import numpy as np

MAX_N = 1 << 25
NORMAL_BITS, WEIGHT_BITS, FIELD_BITS = 12, 7, 31             # the three quantisation exponents: normals, splat weights per axis, field
BASE_LEVEL, MIN_DEPTH, MAX_DEPTH = 2, 3, 9
W_ONE = 1 << (3 * WEIGHT_BITS)                               # a sample's eight weights add up to 2^21
V_ONE = float(1 << (3 * WEIGHT_BITS + NORMAL_BITS))          # 2^33: a unit normal at a node centre
MUTATIONS = ('colour', 'prolong', 's2')                      # what tests/test_screened_poisson_ref.py breaks on purpose


class BorderError(ValueError):
    """the level set reaches the outermost layer of the lattice: the normals point inwards"""


def quantise_normals(normals, use_lengths=False):
    """-> (nq (n,3) int64, used (n,) bool)"""
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    if not np.isfinite(n).all():
        raise ValueError('a normal is not finite')
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    used = length > 0.0
    if use_lengths:
        if (np.abs(n) > 1.0).any():
            raise ValueError('a normal component above 1 with use_lengths')
        unit = n
    else:
        with np.errstate(all='ignore'):
            unit = n / length[:, None]
    nq = np.zeros(n.shape, np.int64)
    nq[used] = np.rint(unit[used] * float(1 << NORMAL_BITS)).astype(np.int64)
    return nq, used


def level_spacing(h, depth, level):
    return float(np.float32(h)) * float(1 << (depth - level))


def axis_u(p, lo, hl):
    return (np.asarray(p, np.float32).astype(np.float64) - float(np.float32(lo))) / hl - 0.5


def axis_weights(p, lo, hl, n):
    """-> (ia, ib, wa, wb) int64: the two nodes of every coordinate and their weights, wa + wb = 128"""
    u = axis_u(p, lo, hl)
    fl = np.floor(u)
    q = np.rint((u - fl) * float(1 << WEIGHT_BITS)).astype(np.int64)
    ia = np.minimum(np.maximum(fl, 0.0), float(n - 1)).astype(np.int64)
    ib = np.minimum(np.maximum(fl + 1.0, 0.0), float(n - 1)).astype(np.int64)
    return ia, ib, (1 << WEIGHT_BITS) - q, q


def axis_home(p, lo, hl, n):
    return np.minimum(np.maximum(np.floor(axis_u(p, lo, hl) + 0.5), 0.0), float(n - 1)).astype(np.int64)


def splat(points, nq, used, lo, h, depth, level):
    """-> (W (n,n,n) int64, V (3,n,n,n) int64), [z, y, x]"""
    n = 1 << level
    hl = level_spacing(h, depth, level)
    P = np.asarray(points, np.float32).reshape(-1, 3)[used]
    Q = nq[used]
    ax = [axis_weights(P[:, d], np.asarray(lo, np.float32)[d], hl, n) for d in range(3)]
    W = np.zeros(n * n * n, np.int64)
    V = np.zeros((3, n * n * n), np.int64)
    for c in range(8):
        pick = [(ax[d][(c >> d) & 1], ax[d][2 + ((c >> d) & 1)]) for d in range(3)]
        w = pick[0][1] * pick[1][1] * pick[2][1]
        lin = (pick[2][0] * n + pick[1][0]) * n + pick[0][0]
        np.add.at(W, lin, w)
        for a in range(3):
            np.add.at(V[a], lin, w * Q[:, a])
    return W.reshape(n, n, n), V.reshape(3, n, n, n)


def occupancy(points, used, lo, h, depth, level):
    n = 1 << level
    hl = level_spacing(h, depth, level)
    P = np.asarray(points, np.float32).reshape(-1, 3)[used]
    hx, hy, hz = (axis_home(P[:, d], np.asarray(lo, np.float32)[d], hl, n) for d in range(3))
    return int(np.unique((hz * n + hy) * n + hx).size)


def depth_used(n_used, occ, depth, fulldepth, samples_per_node):
    """occ[l] for l = 2 .. depth -> the level the solve ends and the surface is extracted at"""
    used = BASE_LEVEL
    for l in range(BASE_LEVEL + 1, depth + 1):
        if l > max(int(fulldepth), BASE_LEVEL) and float(n_used) < float(samples_per_node) * float(occ[l]):
            break
        used = l
    return used


def alpha_of(pointweight, occ_used, n_used):
    return (float(pointweight) * float(occ_used)) / float(n_used)


def system(W, V, alpha, s, mutate=None):
    """-> (rhs, diag) float64 of a level; s = 2^(used - level)"""
    n = W.shape[0]
    What = W.astype(np.float64) / float(W_ONE)
    Vhat = -(V.astype(np.float64)) / V_ONE
    rhs = np.zeros((n, n, n))
    deg = np.zeros((n, n, n))
    for a, axis in enumerate((2, 1, 0)):                             # x, y, z of an array indexed [z, y, x]
        lo_ = [slice(None)] * 3
        hi_ = [slice(None)] * 3
        lo_[axis], hi_[axis] = slice(0, -1), slice(1, None)
        lo_, hi_ = tuple(lo_), tuple(hi_)
        g = 0.5 * (Vhat[a][lo_] + Vhat[a][hi_])
        rhs[hi_] += g                                                # the edge below a node
        rhs[lo_] -= g                                                # the edge above it
        deg[hi_] += 1.0
        deg[lo_] += 1.0
    if mutate != 's2':
        rhs = rhs * (1.0 / (float(s) * float(s)))
    diag = deg + (float(alpha) / float(s)) * What
    return rhs, diag


def neighbour_sum(chi):
    """the present neighbours added in the order -x, +x, -y, +y, -z, +z, from 0"""
    S = np.zeros(chi.shape)
    S[:, :, 1:] += chi[:, :, :-1]
    S[:, :, :-1] += chi[:, :, 1:]
    S[:, 1:, :] += chi[:, :-1, :]
    S[:, :-1, :] += chi[:, 1:, :]
    S[1:, :, :] += chi[:-1, :, :]
    S[:-1, :, :] += chi[1:, :, :]
    return S


def colour_mask(n, colour):
    i = np.arange(n)
    return ((i[:, None, None] + i[None, :, None] + i[None, None, :]) & 1) == colour


def relax(chi, rhs, diag, sweeps, mutate=None):
    """in place; a sweep is the even colour, then the odd"""
    n = chi.shape[0]
    masks = [colour_mask(n, c) for c in ((1, 0) if mutate == 'colour' else (0, 1))]
    for _ in range(int(sweeps)):
        for m in masks:
            new = (rhs + neighbour_sum(chi)) / diag
            chi[m] = new[m]
    return chi


def residual(chi, rhs, diag):
    return float(np.abs(rhs - (diag * chi - neighbour_sum(chi))).max())


def prolong(a, mutate=None):
    wn, wf = (0.5, 0.5) if mutate == 'prolong' else (0.75, 0.25)
    for axis in (2, 1, 0):
        n = a.shape[axis]
        idx = np.arange(n)
        near = np.take(a, idx, axis)
        below = np.take(a, np.maximum(idx - 1, 0), axis)
        above = np.take(a, np.minimum(idx + 1, n - 1), axis)
        shape = list(a.shape)
        shape[axis] = 2 * n
        out = np.empty(shape)
        ev = [slice(None)] * 3
        od = [slice(None)] * 3
        ev[axis], od[axis] = slice(0, None, 2), slice(1, None, 2)
        out[tuple(ev)] = wn * near + wf * below
        out[tuple(od)] = wn * near + wf * above
        a = out
    return a


def pow2_above(m):
    """the smallest power of two >= m (m > 0)"""
    f, e = np.frexp(float(m))
    return float(m) if f == 0.5 else float(np.ldexp(1.0, e))


def quantise_field(chi, E):
    return (np.rint((chi / E) * float(1 << FIELD_BITS)) + float(1 << FIELD_BITS)).astype(np.uint64)


def level_of(W, F):
    """(thr, limb sums lo and hi, sum W) with Python integers"""
    Fi = F.astype(np.int64)
    lo_sum = int((W * (Fi & 0xffff)).sum())
    hi_sum = int((W * (Fi >> 16)).sum())
    sw = int(W.sum())
    return ((hi_sum << 16) + lo_sum) // sw, lo_sum, hi_sum, sw


def field(chi, W):
    """-> dict(M, E, F uint64 [z, y, x], thr, limbs, sumW); M = 0 raises"""
    M = float(np.abs(chi).max())
    if not M > 0.0:
        raise ValueError('the solution is zero everywhere')
    E = pow2_above(M)
    F = quantise_field(chi, E)
    thr, lo_sum, hi_sum, sw = level_of(W, F)
    return dict(M=M, E=E, F=F, thr=thr, limbs=(lo_sum, hi_sum), sumW=sw)


def solve(points, normals, lo, h, depth, fulldepth=5, samples_per_node=1.5, pointweight=4.0, iters=8, coarse_iters=64, use_lengths=False,
          mutate=None, keep_levels=True):
    """The whole procedure -> dict(n_used, n_skipped, occ {level: count}, depth_used, h_used (float32), alpha, levels {level: dict(W, V, rhs,
    diag, chi)}, residuals {level: (before, after)}, chi, W, and field()'s entries)."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if not np.isfinite(P).all():
        raise ValueError('a sample is not finite')
    if not (MIN_DEPTH <= int(depth) <= MAX_DEPTH) or not float(pointweight) > 0.0:
        raise ValueError('depth is in 3..9 and pointweight above 0')
    lo = np.asarray(lo, np.float32).reshape(3)
    h = np.float32(h)
    nq, used_mask = quantise_normals(normals, use_lengths)
    n_used = int(used_mask.sum())
    if n_used < 1 or n_used > MAX_N:
        raise ValueError('no usable sample, or more than 2^25')
    occ = {l: occupancy(P, used_mask, lo, h, depth, l) for l in range(BASE_LEVEL, depth + 1)}
    used = depth_used(n_used, occ, depth, fulldepth, samples_per_node)
    alpha = alpha_of(pointweight, occ[used], n_used)
    levels, residuals = {}, {}
    chi = None
    for l in range(BASE_LEVEL, used + 1):
        n = 1 << l
        W, V = splat(P, nq, used_mask, lo, h, depth, l)
        rhs, diag = system(W, V, alpha, 1 << (used - l), mutate)
        chi = np.zeros((n, n, n)) if l == BASE_LEVEL else prolong(chi, mutate)
        before = residual(chi, rhs, diag)
        relax(chi, rhs, diag, coarse_iters if l == BASE_LEVEL else iters, mutate)
        residuals[l] = (before, residual(chi, rhs, diag))
        if keep_levels or l == used:
            levels[l] = dict(W=W, V=V, rhs=rhs, diag=diag, chi=chi.copy())
    out = dict(n_used=n_used, n_skipped=int(len(P) - n_used), occ=occ, depth_used=used, h_used=np.float32(float(h) * float(1 << (depth - used))),
               alpha=alpha, levels=levels, residuals=residuals, chi=chi, W=levels[used]['W'], lo=lo, h=h, depth=int(depth))
    out.update(field(chi, out['W']))
    return out


def cube_for(points, depth, scale=1.1):
    """(lo (3,) float32, h float32) of the cube of a cloud: ch_shrinkwrap_amd.poisson.cube_for restated"""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    mn, mx = p.min(0), p.max(0)
    side = float(scale) * float((mx - mn).max())
    if not side > 0.0:
        raise ValueError('the cloud has no extent')
    centre = 0.5 * (mn + mx)
    return (centre - 0.5 * side).astype(np.float32), np.float32(side / float(1 << int(depth)))


def mesh(result):
    """(vertices, faces, keys) of F > thr at the level used, by the isosurface restatement's surface nets"""
    import isosurface_ref as I
    try:
        return I.surface_nets(result['F'], result['thr'], result['lo'], result['h_used'])
    except ValueError as e:
        if 'outermost layer' in str(e):
            raise BorderError(str(e))
        raise


def reconstruct(points, normals, depth=7, fulldepth=4, scale=1.1, samples_per_node=1.5, pointweight=4.0, iters=8, coarse_iters=64, **kw):
    lo, h = cube_for(points, depth, scale)
    r = solve(points, normals, lo, h, depth, fulldepth, samples_per_node, pointweight, iters, coarse_iters, keep_levels=False, **kw)
    v, f, k = mesh(r)
    r.update(vertices=v, faces=f, keys=k)
    return r


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------------
def special_positions(lo, hl, nl):
    """node centres, cell boundaries and one float32 step either side, ties of the weight at k + 1/2, the outermost half cells and beyond"""
    lo = float(np.float32(lo))
    out = []
    for i in (0, 1, nl // 2, nl - 2, nl - 1):
        c = lo + (i + 0.5) * hl
        b = lo + (i + 1.0) * hl
        for x in (c, b, lo + i * hl):
            x32 = np.float32(x)
            out += [x32, np.nextafter(x32, np.float32(np.inf)), np.nextafter(x32, np.float32(-np.inf))]
        for k in (0, 1, 63, 64, 126, 127):
            out.append(np.float32(c + (k + 0.5) / 128.0 * hl))
    out += [np.float32(lo), np.float32(lo + 0.25 * hl), np.float32(lo + 0.5 * hl), np.float32(lo + nl * hl), np.float32(lo + (nl - 0.25) * hl),
            np.float32(lo - 3.0 * hl), np.float32(lo + (nl + 7.0) * hl), np.float32(-3.0e38), np.float32(3.0e38)]
    return np.array(out, np.float32)


# ---- clouds with known surfaces ----------------------------------------------------------------------------------------------------------
def sphere_cloud(n, radius=100.0, sigma=0.0, seed=0):
    """(points float32, true outward normals float32) of a sphere at the origin, the points displaced by an isotropic normal error"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    p = radius * u + (sigma * rng.normal(size=(n, 3)) if sigma > 0 else 0.0)
    return p.astype(np.float32), u.astype(np.float32)


def sphere_sdf(v, radius=100.0):
    return np.linalg.norm(np.asarray(v, np.float64), axis=1) - radius


def torus_cloud(n, R=100.0, r=30.0, sigma=0.0, seed=0):
    """uniform in the two angles (denser on the inside of the ring), axis z"""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.0, 2.0 * np.pi, n)
    nrm = np.stack([np.cos(a) * np.cos(b), np.sin(a) * np.cos(b), np.sin(b)], 1)
    p = np.stack([R * np.cos(a), R * np.sin(a), np.zeros(n)], 1) + r * nrm
    p = p + (sigma * rng.normal(size=(n, 3)) if sigma > 0 else 0.0)
    return p.astype(np.float32), nrm.astype(np.float32)


def torus_sdf(v, R=100.0, r=30.0):
    v = np.asarray(v, np.float64)
    return np.sqrt((np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2) - R) ** 2 + v[:, 2] ** 2) - r


def mesh_report(vertices, faces):
    """dict(components [(faces, Euler, volume)], manifold: every edge used twice, balanced)"""
    import isosurface_ref as I
    comps = I.components(vertices, faces)
    return dict(components=[(len(ids), chi, vol) for ids, chi, vol in comps], manifold=bool((I.edge_use(faces) == 2).all()),
                balanced=I.directed_edges_balanced(faces))
