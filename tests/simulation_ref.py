"""
NumPy restatement of include/nw_simulation.h: the yardstick the simulator's kernels are compared with (tests/test_hip_simulation.py) and that
is itself checked against Random123's known answers, the reference's shapes and the reference's loc_error (tests/test_simulation.py).

    philox4x32_10        the published round function; counter (item lo, item hi, stream, draw), key (seed lo, seed hi)
    uniform, normal, key64   the header's maps from a block's four words
    eval_program         the postfix program of nwg_op at (n,3) points, float64, sdf.py's expressions
    lattice              the surface lattice: cells kept by their centre's distance, split into eight per level; shell test; thinning; projection
    loc_error, displace, smlmify, background   the localization model, the clusters, the background
"""
import numpy as np

from ch_shrinkwrap_amd import simulation as S

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
BIAS = 1 << (S.COORD_BITS - 1)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of Salmon, Moraes, Dror and Shaw (SC'11): arrays (or ints) of 32-bit words -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, np.uint64)) & np.uint64(MASK) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                      # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def block(item, stream, draw, seed):
    item = np.atleast_1d(np.asarray(item, np.uint64))
    seed = int(seed)
    return philox4x32_10(item & np.uint64(MASK), item >> np.uint64(32), np.uint64(stream), np.uint64(draw), seed & MASK, (seed >> 32) & MASK)


def _unit(hi, lo):
    return ((((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def uniform(item, stream, draw, seed):
    w = block(item, stream, draw, seed)
    return _unit(w[0], w[1])


def normal(item, stream, draw, seed):
    w = block(item, stream, draw, seed)
    return np.sqrt(-2.0 * np.log(_unit(w[0], w[1]))) * np.cos(2.0 * np.pi * _unit(w[2], w[3]))


def key64(item, stream, seed):
    w = block(item, stream, 0, seed)
    return (w[0] << np.uint64(32)) | w[1]


# ---- the shape ------------------------------------------------------------------------------------------------------------------------
def eval_program(ops, P):
    P = np.asarray(P, np.float64).reshape(-1, 3)
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    qx, qy, qz = px, py, pz
    stack = []
    for op in ops:
        code, a = int(op['code']), [float(x) for x in op['a']]
        if code == S.OP_FRAME:
            ex, ey, ez = px - a[9], py - a[10], pz - a[11]
            qx = (a[0] * ex + a[1] * ey) + a[2] * ez
            qy = (a[3] * ex + a[4] * ey) + a[5] * ez
            qz = (a[6] * ex + a[7] * ey) + a[8] * ez
        elif code == S.OP_SPHERE:
            stack.append(np.sqrt((qx * qx + qy * qy) + qz * qz) - a[0])
        elif code == S.OP_TORUS:
            t = np.sqrt(qx * qx + qz * qz) - a[0]
            stack.append(np.sqrt(t * t + qy * qy) - a[1])
        elif code == S.OP_CAPSULE:
            bx, by, bz = a[3] - a[0], a[4] - a[1], a[5] - a[2]
            ux, uy, uz = qx - a[0], qy - a[1], qz - a[2]
            h = np.clip(((ux * bx + uy * by) + uz * bz) / ((bx * bx + by * by) + bz * bz), 0.0, 1.0)
            dx, dy, dz = ux - bx * h, uy - by * h, uz - bz * h
            stack.append(np.sqrt((dx * dx + dy * dy) + dz * dz) - a[6])
        elif code in (S.OP_ROUND_BOX, S.OP_SHEET):
            x, y, z = np.abs(qx) - a[0], np.abs(qy) - a[1], np.abs(qz) - a[2]
            m = np.maximum(x, np.maximum(y, z))
            if code == S.OP_ROUND_BOX:
                x0, y0, z0 = np.maximum(x, 0.0), np.maximum(y, 0.0), np.maximum(z, 0.0)
                stack.append(np.sqrt((x0 * x0 + y0 * y0) + z0 * z0) + np.minimum(m, 0.0) - a[3])
            else:
                e, f = np.maximum(x, y) + a[3], z + a[2]
                stack.append(np.minimum(np.sqrt(e * e + f * f) - a[3], m))
        else:
            d1, d0, k = stack.pop(), stack.pop(), a[0]
            if code == S.OP_UNION:
                res = np.minimum(d0, d1)
                if k > 0:
                    h = np.maximum(k - np.abs(d0 - d1), 0.0)
                    res = res - h * h * 0.25 / k
            elif code == S.OP_DIFFERENCE:
                res = np.maximum(-d0, d1)
                if k > 0:
                    h = np.maximum(k - np.abs(-d0 - d1), 0.0)
                    res = res + h * h * 0.25 / k
            elif code == S.OP_INTERSECTION:
                res = np.maximum(d0, d1)
                if k > 0:
                    h = np.maximum(k - np.abs(d0 - d1), 0.0)
                    res = res + h * h * 0.25 / k
            else:
                raise ValueError('unknown op %d' % code)
            stack.append(res)
    assert len(stack) == 1
    return stack[0]


def gradient(ops, P, delta=0.1):
    P = np.asarray(P, np.float64).reshape(-1, 3)
    d2 = delta / 2.0
    g = np.empty(P.shape)
    for k in range(3):
        h = np.zeros(3)
        h[k] = d2
        g[:, k] = (eval_program(ops, P + h[None, :]) - eval_program(ops, P - h[None, :])) / delta
    return g


def normals(ops, P):
    g = gradient(ops, P)
    return g / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]


# ---- the surface lattice --------------------------------------------------------------------------------------------------------------
def morton(xyz):
    """63-bit Morton code of (n,3) biased node coordinates: bit 3b + axis = bit b of that axis."""
    xyz = np.asarray(xyz, np.uint64)
    key = np.zeros(xyz.shape[0], np.uint64)
    for b in range(S.COORD_BITS):
        for ax in range(3):
            key |= ((xyz[:, ax] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + ax)
    return key


def node_positions(nodes, centre, dx):
    return np.asarray(centre, np.float64)[None, :] + (np.asarray(nodes, np.int64) - BIAS).astype(np.float64) * dx


def project(ops, P, steps):
    P = np.array(P, np.float64)
    live = np.ones(P.shape[0], bool)
    for _ in range(int(steps)):
        d, g = eval_program(ops, P), gradient(ops, P)
        g2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        live &= g2 > 0.0
        with np.errstate(divide='ignore', invalid='ignore'):
            t = d / g2
        P = np.where(live[:, None], P - t[:, None] * g, P)
    return P


_CHILD = np.array([[k & 1, (k >> 1) & 1, k >> 2] for k in range(8)], np.int64)


def lattice(ops, centre, r_max, dx, p, seed, lipschitz=S.LIPSCHITZ, start_level=-1, n_project=2, brute_force=False):
    """-> dict(keys, nodes (biased int coordinates), lattice (the nodes' positions), points (projected), margin (the smallest
    | |sdf| - dx/2 | over the candidate nodes: the shell test is safe against rounding while it is well above the arithmetic's error),
    n_fluorophores (before thinning))."""
    centre = np.asarray(centre, np.float64).reshape(3)
    half = int(np.floor(r_max / dx))
    imin, imax = BIAS - half, BIAS + half
    if brute_force:
        ax = np.arange(imin, imax + 1, dtype=np.int64)
        z, y, x = np.meshgrid(ax, ax, ax, indexing='ij')
        nodes = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        nodes = nodes[np.argsort(morton(nodes), kind='stable')]
    else:
        level = int(start_level)
        if level < 0:
            level = 0
            while (imax >> level) - (imin >> level) + 1 > 8:
                level += 1
        ax = np.arange(imin >> level, (imax >> level) + 1, dtype=np.int64)
        z, y, x = np.meshgrid(ax, ax, ax, indexing='ij')
        cells = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        cells = cells[np.argsort(morton(cells), kind='stable')]
        while level > 0:
            side = 1 << level
            lo = cells << level
            in_cube = ((lo <= imax) & (lo + side - 1 >= imin)).all(1)
            c = centre[None, :] + ((lo - BIAS).astype(np.float64) + (side - 1) * 0.5) * dx
            bound = lipschitz * (0.8660254037844386 * dx * float(side)) + 0.5 * dx
            keep = in_cube & (np.abs(eval_program(ops, c)) <= bound)
            cells = (cells[keep][:, None, :] * 2 + _CHILD[None, :, :]).reshape(-1, 3)
            level -= 1
        nodes = cells
    inside = ((nodes >= imin) & (nodes <= imax)).all(1)
    nodes = nodes[inside]
    pos = node_positions(nodes, centre, dx)
    d = eval_program(ops, pos) if nodes.shape[0] else np.zeros(0)
    margin = float(np.abs(np.abs(d) - 0.5 * dx).min()) if d.size else np.inf
    shell = (d >= -0.5 * dx) & (d < 0.5 * dx)
    nodes, pos = nodes[shell], pos[shell]
    keys = morton(nodes)
    detected = uniform(keys, S.STREAM_THIN, 0, seed) < p if keys.size else np.zeros(0, bool)
    out = dict(n_fluorophores=int(shell.sum()), margin=margin, keys=keys[detected], nodes=nodes[detected], lattice=pos[detected])
    out['points'] = project(ops, out['lattice'], n_project) if n_project else out['lattice'].copy()
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _psf(psf_width):
    w = np.asarray(psf_width, np.float64)
    return np.full(3, float(w)) if w.ndim == 0 else w


def loc_error(n, seed, stream, psf_width, mean_photon_count, bg_photon_count, items=None):
    """-> (sigma, photons), (n,3) each: l = bg + mean * (-ln U), sigma = (psf / 2.355) / sqrt(l)"""
    items = np.arange(n, dtype=np.uint64) if items is None else np.asarray(items, np.uint64)
    psf = _psf(psf_width)
    l = np.stack([float(bg_photon_count) + float(mean_photon_count) * (-np.log(uniform(items, stream, a, seed))) for a in range(3)], 1)
    return (psf[None, :] / 2.355) / np.sqrt(l), l


def displace(xyz, sigma, seed, stream, items=None):
    xyz = np.asarray(xyz, np.float64)
    items = np.arange(xyz.shape[0], dtype=np.uint64) if items is None else np.asarray(items, np.uint64)
    return xyz + np.asarray(sigma, np.float64) * np.stack([normal(items, stream, a, seed) for a in range(3)], 1)


def select_copies(n, sz, seed, stream_key):
    """the sz copies (of COPIES * n) with the smallest keys, equal keys by index, in copy order"""
    j = np.arange(S.COPIES * n, dtype=np.uint64)
    order = np.lexsort((j, key64(j, stream_key, seed)))
    return np.sort(order[:sz]).astype(np.int64)


def smlmify(xyz, sigma, seed, streams, psf_width, mean_photon_count, bg_photon_count, sz=None):
    xyz, sigma = np.asarray(xyz, np.float64), np.asarray(sigma, np.float64)
    n = xyz.shape[0]
    copy = select_copies(n, n if sz is None else sz, seed, streams[1])
    src = copy % n
    out = displace(xyz[src], sigma[src], seed, streams[0], items=copy)
    return out, loc_error(copy.size, seed, streams[2], psf_width, mean_photon_count, bg_photon_count, items=copy)[0], copy


def background(lo, hi, n, seed, stream):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    i = np.arange(n, dtype=np.uint64)
    return np.stack([uniform(i, stream, a, seed) * (hi[a] - lo[a]) + lo[a] for a in range(3)], 1)
