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


# ---- inputs for the edge tests (tests/test_hip_simulation_edges.py; tests/test_simulation.py checks on the restatement that each reaches what
# it is named for) ------------------------------------------------------------------------------------------------------------------------
OFFSET = np.array([0.21, 0.13, 0.37])          # a lattice origin off the cube's centre: no node sits on the shell's edge
SEEDS = (7, 7 + (1 << 32), (1 << 64) - 1)      # the low word alone; the same low word and a high word; every bit
COUNTS = (1, 255, 256, 257)                    # around one workgroup
COMBINATORS = {'union': S.UnionShape, 'difference': S.DifferenceShape, 'intersection': S.IntersectionShape}
_SIZE_ARG = {S.OP_SPHERE: 0, S.OP_TORUS: 1, S.OP_CAPSULE: 6, S.OP_ROUND_BOX: 3, S.OP_SHEET: 3}      # the argument that shifts a primitive's distance


def _directions():
    d = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
    return d / np.sqrt((d * d).sum(1))[:, None]


def stack_depth(ops):
    """the deepest value stack the program needs"""
    depth = deepest = 0
    for op in ops:
        code = int(op['code'])
        depth += 0 if code == S.OP_FRAME else -1 if code >= S.OP_UNION else 1
        deepest = max(deepest, depth)
    return deepest


def operand_values(ops, P):
    """(n_primitives, n) the distance every primitive pushes, in program order: each primitive alone under the frame that holds for it"""
    out, frame = [], None
    for op in ops:
        code = int(op['code'])
        if code == S.OP_FRAME:
            frame = op
        elif code < S.OP_UNION:
            out.append(eval_program(([frame] if frame is not None else []) + [op], P))
    return np.array(out)


def deciding_operands(ops, P, which=None):
    """(n_primitives, n) bool: whether the program's value at a point changes when that primitive's distance is shifted by 1 (its radius
    argument); `which` picks primitives by their order.  A primitive that is True nowhere could be lost or swapped without a trace on these points."""
    ops = np.array(ops, S.OP_DTYPE)
    base, out = eval_program(ops, P), []
    prims = np.flatnonzero((ops['code'] != S.OP_FRAME) & (ops['code'] < S.OP_UNION))
    for i in prims if which is None else prims[list(which)]:
        code = int(ops['code'][i])
        bumped = ops.copy()
        bumped['a'][i, _SIZE_ARG[code]] += 1.0
        out.append(eval_program(bumped, P) != base)
    return np.array(out)


def chain_spheres(kind, n):
    """n spheres of distinct radii about distinct centres, the first about the origin (it needs no frame op), placed so that every one
    decides a chain of `kind` somewhere: apart from each other for a union (each the nearest near itself); the same, and all inside a last
    large one, for a difference (each carves a piece of its own); all overlapping about the origin for an intersection (each the farthest
    on the side away from its centre, the first -- the smallest -- above and below the others' plane)"""
    ring = [(np.cos(2.0 * np.pi * i / 7.0), np.sin(2.0 * np.pi * i / 7.0)) for i in range(n)]
    if kind == 'intersection':
        return [S.Sphere(radius=9.0)] + [S.Sphere(radius=10.0 + 0.125 * i, centroid=[2.0 * ring[i][0], 2.0 * ring[i][1], 0.0625 * i]) for i in range(1, n)]
    out = [S.Sphere(radius=3.0)] + [S.Sphere(radius=2.0 + 0.125 * i, centroid=[6.0 * ring[i][0], 6.0 * ring[i][1], 0.5 * i - 1.0]) for i in range(1, n)]
    if kind == 'difference':
        out[-1] = S.Sphere(radius=9.5, centroid=[0.25, -0.5, 0.75])
    return out


def chain(kind, k, n, operands=None):
    """The right-nested chain c(o_0, c(o_1, ... c(o_{n-2}, o_{n-1}))): every operand is pushed before the first combinator runs, so the
    program needs a stack of n and operand i waits in slot n - 1 - i.  -> the compiled program"""
    operands = chain_spheres(kind, n) if operands is None else operands
    node = operands[-1]
    for o in operands[-2::-1]:
        node = COMBINATORS[kind](o, node, k=k)
    return S.compile_shape(node)


def chain_winner(kind, ops, P):
    """which operand a k = 0 chain's value is at every point: the nearest of a union, the farthest of an intersection, the largest of
    (-d_0, .., -d_{n-2}, d_{n-1}) of a difference"""
    v = operand_values(ops, P)
    return np.argmin(v, 0) if kind == 'union' else np.argmax(v, 0) if kind == 'intersection' else np.argmax(np.vstack([-v[:-1], v[-1:]]), 0)


def mixed_operands():
    """eight operands, all five primitives among them, one under a RotationShape; the two that a difference carves out overlap what they
    are carved from"""
    return [S.Sphere(radius=12.0), S.Torus(radius=3.0, r=1.5, centroid=[0.0, 9.0, 0.0]), S.Capsule([-9.0, -3.0, 0.0], [-9.0, 4.0, 1.0], 1.25),
            S.Box([2.0, 3.0, 1.0], r=0.5, centroid=[0.0, 9.0, 0.0]), S.RotationShape(S.Sheet([4.0, 3.0, 0.75], 0.75, centroid=[0.0, -9.0, 1.0]), rx=0.3, rz=0.7),
            S.Sphere(radius=2.5, centroid=[7.0, 7.0, 1.0]), S.Box([1.5, 1.5, 2.5], r=0.0, centroid=[1.0, 1.0, -8.0]),
            S.Capsule([6.0, 6.0, -2.0], [8.0, 8.0, 3.0], 1.0)]


def mixed_chain():
    """right-nested over mixed_operands(), depth 8, every combinator, k = 0 and k > 0"""
    o = mixed_operands()
    node = S.UnionShape(o[6], o[7], k=0.5)
    node = S.DifferenceShape(o[5], node, k=0.0)
    node = S.UnionShape(o[4], node, k=0.0)
    node = S.UnionShape(o[3], node, k=0.75)
    node = S.UnionShape(o[2], node, k=0.0)
    node = S.DifferenceShape(o[1], node, k=0.5)
    return S.compile_shape(S.IntersectionShape(o[0], node, k=0.25))


def chain_points(ops, distances=(0.5, 1.5, 2.5, 4.0, 12.0), n_random=64, seed=11):
    """Points about every primitive of the program: the origin of its frame (a capsule's two ends), 26 directions from it at `distances`,
    and a random cloud"""
    ops = np.asarray(ops)
    centres = [np.zeros(3)] + [np.array(op['a'][9:12]) for op in ops if int(op['code']) == S.OP_FRAME]
    for op in ops:
        if int(op['code']) == S.OP_CAPSULE:
            centres += [np.array(op['a'][0:3]), np.array(op['a'][3:6])]
    d = _directions()
    pts = [c[None, :] + t * d for c in centres for t in distances] + [np.array(centres)]
    pts.append(np.random.default_rng(seed).uniform(-14.0, 14.0, (n_random, 3)))
    return np.ascontiguousarray(np.vstack(pts))


def long_program():
    """NWG_MAX_OPS ops at a stack of 2: the left-nested union, k = 0 and k > 0 in turn, of 100 capsules and of 28 boxes about one centre
    (one frame op for all of them), each box longer than every one before it along one axis, so that the last ops decide at its ends.
    -> (the compiled program, points)"""
    rng = np.random.default_rng(5)
    node, centre = None, np.array([1.0, -2.0, 0.5])
    for i in range(128):
        if i < 100:
            a = rng.uniform(-10.0, 10.0, 3)
            prim = S.Capsule(a, a + rng.uniform(1.0, 4.0, 3) * rng.choice([-1.0, 1.0], 3), 0.25 + 0.01 * i)
        else:
            w = np.ones(3)
            w[i % 3] = 3.0 + 0.125 * i
            prim = S.Box(w, r=0.125 * (i % 3), centroid=centre)
        node = prim if node is None else S.UnionShape(node, prim, k=0.25 * (i % 2))
    prog = S.compile_shape(node)
    ends = np.array([s * (2.0 + 0.125 * i) * np.eye(3)[i % 3] for i in range(100, 128) for s in (-1.0, 1.0)])
    return prog, np.ascontiguousarray(np.vstack([chain_points(prog.ops, distances=(1.5,)), centre + ends]))


def primitive_edge_cases():
    """name -> (shape, (n,3) points at the primitive's singular points).  Coordinates are small integers and halves, Pythagorean where a
    square root is taken, so that the distances named in the comments are exact."""
    cases = {}
    c = np.array([10.0, -20.0, 5.0])
    cases['sphere'] = (S.Sphere(radius=5.0, centroid=c),                                                    # the centre; d = 0 exactly
                       c + np.array([[0, 0, 0], [5, 0, 0], [0, -5, 0], [0, 0, 5], [3, 4, 0], [0, -3, 4], [1, 2, 2], [2, 3, 6]], np.float64))
    cases['torus'] = (S.Torus(radius=100.0, r=30.0, centroid=c),                                            # the axis, the centre, the centre circle
                      c + np.array([[0, 0, 0], [0, 7, 0], [0, -75, 0], [100, 0, 0], [0, 0, -100], [60, 0, 80], [-28, 0, 96], [60, 30, 80], [130, 0, 0],
                                    [70, 0, 0], [100, -30, 0]], np.float64))
    a, b = np.array([0.0, -5.0, 0.0]), np.array([0.0, 5.0, 0.0])
    cases['capsule'] = (S.Capsule(a, b, 2.0),                                                               # h < 0, = 0, = 1, > 1; on the axis
                        np.array([[0, -9, 0], [3, -9, 4], [0, -5, 0], [3, -5, 4], [0, 5, 0], [-3, 5, 4], [0, 9, 0], [4, 9, 3], [0, 0, 0], [0, 2.5, 0],
                                  [2, 0, 0], [0, -7, 0], [0, 7, 0]], np.float64))
    cases['capsule_oblique'] = (S.Capsule([1.0, 2.0, 3.0], [4.0, 6.0, 3.0], 1.5),                           # |b - a| = 5
                                np.array([[1, 2, 3], [4, 6, 3], [-2, -2, 3], [7, 10, 3], [1, 2, 5], [4, 6, 1], [2.5, 4, 3], [-3, 5, 3], [8, 3, 3], [1, 2, 4.5], [2.5, 4, 1.5]], np.float64))
    w = np.array([4.0, 3.0, 2.0])
    signs = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.float64)     # centre, 6 faces, 12 edges, 8 corners
    out = np.array([[7, 7, 2], [8, 0, 0], [4, 6, 6], [-7, -7, -4]], np.float64)
    for name, r in (('box', 0.0), ('round_box', 0.5)):
        cases[name] = (S.Box(w, r=r, centroid=c), c + np.vstack([signs * w, signs * (w + r), signs * 0.5 * w, out]))
    for name, r in (('sheet', 0.5), ('sheet_r0', 0.0)):
        cases[name] = (S.Sheet(w, r, centroid=c), c + np.vstack([signs * w, signs * (w + r), signs * 0.5 * w, out, [[0, 0, 2 + r], [4 + r, 0, 0], [4, 3, 0]]]))
    return cases


def tie_case(kind, k):
    """-> (program, points, d0, d1): two spheres of radii 4 and 6 (6 and 6 for union and intersection) about (-3, 0, 0) and (3, 0, 0).
    k = 0: points where the combinator's two arguments are equal in every bit -- d0 == d1 on the plane x = 0, -d0 == d1 where
    |p - a| = |p - b| = 5 (the circle of radius 4 in that plane).  k > 0: points where | d0 - d1 | (difference: | -d0 - d1 |) is k exactly, and
    points 2^-40 (relative) to both sides of them."""
    ra = 4.0 if kind == 'difference' else 6.0
    s0, s1 = S.Sphere(radius=ra, centroid=[-3.0, 0.0, 0.0]), S.Sphere(radius=6.0, centroid=[3.0, 0.0, 0.0])
    prog = chain(kind, k, 2, [s0, s1])
    if k == 0:
        pts = [[0, 4, 0], [0, -4, 0], [0, 0, 4], [0, 2.4, 3.2], [0, -3.2, 2.4]]
        if kind != 'difference':
            pts += [[0, 0, 0], [0, 1, 0], [0, 7, -2], [0, 0.3, 0.7], [0, 100, 50]]
    else:
        # on the x axis between the centres, |x| < 3: |p - a| = x + 3 and |p - b| = 3 - x.  Union and intersection (radii 6, 6): d0 - d1 = 2 x,
        # k at x = +- k / 2.  Difference (radii 4, 6): -d0 - d1 = 10 - (|p - a| + |p - b|) is 4 there; beyond b it is 10 - 2 x, +- k at x = 5 -+ k / 2
        x = [5.0 - 0.5 * k, 5.0 + 0.5 * k] if kind == 'difference' else [0.5 * k, -0.5 * k]
        pts = [[v * f, 0.0, 0.0] for v in x for f in (1.0, 1.0 + 2.0 ** -40, 1.0 - 2.0 ** -40)]
    pts = np.array(pts, np.float64)
    d = operand_values(prog.ops, pts)
    return prog, pts, d[0], d[1]


def lattice_case(name):
    """The rows of the lattice table -> dict(shape, centre, r_max, dx, p, seed, project, levels)"""
    h = float((1 << 20) - 1)
    return {
        # nodes on half-integers, the faces at 8: the layer at 7.5 has d = -0.5 = -dx/2 exactly (kept), the layer at 8.5 d = +0.5 on the faces (left out)
        'shell_edge': dict(shape=S.Box([8.0, 8.0, 8.0], r=0.0), centre=[0.5, 0.5, 0.5], r_max=12.0, dx=1.0, p=1.0, seed=0, project=0, levels=(-1, 0, 3)),
        # the cube cuts the sphere: `>= imin`, `<= imax` and in_cube decide
        'cube_cut': dict(shape=S.Sphere(radius=30.0), centre=OFFSET, r_max=20.0, dx=1.0, p=1.0, seed=0, project=2, levels=(-1, 0, 3)),
        # a plate half a pitch thick: the nodes of its mid-plane are fluorophores at d = -0.25 where the central difference is 0 on every axis
        'flat_spot': dict(shape=S.Box([8.0, 8.0, 0.25], r=0.0), centre=[0.0, 0.0, 0.0], r_max=12.0, dx=1.0, p=1.0, seed=0, project=2, levels=(-1, 0, 3)),
        # node coordinates over all NWG_COORD_BITS bits; start levels 0 and 3 would list more start cells than the call accepts
        'widest': dict(shape=S.Sphere(radius=30.0, centroid=np.array([h - 40.0, -(h - 40.0), 123456.0]) + OFFSET), centre=[0.0, 0.0, 0.0], r_max=h + 0.5, dx=1.0,
                       p=0.5, seed=7, project=2, levels=(-1, 18, 20)),
        'one_node': dict(shape=S.Sphere(radius=0.2), centre=[0.0, 0.0, 0.0], r_max=0.75, dx=1.0, p=1.0, seed=0, project=2, levels=(-1, 0, 3)),
        'outside': dict(shape=S.Sphere(radius=5.0, centroid=[100.0, 0.0, 0.0]), centre=OFFSET, r_max=10.0, dx=1.0, p=1.0, seed=0, project=2, levels=(-1, 0, 3)),
    }[name]


def run_lattice_case(case, level, **over):
    kw = dict(case, **over)
    prog = S.compile_shape(kw['shape'])
    return prog, lattice(prog.ops, kw['centre'], kw['r_max'], kw['dx'], kw['p'], kw['seed'], start_level=level, n_project=kw['project'])
