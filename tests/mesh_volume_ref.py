"""
The banded signed-distance volume restated in NumPy (include/nw_volume.h, ch_shrinkwrap_amd/csrc/nw_volume_core.h): brute force over
all faces and all nodes through mesh_distance_ref.distance, then the band rule, the predecessor path and the quantisation as plain
loops.

    nodes         the lattice's node positions, x fastest
    in_band       u <= d_cap
    predecessor   (i-1, j, k), else (0, j-1, k), else (0, 0, k-1), else None (the seed)
    seed_sign     the seed's sign from its exact evaluation with no cap
    volume        dict(sd, face, mask, field, u, d2, in_band, margin) per node, in node order

MUTATIONS names three one-line changes (volume(mutate=...)); tests/test_mesh_volume_ref.py shows that each turns an assertion red and
ties this file to ground truth that does not come from it (a box's closed-form distance, lattices inside and outside, nested shells).
"""
import numpy as np

import mesh_distance_ref as D

FIELD_SHIFT = 20
MUTATIONS = ('band_strict', 'successor', 'seed_outside')


def nodes(lo, h, dims):
    """(n,3) float64: node (i, j, k) at (double)lo[a] + ((double)index + 0.5) * (double)h, x fastest"""
    lo = np.asarray(lo, np.float32).astype(np.float64)
    h = float(np.float32(h))
    ax = [lo[a] + (np.arange(int(dims[a]), dtype=np.float64) + 0.5) * h for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def in_band(u, d_cap, mutate=None):
    return u < d_cap if mutate == 'band_strict' else u <= d_cap


def predecessor(i, j, k, dims, mutate=None):
    """the linear index of the node whose sign an out-of-band node takes; None for the seed"""
    nx, ny = int(dims[0]), int(dims[1])
    if mutate == 'successor':                      # (the mirrored path: it starts from the last node, which nothing seeds)
        if i < nx - 1:
            return (k * ny + j) * nx + i + 1
        return None
    if i > 0:
        return (k * ny + j) * nx + i - 1
    if j > 0:
        return (k * ny + j - 1) * nx
    if k > 0:
        return (k - 1) * ny * nx
    return None


def seed_sign(dist0, mutate=None):
    """-1.0 or +1.0: the side of node (0, 0, 0) from its exact signed distance"""
    if mutate == 'seed_outside':
        return 1.0
    return -1.0 if dist0 < 0.0 else 1.0


def quantise(sd, d_cap):
    return np.floor((float(d_cap) - np.asarray(sd, np.float64)) * float(1 << FIELD_SHIFT)).astype(np.uint64)


def volume(vertices, faces, lo, h, dims, d_cap, signed=True, twin=None, mutate=None, check_cap=True):
    """The definition, node by node.  check_cap=False forces a band below h past the argument check (the premise test)."""
    h32 = float(np.float32(h))
    d_cap = float(d_cap)
    if check_cap and not (np.isfinite(d_cap) and h32 <= d_cap <= 2.0 ** 40):
        raise ValueError('d_cap must be finite and within [h, 2^40]')
    dims = [int(d) for d in dims]
    p = nodes(lo, h, dims)
    if signed and twin is None:
        twin = D.twins(faces)
    r = D.distance(p, vertices, faces, twin if signed else None)
    u = np.sqrt(r['d2'])
    band = in_band(u, d_cap, mutate)
    n = p.shape[0]
    face = np.where(band, r['face'], -1).astype(np.int32)
    if not signed:
        sd = np.where(band, u, d_cap)
    else:
        sd = np.where(band, r['dist'], np.nan)
        order = range(n - 1, -1, -1) if mutate == 'successor' else range(n)
        nx, ny = dims[0], dims[1]
        for idx in order:
            if band[idx]:
                continue
            i, j, k = idx % nx, (idx // nx) % ny, idx // (nx * ny)
            pr = predecessor(i, j, k, dims, mutate)
            s = seed_sign(r['dist'][0], mutate) if pr is None else (-1.0 if sd[pr] < 0.0 else 1.0)
            sd[idx] = s * d_cap
    out = dict(sd=sd, face=face, mask=sd < 0.0, field=quantise(sd, d_cap), u=u, d2=r['d2'], in_band=band, nodes=p)
    if signed:
        out['margin'] = r['margin']
    return out


def same_as_restatement(mine, ref, signed):
    """The equalities every implementation owes the restatement, mesh_distance_ref.same_as_restatement's rule for the signs: the
    magnitude of sd, the face and band membership bit for bit; the sign, the mask and the field wherever no sign they rest on is a
    matter of rounding -> how many nodes were compared in full."""
    bits = D.bits
    assert np.array_equal(bits(np.abs(mine['sd'])), bits(np.abs(ref['sd'])))
    assert np.array_equal(mine['face'], ref['face'])
    assert not np.signbit(mine['sd'][ref['d2'] == 0]).any()
    if not signed:
        assert not np.signbit(mine['sd']).any() and not np.asarray(mine['mask']).any()
        assert np.array_equal(mine['field'], ref['field'])
        return int(mine['sd'].size)
    # a sign is clear where the node is in band with a clear margin or at distance 0; an out-of-band node inherits: if every in-band
    # sign is clear, so is everything else
    clear_in = ~ref['in_band'] | (ref['d2'] == 0) | (ref['margin'] > D.SIGN_MARGIN)
    ok = np.ones(mine['sd'].size, bool) if clear_in.all() else (ref['in_band'] & clear_in)
    assert np.array_equal(np.signbit(mine['sd'][ok]), np.signbit(ref['sd'][ok]))
    assert np.array_equal(np.asarray(mine['mask'], bool)[ok], ref['mask'][ok])
    assert np.array_equal(np.asarray(mine['field'])[ok], ref['field'][ok])
    return int(ok.sum())


def margins_clear(ref):
    """the premise of the sweep: every in-band node has d2 == 0 or a sign margin above SIGN_MARGIN"""
    b = ref['in_band']
    return bool(((ref['d2'][b] == 0) | (ref['margin'][b] > D.SIGN_MARGIN)).all())


# ---- the inputs the tests of the restatement, of the core and of the device share -------------------------------------------------------
def cube4():
    """mesh_distance_ref.cube() scaled to [0, 4]^3"""
    v, f = D.cube()
    return ((v + 1.0) * 2.0).astype(np.float32), f


CUBE_LATTICE = (np.array([-2.5, -2.5, -2.5], np.float32), 1.0, (9, 9, 9))         # nodes on the integers -2 .. 6


def cube4_sdf(p):
    return D.box_sdf(np.asarray(p, np.float64) - 2.0, 2.0)


def nested_shells():
    """icosphere(2) at R = 10 and an inverted one at R = 5 inside it: a shell"""
    from ch_shrinkwrap_amd.trimesh import icosphere
    v0, f0 = icosphere(2, 10.0)
    v1, f1 = icosphere(2, 5.0)
    return np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, f1[:, ::-1] + len(v0)]).astype(np.int32)


def two_spheres():
    from ch_shrinkwrap_amd.trimesh import icosphere
    v0, f0 = icosphere(1, 4.0)
    return np.concatenate([v0 - [7.0, 0.3, 0.2], v0 + [7.0, 0.1, 0.4]]).astype(np.float32), np.concatenate([f0, f0 + len(v0)]).astype(np.int32)
