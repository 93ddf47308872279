"""
The inputs of tests/test_remesh_device_ref.py (CPU: the restatement reaches the branch an input is named for) and
tests/test_hip_remesh_edges.py (GPU: nw_remesh_device gives the restatement's arrays, bit for bit).  Every input has 1 300 faces or fewer.

CASES: name -> (build, kwargs) with build() -> (vertices float32, faces int32) and kwargs for remesh_device / remesh_device_ref (n, L, ...).
reference(name) runs the restatement once per process and keeps the result (read-only arrays).
"""
import functools
import time

import numpy as np

from ch_shrinkwrap_amd.trimesh import icosahedron, icosphere, subdivide
from remesh_device_ref import remesh_device_ref

CASES = {}
EXPECT = {}           # name -> log entries that must have been counted at least that often (0: must be absent), or 'n_split' ...: exactly that many


def case(name, expect=(), **kw):
    def reg(fn):
        CASES[name] = (fn, kw)
        EXPECT[name] = dict((e, 1) if isinstance(e, str) else e for e in expect)
        return fn
    return reg


def mean_edge(v, f):
    v = np.asarray(v, 'f8')
    return float(np.sqrt(((v[f] - v[np.roll(f, -1, 1)]) ** 2).sum(2)).mean())


def _f4(v, f):
    return np.ascontiguousarray(v, 'f4'), np.ascontiguousarray(f, 'i4')


# ---- dyadic inputs: integer coordinates, every midpoint of five iterations exact ----------------------------------------------------
OCT_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], 'i4')


def octahedron(s=1.0):
    return np.array([[s, 0, 0], [-s, 0, 0], [0, s, 0], [0, -s, 0], [0, 0, s], [0, 0, -s]], 'f8'), OCT_F.copy()


def cube(s=1.0):
    v = np.array([[x, y, z] for x in (-s, s) for y in (-s, s) for z in (-s, s)], 'f8')
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for a, b, c, d in q for t in ((a, b, c), (a, c, d))], 'i4')
    return v, f


def lattice(shape, nsub, s=64.0):
    v, f = shape(s)
    for _ in range(nsub):
        v, f = subdivide(v, f)
    assert (v == np.round(v)).all()
    return _f4(v, f)


def nearest_f32(edge2, factor):
    """the float32 L whose (factor * L)^2 in float64 is nearest edge2, and its two float32 neighbours"""
    L = np.float32(np.sqrt(edge2) / factor)
    c = [np.nextafter(L, np.float32(0)), L, np.nextafter(L, np.float32(np.inf))]
    c.sort(key=lambda x: abs((factor * float(x)) ** 2 - edge2))
    L = c[0]
    return [float(np.nextafter(L, np.float32(0))), float(L), float(np.nextafter(L, np.float32(np.inf)))]


# a twice subdivided octahedron of half-width 64: edges of squared length 2 * 16^2 = 512 (all of them: the faces are lattice triangles)
case('oct_lattice_finer', ['split:bid', 'flip:bid'], n=5, L=9.0)(lambda: lattice(octahedron, 2))
case('oct_lattice_coarser', ['collapse:bid_h'], n=5, L=40.0)(lambda: lattice(octahedron, 3))
# a cube's lattice has two lengths (32 along the axes, 32 sqrt 2 on the face diagonals)
case('cube_lattice_finer', ['split:bid', 'flip:dihedral'], n=5, L=14.0)(lambda: lattice(cube, 2))
case('cube_lattice_between', ['split:bid'], n=5, L=30.0)(lambda: lattice(cube, 2))          # only the diagonals are too long
case('cube_lattice_coarser', ['collapse:bid_h'], n=5, L=50.0)(lambda: lattice(cube, 3))
for _k, _L in enumerate(nearest_f32(512.0, 4.0 / 3.0)):
    case('oct_high_threshold_%d' % _k, [('n_split', 0)] if _k == 2 else ['split:bid'], n=5, L=_L)(lambda: lattice(octahedron, 2))
for _k, _L in enumerate(nearest_f32(512.0, 4.0 / 5.0)):
    case('oct_low_threshold_%d' % _k, ['collapse:bid_h'] if _k == 2 else [('n_collapse', 0)], n=5, L=_L)(lambda: lattice(octahedron, 2))


# ---- small and extreme degrees ----------------------------------------------------------------------------------------------------------
def tetrahedron():
    return _f4(np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], 'f8') * 10, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]))


case('tetrahedron_far_above', ['collapse:degree_cd_at_most_3'], n=5, L=300.0)(tetrahedron)
case('tetrahedron_far_below', ['split:bid', 'flip:degree_ab_at_most_3', 'flip:area', 'flip:max_valence'], n=5, L=4.0)(tetrahedron)
case('octahedron_far_above', ['collapse:bid_h', 'collapse:degree_cd_at_most_3'], n=5, L=300.0)(lambda: _f4(*octahedron(10.0)))
case('octahedron_far_below', ['split:bid'], n=5, L=2.5)(lambda: _f4(*octahedron(10.0)))
case('icosahedron_far_above', ['collapse:bid_h'], n=5, L=30.0)(lambda: _f4(icosahedron()[0] * 10, icosahedron()[1]))
# (2.5 and not 2.0 or 2.1: there a flip's orientation test comes within 4e-15 of a tie behind a square root; the CPU module keeps every input 1e-9 clear)
case('icosahedron_far_below', ['split:bid'], n=5, L=2.5)(lambda: _f4(icosahedron()[0] * 10, icosahedron()[1]))


def bipyramid(n, r=10.0, h=6.0):
    a = 2 * np.pi * np.arange(n) / n
    v = np.vstack([np.stack([r * np.cos(a), r * np.sin(a), 0 * a], 1), [[0, 0, h], [0, 0, -h]]])
    i = np.arange(n)
    j = (i + 1) % n
    f = np.vstack([np.stack([i, j, 0 * i + n], 1), np.stack([j, i, 0 * i + n + 1], 1)])
    return _f4(v, f)


# every edge is below 4/5 L; a rim edge lies on the 3-cycle rim - apex - rim (common == 3), a spoke's collapse adds the apex's degree
for _n, _e in ((15, ['collapse:link_3']), (16, ['collapse:link_3']), (17, ['collapse:degree_sum_above_max'])):
    case('bipyramid_%d' % _n, _e, n=5, L=16.0, max_valence=16)(functools.partial(bipyramid, _n))
# at a fine target the splits leave vertices of degree 15 and 16 behind: a flip may bring c or d to 16 = max_valence and no further
case('bipyramid_15_finer', ['flip:bid_at_max_valence', 'flip:max_valence'], n=5, L=2.0, max_valence=16)(functools.partial(bipyramid, 15))
for _n, _mv in ((60, 60), (61, 60), (60, 100), (61, 100)):
    case('bipyramid_%d_max_%d' % (_n, _mv), ['collapse:bid_h', 'flip:bid'], n=3, L=16.0, max_valence=_mv)(functools.partial(bipyramid, _n, 40.0, 6.0))
case('bipyramid_64', ['collapse:bid_h', 'flip:bid', ('collapse:frozen', 0), ('flip:frozen', 0)], n=3, L=16.0, max_valence=60)(functools.partial(bipyramid, 64, 40.0, 6.0))
case('bipyramid_65', ['collapse:frozen', 'flip:frozen'], n=3, L=16.0, max_valence=60)(functools.partial(bipyramid, 65, 40.0, 6.0))


def crown(n, r=5.0, up=10.0, top=30.0):
    """a bipyramid whose rim zigzags between z = +up and -up: the rim's edges are as long as the spokes, so at a target that splits them the apexes gain
    a degree with every rim edge (a flat rim of 64 edges is a tenth of a spoke long: splitting it takes 2 * 10^4 faces)"""
    a = 2 * np.pi * np.arange(n) / n
    v = np.vstack([np.stack([r * np.cos(a), r * np.sin(a), up * (1 - 2 * (np.arange(n) % 2))], 1), [[0, 0, top], [0, 0, -top]]])
    i = np.arange(n)
    j = (i + 1) % n
    f = np.vstack([np.stack([i, j, 0 * i + n], 1), np.stack([j, i, 0 * i + n + 1], 1)])
    return _f4(v, f)


# the rim (edges of 20) splits at 4/3 L = 16.  60 / 100: the clamp to 60 where
# the apex is at it.  64: the apex is not frozen, passes 64 with the first splits, and from then on no walk round it closes: no collapse or flip that would
# walk it gets that far (the degree tests come first: 60 is the largest max_valence there is), and the relaxation leaves it where it is.  65: frozen, and
# still c or d of the rim's splits.
case('crown_60_max_60', ['flip:max_valence'], n=1, L=12.0, max_valence=60)(functools.partial(crown, 60))
case('crown_60_max_100', ['flip:max_valence'], n=1, L=12.0, max_valence=100)(functools.partial(crown, 60))
case('crown_64', ['flip:max_valence', 'collapse:degree_sum_above_max', ('collapse:frozen', 0)], n=3, L=12.0, max_valence=60)(functools.partial(crown, 64))
case('crown_64_relax', ['flip:max_valence', ('collapse:frozen', 0)], n=1, L=12.0, max_valence=60, n_relax=1)(functools.partial(crown, 64))
case('crown_65', ['split:bid', 'collapse:frozen', 'flip:frozen'], n=1, L=12.0, max_valence=60, n_relax=1)(functools.partial(crown, 65))


# ---- admission tests ----------------------------------------------------------------------------------------------------------------------
def glued_spheres():
    """two icosahedra glued along a face (taken out of both): its three edges are a 3-cycle that is no face; one of them is made short"""
    v, f = icosahedron()
    x, y, z = f[0]
    n = np.cross(v[y] - v[x], v[z] - v[x])
    n /= np.linalg.norm(n)
    c = v[[x, y, z]].mean(0)
    w = v - 2 * ((v - c) @ n)[:, None] * n                       # mirrored in the face's plane
    ids = np.arange(12) + 12
    ids[[x, y, z]] = [x, y, z]
    g = ids[f[1:]][:, ::-1]
    vv = np.vstack([v, w]) * 10
    mid = 0.5 * (vv[x] + vv[y])
    vv[x] = mid + 0.3 * (vv[x] - mid)
    vv[y] = mid + 0.3 * (vv[y] - mid)
    ff = np.vstack([f[1:], g])
    used = np.unique(ff)
    re = np.full(24, -1)
    re[used] = np.arange(used.size)
    return _f4(vv[used], re[ff])


case('glued_spheres', ['collapse:link_3', 'flip:bid'], n=1, L=12.0)(glued_spheres)


def ellipsoid():
    v, f = icosphere(2, 10.0)
    return _f4(v * np.array([1, 1, 4.0]), f)


case('ellipsoid_1_1_4', ['collapse:long_edge', 'collapse:bid_h'], n=5, L=9.0)(ellipsoid)


def noisy(nsub, amp, seed, radius=10.0):
    v, f = icosphere(nsub, radius)
    rng = np.random.default_rng(seed)
    return _f4(v + amp * mean_edge(v, f) * rng.standard_normal(v.shape), f)


def cap_cut_off():
    v, f = icosphere(3, 100.0)
    g = f[v[f].mean(1)[:, 2] < 60.0]
    used = np.unique(g)
    re = np.full(v.shape[0], -1)
    re[used] = np.arange(used.size)
    return _f4(v[used], re[g])


def strip(n=12):
    v = np.array([[i * 0.5, (i % 2) * 1.0, 0.0] for i in range(n + 2)])
    f = np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n)])
    return _f4(v, f)


def interior_edge_between_boundary_vertices():
    """two triangles: the diagonal is interior, its ends are on the boundary"""
    v = np.array([[0, 0, 0], [10, 0, 0], [10, 10, 0], [0, 10, 0]], 'f8')
    return _f4(v, np.array([[0, 1, 2], [0, 2, 3]]))


def bow_tie():
    """two octahedra that share one vertex"""
    v, f = octahedron(10.0)
    w = v + np.array([20.0, 0, 0])
    ids = np.arange(6) + 6
    ids[1] = 0                                                  # the second one's -x corner is the first one's +x corner
    vv = np.vstack([v, w])
    ff = np.vstack([f, ids[f]])
    used = np.unique(ff)
    re = np.full(12, -1)
    re[used] = np.arange(used.size)
    return _f4(vv[used], re[ff])


def spare_slots():
    v, f = icosphere(2, 50.0)
    far = np.full((2, 3), 1e3)
    at = v.shape[0] // 2
    vv = np.vstack([far, v[:at], far, v[at:], far])
    re = np.concatenate([np.arange(at) + 2, np.arange(at, v.shape[0]) + 4])
    return _f4(vv, re[f])


case('cap_cut_off', ['split:bid', 'flip:frozen'], n=5, L=0.7 * 15.3)(cap_cut_off)
case('strip', [('n_split', 0), ('n_collapse', 0), ('n_flip', 0)], n=5, L=0.3)(strip)
case('interior_edge_between_boundary_vertices', [('n_split', 0), ('n_collapse', 0), ('n_flip', 0)], n=5, L=1.0)(interior_edge_between_boundary_vertices)
case('bow_tie', ['split:bid'], n=5, L=5.0)(bow_tie)
case('spare_slots', ['split:bid'], n=5, L=0.6 * 15.3)(spare_slots)
case('far_from_origin', ['split:bid'], n=5, L=4.0)(lambda: _f4(icosphere(2, 10.0)[0].astype('f8') + 1e6, icosphere(2)[1]))
case('flat_along_z', ['split:bid'], n=5, L=3.0)(lambda: _f4(np.array([[0, 0, 3], [16, 0, 3], [16, 8, 3], [0, 8, 3], [8, 4, 3]], 'f8'),
                                               np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]])))

# ---- many operations at once --------------------------------------------------------------------------------------------------------------
_E3 = mean_edge(*icosphere(3, 100.0))
_E2 = mean_edge(*icosphere(2, 100.0))
for _rel in (0.7, 1.6, 2.2):
    for _n in (1, 5):
        case('icosphere3_x%.2f_n%d' % (_rel, _n), n=_n, L=_rel * _E3)(lambda: icosphere(3, 100.0))
        case('noisy3_x%.2f_n%d' % (_rel, _n), n=_n, L=_rel * _E3)(lambda: noisy(3, 0.15, 11, 100.0))
# (0.45 x the mean edge: the restatement needs 3 - 6 s for icosphere(3) there -- the same surface one subdivision coarser)
for _n in (1, 5):
    case('icosphere2_x0.45_n%d' % _n, n=_n, L=0.45 * _E2)(lambda: icosphere(2, 100.0))
    case('noisy2_x0.45_n%d' % _n, n=_n, L=0.45 * _E2)(lambda: noisy(2, 0.15, 11, 100.0))
# a flip is admitted while it brings c and d to max_valence at most: at 6 and 7 nearly every flip is at that edge
for _mv in (6, 7):
    case('noisy2_max_valence_%d' % _mv, ['flip:bid_at_max_valence', 'flip:max_valence', 'collapse:degree_sum_above_max'], n=5, L=0.7 * _E2, max_valence=_mv)(lambda: noisy(2, 0.15, 11, 100.0))
for _r in (0, 1, 10):
    case('relax_%d' % _r, n=5, L=0.7 * _E2, n_relax=_r, l=0.5)(lambda: icosphere(2, 100.0))
# crumpled spheres: where the flips' geometric tests and the collapses' fold test turn candidates away
case('crumpled_a', ['collapse:fold_sign', 'collapse:fold_cosine', 'flip:dihedral', 'flip:orientation_0', 'flip:orientation_1'], n=2, L=1.0 * mean_edge(*icosphere(2, 10.0)))(lambda: noisy(2, 0.45, 3))
case('crumpled_b', ['collapse:fold_cosine', 'flip:dihedral', 'flip:skew'], n=2, L=1.3 * mean_edge(*icosphere(2, 10.0)))(lambda: noisy(2, 0.6, 5))


# ---- one operation: the smallest inputs with one edge too long or too short, or one flip that gains (tests/test_remesh_device_ref.py compares these with
# the serial host remesher as well) ---------------------------------------------------------------------------------------------------------
def one_long_edge():
    v, f = icosphere(1, 10.0)
    v = v.astype('f8')
    a, b = f[7, 0], f[7, 1]
    mid = 0.5 * (v[a] + v[b])
    s = 1.1 * (4.0 / 3.0 * mean_edge(*icosphere(1, 10.0))) / float(np.linalg.norm(v[a] - v[b]))
    v[a], v[b] = mid + s * (v[a] - mid), mid + s * (v[b] - mid)
    return _f4(v, f)


def hex_patch(rings=3):
    """equilateral triangles of edge 1 in the plane z = 0: a hexagon of `rings` rings round the origin (its rim is frozen); ids by axial coordinates"""
    ax = [(i, j) for i in range(-rings, rings + 1) for j in range(-rings, rings + 1) if abs(i + j) <= rings]
    ids = {p: k for k, p in enumerate(ax)}
    v = np.array([[i + 0.5 * j, np.sqrt(0.75) * j, 0.0] for i, j in ax])
    f = []
    for i, j in ax:
        if (i + 1, j) in ids and (i, j + 1) in ids:
            f.append([ids[i, j], ids[i + 1, j], ids[i, j + 1]])
        if (i + 1, j) in ids and (i + 1, j - 1) in ids:
            f.append([ids[i, j], ids[i + 1, j - 1], ids[i + 1, j]])
    return v, np.array(f), ids


def one_short_edge(push=0.0):
    """the edge from the origin b to its neighbour r0 (moved outwards by `push`) split a quarter of the way: a new vertex a of degree 4 and one short edge
    a - b.  Taking b into a would make edges of 1.25; taking a into b brings back b - r0 = 1 + push."""
    v, f, ids = hex_patch()
    b, r0 = ids[0, 0], ids[1, 0]
    v[r0, 0] += push
    a = v.shape[0]
    v = np.vstack([v, v[b] + 0.25 * (v[r0] - v[b])])
    g = []
    for x in f.tolist():
        if b in x and r0 in x:
            k = x.index(b) if x[(x.index(b) + 1) % 3] == r0 else x.index(r0)
            p, q, o = x[k], x[(k + 1) % 3], x[(k + 2) % 3]
            g += [[p, a, o], [a, q, o]]
        else:
            g.append(x)
    return _f4(v * 10, np.array(g))


def one_gainful_flip(z=0.0, bx=0.0):
    """the edge b - r0 at the origin flipped to r1 - r5 (degrees 7, 7 across 5, 5: flipping back gains 4), r1 and r5 drawn together so that no edge is
    too long or too short; b and r0 lifted by z fold the patch along the edge (2 atan(z / 0.5) between the two normals); bx = 0.5 puts b on the line r1 - r5: a triangle of area exactly 0"""
    v, f, ids = hex_patch()
    b, r0, r1, r5 = ids[0, 0], ids[1, 0], ids[0, 1], ids[1, -1]
    g = [x for x in f.tolist() if not (b in x and r0 in x)] + [[r1, r5, r0], [r5, r1, b]]
    v[r1, 1], v[r5, 1] = 0.62, -0.62
    v[b, 2] = v[r0, 2] = z
    v[b, 0] = bx
    return _f4(v * 10, np.array(g))


def tube(sizes, walks, side=7.0, segment=10.0):
    """a closed tube bent into a ring: cross-section s is a regular polygon of sizes[s] vertices and edge `side`, `segment` from the next; the band
    from section s (B) to s + 1 (T) is walked from the edge B0 - T0 by walks[s]: 'b' adds the face (Bi, Bi+1, Tj), 't' the face (Bi, Tj+1, Tj)"""
    n = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    big = segment * n / (2 * np.pi)
    v, f = [], []
    for s in range(n):
        m, m1 = sizes[s], sizes[(s + 1) % n]
        r = side / (2 * np.sin(np.pi / m))
        for j in range(m):
            t = 2 * np.pi * j / m + 0.5
            v.append([(big + r * np.cos(t)) * np.cos(2 * np.pi * s / n), (big + r * np.cos(t)) * np.sin(2 * np.pi * s / n), r * np.sin(t)])
        assert walks[s].count('b') == m and walks[s].count('t') == m1
        i = j = 0
        for ch in walks[s]:
            if ch == 'b':
                f.append([off[s] + i % m, off[s] + (i + 1) % m, off[(s + 1) % n] + j % m1])
                i += 1
            else:
                f.append([off[s] + i % m, off[(s + 1) % n] + (j + 1) % m1, off[(s + 1) % n] + j % m1])
                j += 1
    return _f4(np.array(v), np.array(f))


def thin_torus():
    """24 triangular cross-sections, every vertex of degree 6 (no flip gains): only the 72 edges of the cross-sections are short, and each lies on its
    cross-section, a 3-cycle that is no face"""
    return tube([3] * 24, ['btbtbt'] * 24)


def joined_tube():
    """a flip that gains although c and d are joined: the cross-section (a, c, d) is a 3-cycle that is no face; the band to the next section (b, e1, e2)
    joins b to all three, and the band from a section of four before it brings the degrees of a, b, c, d to 7, 7, 5, 7 (flipping a - b gains 2)"""
    sizes, walks = [3] * 12, ['btbtbt'] * 12
    sizes[4] = 4
    walks[3], walks[4], walks[5] = 'btbtbtt', 'bbbttbt', 'btbttb'
    return tube(sizes, walks)


def fin(theta=84.0, dist=0.5, half=0.55, rest=0.93):
    """a short edge whose collapse is turned away by the fold test alone: the face (p, q, r) at the centre of a hex patch is replaced by a vertex a of
    degree 3 that stands over the edge q - r as a fin: a and p are `dist` from the line q - r, `theta` degrees apart as seen from it, so that taking a
    into p turns the triangle (a, q, r) by theta (the other direction would make long edges).  The window between the two thresholds is 5 : 3 wide,
    so q - r is stretched to 2 * half and the patch round the four is relaxed (springs of length `rest`, in the plane) until no other edge is too
    short or too long.  p, q and r have degree 7 now: the flips of p - q and r - p would gain, so one face is taken out beyond each, which freezes
    their far vertex; the flip of q - r fails the dihedral test against the fin."""
    v, f, ids = hex_patch()
    p, q, r = ids[0, 0], ids[1, 0], ids[0, 1]
    m = 0.5 * (v[q] + v[r])
    e = (v[r] - v[q]) / np.linalg.norm(v[r] - v[q])
    to_p = (v[p] - m) / np.linalg.norm(v[p] - m)
    a = v.shape[0]
    v = np.vstack([v, m + dist * (np.cos(np.radians(theta)) * to_p + np.sin(np.radians(theta)) * np.array([0, 0, 1.0]))])
    v[q], v[r], v[p] = m - half * e, m + half * e, m + dist * to_p
    holes = [sorted([ids[1, -1], ids[2, -2], ids[2, -1]]), sorted([ids[-1, 1], ids[-2, 2], ids[-1, 2]])]
    f = np.array([x for x in f.tolist() if sorted(x) != sorted([p, q, r]) and sorted(x) not in holes] + [[p, q, a], [q, r, a], [r, p, a]])
    ed = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    free = np.ones(v.shape[0], bool)
    free[[p, q, r, a]] = False
    for _ in range(400):
        d = v[ed[:, 1]] - v[ed[:, 0]]
        n = np.linalg.norm(d, axis=1)
        g = ((n - rest) / n)[:, None] * d
        acc = np.zeros_like(v)
        np.add.at(acc, ed[:, 0], g)
        np.add.at(acc, ed[:, 1], -g)
        acc[:, 2] = 0.0
        v[free] += 0.2 * acc[free]
    return _f4(np.round(v * 10, 3), f)


_NONE = [('n_split', 0), ('n_collapse', 0), ('n_flip', 0)]
case('one_split', [('n_split', 1), ('split:bid', 1)], n=1, L=mean_edge(*icosphere(1, 10.0)))(one_long_edge)
# 4/5 L = 7 and 4/3 L = 11.67: the other edges are 7.5 to 10 long
case('one_collapse', [('n_split', 0), ('n_collapse', 1), ('n_flip', 0), ('collapse:long_edge', 1), ('collapse:bid_twin', 1)], n=1, L=8.75)(one_short_edge)
case('one_collapse_refused_long_edge', _NONE + [('collapse:long_edge', 2)], n=1, L=8.75)(functools.partial(one_short_edge, 0.22))
case('one_flip', [('n_split', 0), ('n_collapse', 0), ('n_flip', 1), ('flip:bid', 1)], n=1, L=9.6)(one_gainful_flip)
case('one_flip_refused_dihedral', _NONE + [('flip:dihedral', 1)], n=1, L=9.6)(functools.partial(one_gainful_flip, 0.4))     # 77 degrees: cosine 0.22 < 0.3
# every short edge is turned away, and nothing else is a candidate: whatever the order, the input comes back
case('thin_torus', _NONE + [('collapse:link_3', 144)], n=1, L=10.0)(thin_torus)
case('fin_fold_cosine', _NONE + [('collapse:fold_cosine', 1), ('collapse:long_edge', 1), ('flip:frozen', 2), ('flip:dihedral', 1)], n=1, L=8.8)(fin)
case('fin_fold_sign', _NONE + [('collapse:fold_sign', 1), ('collapse:long_edge', 1), ('flip:frozen', 2), ('flip:dihedral', 1)], n=1, L=9.0)(functools.partial(fin, 95.0, 0.48))
# (a triangle of area 0 has two edges that together are as long as the third: at this target they are short, and every collapse would make a long edge)
case('flip_no_area', _NONE + [('flip:no_area', 1), ('collapse:long_edge', 8)], n=1, L=12.0)(functools.partial(one_gainful_flip, 0.0, 0.5))
ONE_OPERATION = ['one_split', 'one_collapse', 'one_collapse_refused_long_edge', 'one_flip', 'one_flip_refused_dihedral', 'thin_torus', 'fin_fold_cosine',
                 'fin_fold_sign', 'flip_no_area']
case('joined_tube', ['flip:already_joined', 'flip:bid'], n=1, L=10.0)(joined_tube)


@functools.lru_cache(maxsize=None)
def inputs(name):
    v, f = CASES[name][0]()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def kwargs(name):
    return dict(CASES[name][1])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(vertices, faces, info, seconds) of the restatement, computed once"""
    v, f = inputs(name)
    t0 = time.perf_counter()
    rv, rf, info = remesh_device_ref(v, f, **kwargs(name))
    dt = time.perf_counter() - t0
    rv.setflags(write=False)
    rf.setflags(write=False)
    return rv, rf, info, dt
