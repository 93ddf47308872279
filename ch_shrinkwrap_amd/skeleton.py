"""
The centreline graph of a fitted network: the level-set diagram of a scalar field on the mesh.  ctypes binding of include/nw_skeleton.h
(kernels in libnanowrap_hip.so, csrc/nw_skeleton.hip) and what sits on top of it.

How many tubes, how long, how thick, how many junctions and loops, and where the centreline runs: upstream answers with
SkeletonizeMembrane (recipe_modules/surface_feature_extraction.py), mean-curvature flow with Voronoi poles and a remesher of its own.
That method is iterative, needs scipy's Voronoi and is not a function of its input; it is not mirrored.  What is computed here is the
classical level-set diagram (a Reeb graph over bands of a field): the surface is cut into bands {k w <= D < (k + 1) w} of a per-vertex
field D, every connected piece of a band is a node, pieces of neighbouring bands that touch are joined by an arc, a node sits at the
centre of its cross-section contour, and the contour's perimeter gives the tube's radius.  The definition is this project's own and is
written down in csrc/nw_skeleton_core.h; tests/mesh_skeleton_ref.py restates it in NumPy.

WHAT THIS SKELETON IS NOT.  IT IS A LEVEL-SET DIAGRAM OF ONE FIELD, not a medial axis and not upstream's curve skeleton.  It depends on
the field and so on the source the field was grown from.  A sheet becomes a chain.  LOOPS NARROWER THAN A BAND VANISH: on a 24 x 12 torus
(R = 3, r = 1) with a graph-distance field the loop is there at band widths of 0.3, 1 and 2 mean edge lengths and gone at 4.  "Exact"
means: a function of the input alone, equal bit for bit to the restatement, whatever the launch geometry or the order of the atomics.

  the exact layer
    SkeletonContext       one nwa_ctx: set_mesh once, level_sets as often as needed (another field, another band width)
    level_set_skeleton    one call: a mesh and a field (or sources, or nothing) in; nodes, arcs, vertex_node, the raw integer tables out
  on top of it: host float64 arithmetic with no exactness claim
    skeleton_graph        degree, ends, junctions, branches with length and mean radius, loops, components; pruning of short end branches
    branch_of_vertex      which branch a vertex belongs to
  recipe-module surface
    SkeletonizeMembrane   a mesh -> a table of nodes and a table of branches

Everything that joins pieces runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwa_abi_version', 'nwa_create', 'nwa_destroy', 'nwa_last_error', 'nwa_set_mesh', 'nwa_skeleton', 'nwa_fetch']
ABI_VERSION = 1
NWA_OK, NWA_ERR_BADARG, NWA_ERR_HIP, NWA_ERR_NONFINITE, NWA_ERR_NOMEM, NWA_ERR_NOMESH, NWA_ERR_NORESULT = 0, -1, -2, -3, -4, -5, -6
ERRORS = {NWA_ERR_BADARG: 'bad argument', NWA_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWA_ERR_NONFINITE: 'non-finite position',
          NWA_ERR_NOMEM: 'out of device memory', NWA_ERR_NOMESH: 'the context holds no mesh yet', NWA_ERR_NORESULT: 'the context holds no result yet'}
NWA_FLAG_TIMING = 1
NWA_INFO_WORDS = 24
INFO_NAMES = ('pieces', 'nodes', 'arcs', 'live_faces', 'live_vertices', 'segments', 'max_band', 'arc_keys', 'hook_retries', 'atomics', 'bands_us',
              'scan_us', 'init_us', 'hook_us', 'compress_us', 'sums_us', 'arcs_us', 'vertex_us', 'keys_download_us', 'dedup_us', 'upload_us')
NWA_SUM_COLUMNS = 12
(S_PIECES, S_CENTROID, S_SEGMENTS, S_LENGTH, S_MOMENT_LO, S_MOMENT_HI) = (0, 1, 4, 5, 6, 9)
COORD_BITS = 20
LEN_SHIFT = 10
MAX_N = 1 << 30
MAX_FACES = 1 << 29
MAX_BAND = 1 << 30
MAX_PIECES = 1 << 28
# the info entries that depend on the order in which the hardware runs workgroups, or on the clock: in no bit comparison
NOT_DETERMINISTIC = ('hook_retries', 'atomics') + tuple(n for n in INFO_NAMES if n.endswith('_us'))

_L = None


def load():
    """The library's nwa_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwa_abi_version': [], 'nwa_create': [i32, ctypes.POINTER(vp)], 'nwa_destroy': [vp], 'nwa_last_error': [vp],
            'nwa_set_mesh': [vp, vp, i64, vp, i64, vp, i32, vp], 'nwa_skeleton': [vp, vp, i32, f64, i32, vp], 'nwa_fetch': [vp] * 7},
            'nwa_abi_version', ABI_VERSION, 'nw_skeleton')
    return _L


_p = _lib.ptr


def _is_device(a):
    return isinstance(a, tuple) and len(a) == 2 and isinstance(a[0], (int, np.integer))


def nodes_from_sums(node_sums, node_band, low, q):
    """The nodes' float64 attributes from their integer sums (host arithmetic, no exactness claim): position = the contour's centroid
    (segment midpoints weighted by their lengths) where the node has a contour, else the mean of its faces' centroids; perimeter = the
    contour's length; radius = perimeter / 2 pi.  Positions are within q / 2 per axis of the same means of the unquantised points."""
    S = np.asarray(node_sums, np.uint64).reshape(-1, NWA_SUM_COLUMNS).astype(np.float64)
    low, q = np.asarray(low, np.float64), float(q)
    n, length = S[:, S_PIECES], S[:, S_LENGTH]
    moment = S[:, S_MOMENT_HI:S_MOMENT_HI + 3] * 4294967296.0 + S[:, S_MOMENT_LO:S_MOMENT_LO + 3]
    with np.errstate(invalid='ignore', divide='ignore'):
        contour = moment / (2.0 * length[:, None])
        mean = S[:, S_CENTROID:S_CENTROID + 3] / (3.0 * n[:, None])
    perimeter = length * (q / float(1 << LEN_SHIFT))
    return dict(position=np.where((length > 0)[:, None], contour, mean) * q + low, radius=perimeter / (2.0 * np.pi), perimeter=perimeter,
                band=np.asarray(node_band, np.int32), n_pieces=n.astype(np.int64), n_segments=S[:, S_SEGMENTS].astype(np.int64))


class SkeletonContext(_lib.QueryContext):
    """One nwa_ctx: a mesh taken in once by set_mesh and kept on the device, and any number of level-set diagrams on it."""
    prefix, errors, gpu_only, load = 'nwa_', ERRORS, 'the level-set skeleton runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_vertices = self.n_faces = 0
        self.low, self.q = np.zeros(3), 1.0

    def set_mesh(self, vertices, faces, twin):
        """Take a float32 mesh in.  vertices: (V,3) on the host, or (device pointer, V).  twin: int32 (3F,), -1 on a border, mutual: a
        mesh with a non-manifold edge has none and is refused."""
        if _is_device(vertices):
            pos, n, on_device = _p(int(vertices[0])), int(vertices[1]), 1
        else:
            keep = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
            pos, n, on_device = _p(keep), keep.shape[0], 0
        faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        if twin is None:
            raise ValueError('the level-set skeleton needs the half-edge twins')
        tw = np.ascontiguousarray(twin, np.int32).ravel()
        if tw.size != 3 * faces.shape[0]:
            raise ValueError('twin must have three entries per face')
        self.n_vertices = self.n_faces = 0
        quantum = np.zeros(4)
        self.check(self.L.nwa_set_mesh(self.h, pos, n, _p(faces), faces.shape[0], _p(tw), on_device, _p(quantum)), 'nwa_set_mesh')
        self.n_vertices, self.n_faces, self.low, self.q = n, faces.shape[0], quantum[:3].copy(), float(quantum[3])
        return self

    def level_sets(self, field, band_width, timing=False):
        """The level-set diagram of one field on the mesh at hand -> dict(piece_start (F+1,), piece_node (P,), vertex_node (V,), node_band
        (N,), node_sums (N,12) uint64, arcs (A,2), low, q, info): the exact layer, integers only.
        field: (V,) float64 on the host, finite or +inf (dead), or (device pointer, V).  band_width > 0.
        A LEVEL-SET DIAGRAM OF ONE FIELD: it depends on the field's source, and a loop narrower than a band vanishes.
        info: hook_retries, atomics and the *_us entries depend on the hardware's scheduling or on the clock, ARE NOT DETERMINISTIC and
        belong in no comparison (NOT_DETERMINISTIC); the *_us entries are filled with timing=True, which waits after every stage."""
        if not self.n_vertices:
            raise RuntimeError('nwa_skeleton: %s' % ERRORS[NWA_ERR_NOMESH])
        if _is_device(field):
            if int(field[1]) != self.n_vertices:
                raise ValueError('the field has one value per vertex')
            fp, on_device = _p(int(field[0])), 1
        else:
            keep = np.ascontiguousarray(field, np.float64).reshape(-1)
            if keep.size != self.n_vertices:
                raise ValueError('the field has one value per vertex')
            fp, on_device = _p(keep), 0
        words = np.zeros(NWA_INFO_WORDS, np.int64)
        self.check(self.L.nwa_skeleton(self.h, fp, on_device, float(band_width), NWA_FLAG_TIMING if timing else 0, _p(words)), 'nwa_skeleton')
        info = dict((name, int(words[i])) for i, name in enumerate(INFO_NAMES))
        P, N, A = info['pieces'], info['nodes'], info['arcs']
        out = dict(piece_start=np.zeros(self.n_faces + 1, np.int32), piece_node=np.zeros(P, np.int32), vertex_node=np.zeros(self.n_vertices, np.int32),
                   node_band=np.zeros(N, np.int32), node_sums=np.zeros((N, NWA_SUM_COLUMNS), np.uint64), arcs=np.zeros((A, 2), np.int32))
        self.check(self.L.nwa_fetch(self.h, _p(out['piece_start']), _p(out['piece_node']), _p(out['vertex_node']), _p(out['node_band']), _p(out['node_sums']),
                                    _p(out['arcs'])), 'nwa_fetch')
        out.update(low=self.low.copy(), q=self.q, info=info)
        return out


def _vertex_components(n_vertices, faces):
    """label[v] = the smallest vertex id of v's component of the edge graph (host; min-label propagation with pointer jumping)"""
    lab = np.arange(n_vertices)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    while True:
        m = np.minimum(lab[e[:, 0]], lab[e[:, 1]])
        new = lab.copy()
        np.minimum.at(new, e[:, 0], m)
        np.minimum.at(new, e[:, 1], m)
        new = new[new]
        if (new == lab).all():
            return lab
        lab = new


def double_sweep_field(mesh_arrays, device=0):
    """The default field: per component of the mesh the geodesic graph distance (geodesic.geodesic_distance) from the vertex farthest
    from the component's smallest vertex id.  Vertices no face holds are dead (+inf).  -> (field, sources)"""
    from .geodesic import GeodesicContext
    pos, faces, twin = mesh_arrays
    lab = _vertex_components(pos.shape[0], faces)
    used = np.zeros(pos.shape[0], bool)
    used[faces.reshape(-1)] = True
    first = np.unique(lab[used]).astype(np.int32)
    ctx = GeodesicContext(device)
    try:
        ctx.set_mesh(pos, faces, twin)
        d = ctx.distances(first)['distance']
        far = np.empty(first.size, np.int32)
        for i, s in enumerate(first):                             # the farthest vertex of each component, the smallest id among equals
            members = np.flatnonzero((lab == s) & used)
            far[i] = members[np.argmax(d[members])]
        return ctx.distances(far)['distance'], far
    finally:
        ctx.close()


def level_set_skeleton(mesh, field=None, band_width=None, sources=None, context=None, device=0):
    """The centreline graph of a mesh -> dict(nodes=dict(position, radius, perimeter, band, n_pieces, n_segments), arcs (A,2), vertex_node
    (V,), piece_start, piece_node, raw (the integer tables: node_sums, node_band, low, q), info, field, band_width).
    mesh: a TriMesh, a MembraneMesh or a (vertices, faces) pair; a mesh with a non-manifold edge raises, border edges are fine.
    field: a per-vertex float64 array, finite or +inf (dead).  None: the geodesic graph distance (geodesic.geodesic_distance) from
    `sources`; with sources=None too, a double sweep per mesh component: from the smallest vertex id of each component, then from the
    farthest vertex found.  band_width=None: twice the mean edge length.
    THIS IS A LEVEL-SET DIAGRAM OF ONE FIELD, not a medial axis: it depends on the source, a sheet becomes a chain, and LOOPS NARROWER THAN A
    BAND VANISH.  nodes, arcs and vertex_node come from the exact layer; nodes' float attributes are host arithmetic on exact integer sums.
    context: a SkeletonContext to use (it holds the mesh afterwards); one is made and closed otherwise."""
    from .distance import _mesh_arrays
    pos, faces, twin = _mesh_arrays(mesh, True)
    if band_width is None:
        from .isosurface import mean_edge_length
        band_width = 2.0 * mean_edge_length(pos, faces)
    if not (float(band_width) > 0 and np.isfinite(float(band_width))):
        raise ValueError('the band width must be positive and finite')
    own = context is None
    ctx = SkeletonContext(device) if own else context
    try:
        ctx.set_mesh(pos, faces, twin)
        if field is None:
            if sources is None:
                field, sources = double_sweep_field((pos, faces, twin), device)
            else:
                from .geodesic import geodesic_distance
                field = geodesic_distance((pos, faces), sources, device=device)['distance']
        raw = ctx.level_sets(field, band_width)
    finally:
        if own:
            ctx.close()
    return dict(nodes=nodes_from_sums(raw['node_sums'], raw['node_band'], raw['low'], raw['q']), arcs=raw['arcs'], vertex_node=raw['vertex_node'],
                piece_start=raw['piece_start'], piece_node=raw['piece_node'],
                raw=dict(node_sums=raw['node_sums'], node_band=raw['node_band'], low=raw['low'], q=raw['q']), info=raw['info'],
                field=None if _is_device(field) else np.asarray(field, np.float64), band_width=float(band_width), sources=sources)


# ---- on top of it: host float64 arithmetic with no exactness claim -------------------------------------------------------------------
def _graph_components(n, arcs):
    lab = np.arange(n)
    a = np.asarray(arcs, np.int64).reshape(-1, 2)
    while a.size:
        m = np.minimum(lab[a[:, 0]], lab[a[:, 1]])
        new = lab.copy()
        np.minimum.at(new, a[:, 0], m)
        np.minimum.at(new, a[:, 1], m)
        new = new[new]
        if (new == lab).all():
            break
        lab = new
    return lab


def _branches(n, arcs, keep, position, radius):
    """maximal chains of degree-2 nodes between nodes of any other degree, and the cycles without such a node"""
    nbr = [[] for _ in range(n)]
    for a, b in np.asarray(arcs).tolist():
        nbr[a].append(b)
        nbr[b].append(a)
    degree = np.array([len(x) for x in nbr], np.int64)
    seen = set()
    out = []

    def walk(start, nxt):
        chain = [start, nxt]
        seen.add((min(start, nxt), max(start, nxt)))
        while degree[chain[-1]] == 2 and chain[-1] != start:
            a, b = nbr[chain[-1]]
            step = b if a == chain[-2] else a
            seen.add((min(chain[-1], step), max(chain[-1], step)))
            chain.append(step)
        return chain
    for s in np.flatnonzero((degree != 2) & keep).tolist():
        for t in nbr[s]:
            if (min(s, t), max(s, t)) not in seen:
                out.append(walk(s, t))
    for s in np.flatnonzero((degree == 2) & keep).tolist():       # what is left are cycles of degree-2 nodes
        t = nbr[s][0]
        if (min(s, t), max(s, t)) not in seen:
            out.append(walk(s, t))
    res = []
    for chain in out:
        c = np.array(chain, np.int64)
        r = radius[c]
        r = r[r > 0]
        res.append(dict(nodes=c, ends=(int(c[0]), int(c[-1])), length=float(np.sqrt(((position[c[1:]] - position[c[:-1]]) ** 2).sum(1)).sum()),
                        mean_radius=float(r.mean()) if r.size else float('nan')))
    return degree, res


def skeleton_graph(result, prune=0.0):
    """What is asked of the graph of level_set_skeleton's result -> dict(degree (N,), ends, junctions, isolated (node ids), branches (a list
    of dict(nodes, ends, length, mean_radius)), n_branches, total_length, n_loops = arcs - nodes + components, n_components, kept (N,) bool,
    arcs (the arcs that are left)).  A branch is a maximal chain of degree-2 nodes with the two nodes that end it (or a closed cycle);
    its length runs along the node positions, its mean radius is over its nodes that have a contour.
    prune > 0 drops, repeatedly, every end branch (one end of degree 1, the other a junction) that is shorter than prune x its junction's
    radius; the loop count does not change by that.  Host float64 code on top of the exact layer: no exactness claim."""
    nodes = result['nodes']
    position, radius = np.asarray(nodes['position'], np.float64), np.asarray(nodes['radius'], np.float64)
    n = position.shape[0]
    arcs = np.asarray(result['arcs'], np.int64).reshape(-1, 2)
    keep = np.ones(n, bool)
    while True:
        degree, branches = _branches(n, arcs, keep, position, radius)
        if not prune > 0:
            break
        drop = np.zeros(n, bool)
        for b in branches:
            for end, other in (b['ends'], b['ends'][::-1]):
                if degree[end] == 1 and degree[other] >= 3 and b['length'] < prune * radius[other]:
                    drop[b['nodes'][b['nodes'] != other]] = True
        if not drop.any():
            break
        keep &= ~drop
        arcs = arcs[keep[arcs[:, 0]] & keep[arcs[:, 1]]]
    lab = _graph_components(n, arcs)
    n_nodes = int(keep.sum())
    n_components = int(np.unique(lab[keep]).size)
    return dict(degree=np.where(keep, degree, -1), ends=np.flatnonzero(keep & (degree == 1)), junctions=np.flatnonzero(keep & (degree >= 3)),
                isolated=np.flatnonzero(keep & (degree == 0)), branches=branches, n_branches=len(branches),
                total_length=float(sum(b['length'] for b in branches)), n_loops=int(arcs.shape[0] - n_nodes + n_components), n_components=n_components,
                kept=keep, arcs=arcs.astype(np.int32))


def branch_of_vertex(result, graph):
    """(V,) int32: the branch (index into graph['branches']) of the node a vertex belongs to; -1 for a dead vertex, for a vertex of a
    junction node (it belongs to several) and for one whose node was pruned.  Host code, no exactness claim."""
    n = np.asarray(result['nodes']['position']).shape[0]
    of_node = np.full(n + 1, -1, np.int32)
    for i, b in enumerate(graph['branches']):
        inner = b['nodes'][graph['degree'][b['nodes']] <= 2]
        of_node[inner] = i
    of_node[n] = -1
    vn = np.asarray(result['vertex_node'], np.int64)
    return of_node[np.where(vn >= 0, vn, n)]


# ---- recipe-module surface ----------------------------------------------------------------------------------------------------------------
class SkeletonizeMembrane(object):
    """Recipe-module surface for the centreline graph of a fit.  It keeps upstream's name (recipe_modules/surface_feature_extraction.py) and
    none of its method: upstream contracts the mesh by mean-curvature flow with Voronoi poles; this is the level-set diagram of the
    geodesic graph distance (level_set_skeleton), so its parameters are its own.  The mesh under `input` -> under `output_nodes` a table
    with one row per node: x y z radius perimeter band degree branch, and under `output_branches` one row per branch: start end length
    mean_radius n_nodes.  The node table's metadata carries arcs, n_loops, n_components, band_width and info.
    A level-set diagram of one field: it depends on the source, a sheet becomes a chain, loops narrower than a band vanish."""

    def __init__(self, **kw):
        self.input, self.output_nodes, self.output_branches = 'membrane', 'skeleton_nodes', 'skeleton_branches'
        self.band_width = None                # None: twice the mean edge length
        self.sources = None                   # None: a double sweep per component
        self.prune = 0.0
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        r = level_set_skeleton(namespace[self.input], band_width=self.band_width, sources=self.sources, device=self.device)
        g = skeleton_graph(r, prune=float(self.prune))
        n = r['nodes']
        branch = np.full(n['position'].shape[0], -1, np.int32)
        for i, b in enumerate(g['branches']):
            branch[b['nodes'][g['degree'][b['nodes']] <= 2]] = i
        nodes = {'x': n['position'][:, 0], 'y': n['position'][:, 1], 'z': n['position'][:, 2], 'radius': n['radius'], 'perimeter': n['perimeter'],
                 'band': n['band'], 'degree': g['degree'], 'branch': branch,
                 'metadata': {'arcs': g['arcs'], 'n_loops': g['n_loops'], 'n_components': g['n_components'], 'band_width': r['band_width'], 'prune': float(self.prune),
                              'info': r['info']}}
        B = g['branches']
        branches = {'start': np.array([b['ends'][0] for b in B], np.int32), 'end': np.array([b['ends'][1] for b in B], np.int32),
                    'length': np.array([b['length'] for b in B], np.float64), 'mean_radius': np.array([b['mean_radius'] for b in B], np.float64),
                    'n_nodes': np.array([b['nodes'].size for b in B], np.int32)}
        namespace[self.output_nodes], namespace[self.output_branches] = nodes, branches
        return nodes, branches
