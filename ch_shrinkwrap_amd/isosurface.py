"""
The start surface of a fit from the localization cloud itself: ctypes binding of include/nw_isosurface.h (count per voxel, integer
binomial smoothing, threshold from the median of the occupied voxels, sheet-aware surface nets -- all kernels in libnanowrap_hip.so) and
what stands in for the first two modules of upstream's recipe (ch_shrinkwrap/test_evaluation_recipe.yaml:25-38):

    pointcloud.Octree -> surface_fitting.DualMarchingCubes(threshold_density, remesh) -> surface_fitting.ShrinkwrapMembrane

Octree and DualMarchingCubes are PYME's and not in the reference tree; this is NOT their algorithm.  It differs in three ways: a regular
grid instead of an octree, one fixed bandwidth (`passes` rounds of [1 2 1] at one voxel size) instead of a density estimate that adapts
to the local number of points, and one resolution for the whole surface.  `threshold_density` keeps upstream's meaning (localizations
per nm^3).

    density_isosurface   cloud -> (vertices, faces, info): the raw isosurface, outer and inner sheets alike
    knn_isosurface       the same from the k-NN density (neighbours.py): the bandwidth follows (threshold_density, n_points_min) or the
                         cloud's own density, and the voxel size is resolution only
    start_surface        ... then the inner sheets and dust dropped (surgery.inner_components) and the mesh remeshed (remesh_device)
    DensitySurface       the recipe-module mirror: DensitySurface().execute(ns); ShrinkwrapMembrane().execute(ns)

There is no CPU fallback: without a GPU every one of them raises RuntimeError.  tests/isosurface_ref.py restates the kernels in NumPy.
"""
import ctypes
import time

import numpy as np

from . import _lib

SYMBOLS = ['nwi_abi_version', 'nwi_create', 'nwi_destroy', 'nwi_last_error', 'nwi_set_sheet_table', 'nwi_density', 'nwi_threshold_auto',
           'nwi_extract', 'nwi_get', 'nwi_set_field']
ABI_VERSION = 1
MAX_PASSES = 5
(NWI_OK, NWI_ERR_BADARG, NWI_ERR_HIP, NWI_ERR_NONFINITE, NWI_ERR_NOMEM, NWI_ERR_OUTSIDE, NWI_ERR_STATE, NWI_ERR_BORDER,
 NWI_ERR_EMPTY) = 0, -1, -2, -3, -4, -5, -6, -7, -8
ERRORS = {NWI_ERR_BADARG: 'bad argument', NWI_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWI_ERR_NONFINITE: 'non-finite localization',
          NWI_ERR_NOMEM: 'out of device memory', NWI_ERR_OUTSIDE: 'localization outside the grid', NWI_ERR_STATE: 'call out of order',
          NWI_ERR_BORDER: 'the surface touches the border of the grid', NWI_ERR_EMPTY: 'nothing above the threshold'}

_L = None


def load():
    """The library's nwi_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f32, f64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_uint64
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwi_abi_version': [], 'nwi_create': [i32, ctypes.POINTER(vp)], 'nwi_destroy': [vp], 'nwi_last_error': [vp],
            'nwi_set_sheet_table': [vp, vp],
            'nwi_density': [vp, vp, i64, i32, vp, f32, vp, i32, vp, vp],
            'nwi_threshold_auto': [vp, f64, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(f64), ctypes.POINTER(i64)],
            'nwi_extract': [vp, u64, ctypes.POINTER(i64), ctypes.POINTER(i64)],
            'nwi_get': [vp, vp, vp, vp],
            'nwi_set_field': [vp, vp, i32, vp, f32, vp]}, 'nwi_abi_version', ABI_VERSION, 'nw_isosurface')
    return _L


_p = _lib.ptr


def sheet_table():
    """The 256 x 12 int8 sheet table the kernels are handed: synth._sheet_labels(), the one table both meshers use."""
    from .synth import _SHEET
    return np.ascontiguousarray(_SHEET, np.int8)


def grid_for(points, h, pad):
    """(lo (3,) float32, dims (3,) int32) of the voxel grid of a cloud: the bounding box, snapped to multiples of h, with `pad` voxels on
    every side.  Computed in float64 and rounded once: the kernels and any reference are handed the same numbers."""
    p = np.asarray(points).reshape(-1, 3)
    if p.shape[0] == 0 or not np.isfinite(p).all():
        raise ValueError('grid_for: the cloud is empty or holds a non-finite localization')
    h = float(h)
    if not (h > 0 and np.isfinite(h)) or int(pad) < 1:
        raise ValueError('grid_for: voxel size must be positive and pad at least 1')
    mn, mx = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    lo = ((np.floor(mn / h) - int(pad)) * h).astype(np.float32)
    dims = (np.floor((mx - lo.astype(np.float64)) / h).astype(np.int64) + 1 + int(pad)).astype(np.int32)
    return lo, dims


def pick_voxel_size(points, sigma=None):
    """The voxel size when none is given.  With localization errors: their median (10 nm for a typical error_x; the [1 2 1] passes then
    smooth over a few sigma).  Without: the smallest of h0 * 1.25^k, h0 = (bounding-box volume / N)^(1/3), at which an occupied voxel
    holds at least 4 localizations on average.  A rule, not a tuned value."""
    if sigma is not None:
        s = np.asarray(sigma, np.float64)
        s = s[np.isfinite(s) & (s > 0)]
        if s.size:
            return float(np.median(s))
    p = np.asarray(points, np.float64).reshape(-1, 3)
    ext = np.maximum(p.max(0) - p.min(0), 1e-3 * max(float((p.max(0) - p.min(0)).max()), 1e-6))
    h = float(np.cbrt(ext.prod() / p.shape[0]))
    for _ in range(40):
        v = np.floor((p - p.min(0)) / h).astype(np.int64)
        occupied = np.unique((v[:, 2] * (v[:, 1].max() + 1) + v[:, 1]) * (v[:, 0].max() + 1) + v[:, 0]).size
        if p.shape[0] >= 4 * occupied:
            break
        h *= 1.25
    return h


class IsosurfaceContext(_lib.QueryContext):
    """One nwi_ctx: the density field of one cloud on one device and the surface nets of its level sets."""
    prefix, errors, gpu_only, load = 'nwi_', ERRORS, 'the density isosurface runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.dims = self.h_voxel = self.passes = None
        tab = sheet_table()
        self.check(self.L.nwi_set_sheet_table(self.h, _p(tab)), 'nwi_set_sheet_table')

    def density(self, points, lo, h, dims, passes=2, return_field=False, return_counts=False):
        """Count and smooth.  points: (N,3) host array, or a raw device pointer with `n_points` as a tuple (ptr, n).  Returns the
        uint64 field (and the uint32 counts), [z, y, x], if asked for; the field stays on the device either way."""
        lo = np.ascontiguousarray(lo, np.float32).reshape(3)
        dims = np.ascontiguousarray(dims, np.int32).reshape(3)
        if isinstance(points, tuple):
            src, n, on_device = int(points[0]), int(points[1]), 1
        else:
            pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            src, n, on_device = pts, pts.shape[0], 0
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        field = np.empty(shape, np.uint64) if return_field else None
        counts = np.empty(shape, np.uint32) if return_counts else None
        self.check(self.L.nwi_density(self.h, _p(src), n, on_device, _p(lo), float(h), _p(dims), int(passes), _p(field), _p(counts)), 'nwi_density')
        self.dims, self.h_voxel, self.passes = dims, float(np.float32(h)), int(passes)
        return (field, counts) if return_field and return_counts else field if return_field else counts

    def set_field(self, field, lo, h, dims):
        """Adopt a field made elsewhere, by copy: a uint64 host array [z, y, x], or a raw device pointer (an int) to dims[2] x dims[1] x
        dims[0] values.  extract works on it; threshold_auto does not (there are no counts) until the next density."""
        lo = np.ascontiguousarray(lo, np.float32).reshape(3)
        dims = np.ascontiguousarray(dims, np.int32).reshape(3)
        if isinstance(field, (int, np.integer)):
            src, on_device = int(field), 1
        else:
            src, on_device = np.ascontiguousarray(field, np.uint64), 0
            if src.shape != (int(dims[2]), int(dims[1]), int(dims[0])):
                raise ValueError('set_field: the field must be indexed [z, y, x] with the shape of dims')
        self.check(self.L.nwi_set_field(self.h, _p(src), on_device, _p(lo), float(h), _p(dims)), 'nwi_set_field')
        self.dims, self.h_voxel, self.passes = dims, float(np.float32(h)), 0

    def threshold_auto(self, fraction=0.3):
        """dict(median, thr (field values), threshold_density (nm^-3), n_occupied): thr = floor(fraction * lower median of the field over
        the occupied voxels)."""
        med, thr, dens, occ = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double(), ctypes.c_int64()
        self.check(self.L.nwi_threshold_auto(self.h, float(fraction), ctypes.byref(med), ctypes.byref(thr), ctypes.byref(dens), ctypes.byref(occ)),
                   'nwi_threshold_auto')
        return dict(median=int(med.value), thr=int(thr.value), threshold_density=float(dens.value), n_occupied=int(occ.value))

    def extract(self, thr, return_keys=False):
        """(vertices (V,3) float32, faces (F,3) int32[, keys (V,) int64]) of `field > thr`."""
        nv, nf = ctypes.c_int64(), ctypes.c_int64()
        self.check(self.L.nwi_extract(self.h, int(thr), ctypes.byref(nv), ctypes.byref(nf)), 'nwi_extract')
        v = np.empty((nv.value, 3), np.float32)
        f = np.empty((nf.value, 3), np.int32)
        k = np.empty(nv.value, np.int64) if return_keys else None
        self.check(self.L.nwi_get(self.h, _p(v), _p(f), _p(k)), 'nwi_get')
        return (v, f, k) if return_keys else (v, f)


def field_scale(h, passes):
    """field value = density (nm^-3) * field_scale: the weights of `passes` rounds of [1 2 1] along three axes sum to 4^(3 passes)"""
    h = float(np.float32(h))
    return float(4 ** (3 * int(passes))) * h * h * h


def density_isosurface(points, voxel_size=None, passes=2, threshold_density=None, threshold_fraction=0.3, pad=None, device=0, sigma=None):
    """(vertices float32, faces int32, info) of the isosurface of the smoothed localization density.

    voxel_size None: pick_voxel_size(points, sigma).  threshold_density (nm^-3, upstream's DualMarchingCubes.threshold_density) None:
    threshold_fraction x the median density of the occupied voxels.  pad: voxels of margin on every side, default passes + 3 (the
    smoothed field reaches `passes` voxels beyond the outermost localization).  The surface is closed and oriented, and manifold on a
    smoothed density (include/nw_isosurface.h says when not); it has an inner sheet (inverted, of negative volume) wherever the cloud is
    a shell: start_surface drops those."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    passes = int(passes)
    if not 0 <= passes <= MAX_PASSES:
        raise ValueError('passes must be in 0..%d' % MAX_PASSES)
    h = float(np.float32(pick_voxel_size(pts, sigma) if voxel_size is None else voxel_size))
    pad = passes + 3 if pad is None else int(pad)
    lo, dims = grid_for(pts, h, pad)
    ctx = IsosurfaceContext(device)
    try:
        t0 = time.time()
        ctx.density(pts, lo, h, dims, passes)
        if threshold_density is None:
            t = ctx.threshold_auto(threshold_fraction)
        else:
            thr = int(np.floor(float(threshold_density) * field_scale(h, passes)))
            t = dict(median=None, thr=thr, threshold_density=thr / field_scale(h, passes), n_occupied=None)
        v, f = ctx.extract(t['thr'])
        dt = time.time() - t0
    finally:
        ctx.close()
    info = dict(lo=lo, h=h, dims=dims, passes=passes, pad=pad, thr=t['thr'], threshold_density=t['threshold_density'], median=t['median'],
                n_occupied=t['n_occupied'], seconds=dt)
    return v, f, info


def knn_threshold(h, n_points_min, threshold_density):
    """(R_thr, r_cap, pad, thr) of the level set of the k-NN density k / (4/3 pi r_k^3) at threshold_density on a lattice of spacing h:
    R_thr = (3 k / (4 pi threshold_density))^(1/3) is where r_k crosses; r_cap = R_thr + 2 h is where the field is clamped (r_k is
    1-Lipschitz, so the outer node of every crossed lattice edge lies below the cap and is not clamped); pad = ceil(R_thr / h) + 2
    voxels of margin keep every border node more than R_thr from the cloud, hence outside; thr = floor((r_cap - R_thr) 2^20) is the
    level in the field's units."""
    k, td, h = int(n_points_min), float(threshold_density), float(h)
    if not (td > 0 and np.isfinite(td)):
        raise ValueError('knn_isosurface: threshold_density must be positive and finite (is the cloud k + 1 coincident points?)')
    R_thr = float(np.cbrt(3.0 * k / (4.0 * np.pi * td)))
    r_cap = R_thr + 2.0 * h
    return R_thr, r_cap, int(np.ceil(R_thr / h)) + 2, int(np.floor((r_cap - R_thr) * float(1 << 20)))


def knn_isosurface(points, voxel_size=None, n_points_min=20, threshold_density=None, threshold_fraction=0.3, device=0, sigma=None):
    """(vertices float32, faces int32, info) of the isosurface of the k-NN density of the cloud, k = n_points_min (upstream's
    Octree.n_points_min): the level set r_k(x) = R_thr of the distance to the k-th nearest localization, which is where a ball of
    radius R_thr holds k localizations.  The bandwidth R_thr follows (threshold_density, n_points_min) and not the voxel size, which is
    resolution only.  threshold_density (nm^-3, upstream's DualMarchingCubes.threshold_density) None: threshold_fraction x the median
    of neighbours.local_density(points, n_points_min), so that R_thr follows the cloud.  voxel_size None: pick_voxel_size(points, sigma).
    Still not PYME's octree: a regular grid at one resolution.  The field (neighbours.NeighbourContext.node_field) goes from its kernel
    to the surface nets on the device; it never visits the host.  As with density_isosurface the surface has an inner sheet wherever
    the cloud is a shell."""
    from . import neighbours
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    k = int(n_points_min)
    if not 1 <= k < neighbours.MAX_K:
        raise ValueError('n_points_min must be in 1..%d' % (neighbours.MAX_K - 1))
    h = float(np.float32(pick_voxel_size(pts, sigma) if voxel_size is None else voxel_size))
    nctx = neighbours.NeighbourContext(device)
    try:
        t0 = time.time()
        median = None
        if threshold_density is None:
            median = float(np.median(neighbours.local_density(pts, k, context=nctx)))
            threshold_density = float(threshold_fraction) * median
        else:
            nctx.set_cloud(pts)
        R_thr, r_cap, pad, thr = knn_threshold(h, k, threshold_density)
        lo, dims = grid_for(pts, h, pad)
        nctx.node_field(lo, h, dims, k, r_cap)
        ctx = IsosurfaceContext(device)
        try:
            ctx.set_field(nctx.field_pointer(), lo, h, dims)
            v, f = ctx.extract(thr)
        finally:
            ctx.close()
        dt = time.time() - t0
    finally:
        nctx.close()
    info = dict(lo=lo, h=h, dims=dims, pad=pad, thr=thr, n_points_min=k, R_thr=R_thr, r_cap=r_cap, threshold_density=float(threshold_density),
                median_density=median, seconds=dt)
    return v, f, info


class Surface(object):
    """What start_surface returns: anything with .vertices / .faces is a start surface for ShrinkwrapMembrane."""

    def __init__(self, vertices, faces, info):
        self.vertices, self.faces, self.info = vertices, faces, info


def mean_edge_length(vertices, faces):
    v = np.asarray(vertices, np.float64)
    e = np.concatenate([v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 1]], v[faces[:, 0]] - v[faces[:, 2]]])
    return float(np.sqrt((e * e).sum(1)).mean())


def start_surface(points, voxel_size=None, passes=2, threshold_density=None, threshold_fraction=0.3, pad=None, device=0, sigma=None,
                  cull_inner=True, remesh=True, target_edge_length=None, min_component_faces=32, method='grid', n_points_min=20):
    """density_isosurface (method='grid') or knn_isosurface (method='knn', with n_points_min; passes and pad do not apply), then the
    package's existing pieces: components by SurgeryContext.label_faces / component_stats, inner sheets by
    surgery.inner_components (inverted shells, shells inside a kept one), dust below min_component_faces faces, and three passes of
    remesh_device at target_edge_length (default: the mesh's own mean edge length, as the synthetic start meshes are made).
    Returns a Surface (.vertices, .faces, .info)."""
    from . import surgery
    if method == 'grid':
        v, f, info = density_isosurface(points, voxel_size, passes, threshold_density, threshold_fraction, pad, device, sigma)
    elif method == 'knn':
        v, f, info = knn_isosurface(points, voxel_size, n_points_min, threshold_density, threshold_fraction, device, sigma)
    else:
        raise ValueError("start_surface: method must be 'grid' or 'knn'")
    info['method'] = method
    t0 = time.time()
    ctx = surgery.SurgeryContext(device)
    try:
        twin = surgery.twins(f, v.shape[0])
        lab, n = ctx.label_faces(f, twin)
        st = ctx.component_stats(v, f, twin, lab, n)
        removed = []
        if cull_inner:
            samples = surgery.sample_vertices(f, lab, n)
            removed = surgery.inner_components(st['volume'], samples, lambda qv, qc: ctx.winding(v, f, lab, n, v[qv], qc))
        gone = set(c for c, _ in removed)
        for c in range(n):
            if c not in gone and st['faces'][c] < int(min_component_faces):
                removed.append((c, '%d faces, fewer than %d' % (st['faces'][c], int(min_component_faces))))
                gone.add(c)
    finally:
        ctx.close()
    info.update(n_components=n, removed=sorted(removed), component_faces=st['faces'].copy(), component_volume=st['volume'].copy())
    if len(gone) == n:
        raise RuntimeError('start_surface: no component of the isosurface is left (%s)' % '; '.join(r for _, r in removed))
    if gone:
        f = f[~np.isin(lab, sorted(gone))]
        used = np.zeros(v.shape[0], bool)
        used[f.ravel()] = True
        v, f = np.ascontiguousarray(v[used]), np.ascontiguousarray((np.cumsum(used) - 1)[f], np.int32)
    if remesh:
        from .remesh import remesh_device
        target = mean_edge_length(v, f) if target_edge_length is None else float(target_edge_length)
        v, f = remesh_device(v, f, 3, target, 0.5, 0, device=device)
        info['target_edge_length'] = target
    info['seconds_cleanup'] = time.time() - t0
    return Surface(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), info)


class DensitySurface(object):
    """Recipe-module mirror for the start surface, in the plain-attribute style of ShrinkwrapMembrane: it takes the place of upstream's
    Octree -> DualMarchingCubes pair (it is not their algorithm: see the module docstring) and stores a surface with .vertices / .faces
    under `output`, so that DensitySurface().execute(ns); ShrinkwrapMembrane().execute(ns) is upstream's recipe."""

    def __init__(self, **kw):
        self.input, self.output = 'filtered_localizations', 'surf'
        self.threshold_density = None              # nm^-3, DualMarchingCubes.threshold_density; None = threshold_fraction x the median of the occupied voxels
        self.threshold_fraction = 0.3
        self.remesh = True                         # DualMarchingCubes.remesh
        self.voxel_size = None                     # nm; None = the median of the `sigma_x` column, or pick_voxel_size's rule without one
        self.passes = 2
        self.method = 'grid'                       # 'knn': the level set of the k-NN density (knn_isosurface), bandwidth from n_points_min and the threshold
        self.n_points_min = 20                     # Octree.n_points_min: the k of method = 'knn'
        self.cull_inner_surfaces = True
        self.min_component_faces = 32
        self.target_edge_length = None
        self.sigma_x = 'error_x'
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        src = namespace[self.input]
        pts = np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T, np.float32)
        try:
            sigma = src[self.sigma_x]
        except (KeyError, IndexError, ValueError):
            sigma = None
        surf = start_surface(pts, voxel_size=self.voxel_size, passes=self.passes, threshold_density=self.threshold_density,
                             threshold_fraction=self.threshold_fraction, device=self.device, sigma=sigma, cull_inner=self.cull_inner_surfaces,
                             remesh=self.remesh, target_edge_length=self.target_edge_length, min_component_faces=self.min_component_faces,
                             method=self.method, n_points_min=self.n_points_min)
        namespace[self.output] = surf
        return surf
