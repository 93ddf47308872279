"""
Screened Poisson surface reconstruction of an oriented cloud on a regular lattice: the comparator of upstream's evaluation
(ch_shrinkwrap/evaluation.py runs compute_shrinkwrap and compute_spr on the same simulated cloud).  ctypes binding of
include/nw_poisson.h (kernels in libnanowrap_hip.so, csrc/nw_poisson.hip) and what sits on top of it.

Upstream's surface_fitting.ScreenedPoissonMesh wraps pymeshlab.  This is NOT pymeshlab's / Kazhdan's octree solver: it is a complete
cube of 2^depth nodes an axis, piecewise-linear splats in integers and a cascadic coarse-to-fine red-black Gauss-Seidel solve, with
upstream's parameter names at their meaning where they have one.  The definition is this project's own, written down in
csrc/nw_poisson_core.h and restated in NumPy in tests/screened_poisson_ref.py; the device gives that restatement's bits.

  the solver
    PoissonContext            one nwo_ctx: set_samples, plan, then solve -- or level_begin / relax / get_level phase by phase -- and field
    cube_for                  the cube of a cloud: upstream's `scale`
    screened_poisson          upstream's signature: (points, normals) -> (vertices float32, faces int32), extracted by the isosurface
                              unit's surface nets from the field, which never visits the host
  normals for a cloud that has none
    orient_normals            turns each normal to the side of the nearest face of a start surface: host NumPy on device results
  recipe-module surface
    ScreenedPoissonMesh       upstream's sixteen traits: a table -> a MembraneMesh under `membrane`

Everything that counts runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes
import time

import numpy as np

from . import _lib

SYMBOLS = ['nwo_abi_version', 'nwo_create', 'nwo_destroy', 'nwo_last_error', 'nwo_set_samples', 'nwo_plan', 'nwo_level_begin', 'nwo_relax',
           'nwo_get_level', 'nwo_set_chi', 'nwo_solve', 'nwo_field', 'nwo_field_pointer', 'nwo_get_field']
ABI_VERSION = 1
NWO_OK, NWO_ERR_BADARG, NWO_ERR_HIP, NWO_ERR_NONFINITE, NWO_ERR_NOMEM, NWO_ERR_STATE, NWO_ERR_EMPTY = 0, -1, -2, -3, -4, -5, -6
ERRORS = {NWO_ERR_BADARG: 'bad argument', NWO_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWO_ERR_NONFINITE: 'non-finite sample',
          NWO_ERR_NOMEM: 'out of device memory', NWO_ERR_STATE: 'a call before the one it needs',
          NWO_ERR_EMPTY: 'no sample with a normal, or a solution that is zero everywhere'}
NWO_GET_W, NWO_GET_V, NWO_GET_RHS, NWO_GET_DIAG, NWO_GET_CHI = range(5)
NWO_RESIDUAL_WORDS = 20
MAX_N = 1 << 25
NORMAL_BITS, WEIGHT_BITS, FIELD_BITS = 12, 7, 31          # the three quantisation exponents: normals, splat weights per axis, the field
BASE_LEVEL, MIN_DEPTH, MAX_DEPTH = 2, 3, 9
IGNORED = ('visiblelayer', 'cgdepth', 'preclean', 'threads')

_L = None


def load():
    """The library's nwo_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
        L = _lib.load_entry_points(SYMBOLS, {
            'nwo_abi_version': [], 'nwo_create': [i32, ctypes.POINTER(vp)], 'nwo_destroy': [vp], 'nwo_last_error': [vp],
            'nwo_set_samples': [vp, vp, vp, i64, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)],
            'nwo_plan': [vp, vp, f32, i32, i32, f64, ctypes.POINTER(i32), vp],
            'nwo_level_begin': [vp, i32, f64], 'nwo_relax': [vp, i32, ctypes.POINTER(f64), ctypes.POINTER(f64)],
            'nwo_get_level': [vp, i32, vp], 'nwo_set_chi': [vp, vp],
            'nwo_solve': [vp, f64, i32, i32, ctypes.POINTER(f64), vp],
            'nwo_field': [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(f64), ctypes.POINTER(ctypes.c_uint64)],
            'nwo_field_pointer': [vp], 'nwo_get_field': [vp, vp]}, 'nwo_abi_version', ABI_VERSION, 'nw_poisson')
        L.nwo_field_pointer.restype = vp                   # (the one entry point that returns a pointer)
        _L = L
    return _L


_p = _lib.ptr


def _triples(a):
    """-> (what keeps the memory alive, pointer, n, on_device): an (n,3) array (copied to float32 if it is not) or (device pointer, n)"""
    if isinstance(a, tuple) and len(a) == 2 and isinstance(a[0], (int, np.integer)):
        return None, _p(int(a[0])), int(a[1]), 1
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    return a, _p(a), a.shape[0], 0


class PoissonContext(_lib.QueryContext):
    """One nwo_ctx: the samples, the lattice, one level of the solve at a time and the field of the last one, all on the device."""
    prefix, errors, gpu_only, load = 'nwo_', ERRORS, 'the screened Poisson solver runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_used = self.n_skipped = 0
        self.depth = self.depth_used = self.level = 0
        self.occ = None

    def set_samples(self, points, normals, use_lengths=False):
        """Positions and outward normals, both (n,3) float32 on the host or both (device pointer, n).  -> (n_used, n_skipped): a normal
        of length 0 is skipped.  use_lengths (upstream's confidence) takes the normals' lengths as weights, at most 1 a component."""
        kp, pp, n, dev = _triples(points)
        kn, pn, n2, dev2 = _triples(normals)
        if n != n2 or dev != dev2:
            raise ValueError('set_samples: positions and normals are two (n,3) arrays or two device pointers of one length')
        used, skipped = ctypes.c_int64(), ctypes.c_int64()
        self.n_used = self.depth_used = self.level = 0
        self.check(self.L.nwo_set_samples(self.h, pp, pn, n, dev, int(bool(use_lengths)), ctypes.byref(used), ctypes.byref(skipped)), 'nwo_set_samples')
        self.n_used, self.n_skipped = int(used.value), int(skipped.value)
        return self.n_used, self.n_skipped

    def plan(self, lo, h, depth, fulldepth=5, samples_per_node=1.5):
        """The cube (lo, h: float32, the spacing of the finest level) and the depth used -> (depth_used, occ {level: distinct home nodes})."""
        lo = np.ascontiguousarray(lo, np.float32).reshape(3)
        used = ctypes.c_int()
        occ = np.zeros(int(depth) + 1 if 0 <= int(depth) <= MAX_DEPTH else 1, np.int64)
        self.depth_used = self.level = 0
        self.check(self.L.nwo_plan(self.h, _p(lo), float(h), int(depth), int(fulldepth), float(samples_per_node), ctypes.byref(used), _p(occ)), 'nwo_plan')
        self.depth, self.depth_used = int(depth), int(used.value)
        self.lo, self.h_fine = lo, np.float32(h)
        self.occ = {l: int(occ[l]) for l in range(BASE_LEVEL, self.depth + 1)}
        return self.depth_used, self.occ

    @property
    def h_used(self):
        return np.float32(float(self.h_fine) * float(1 << (self.depth - self.depth_used)))

    def alpha(self, pointweight):
        return (float(pointweight) * float(self.occ[self.depth_used])) / float(self.n_used)

    def level_begin(self, level, alpha):
        self.level = 0
        self.check(self.L.nwo_level_begin(self.h, int(level), float(alpha)), 'nwo_level_begin')
        self.level = int(level)

    def relax(self, sweeps):
        """-> the largest residual (before, after) the sweeps"""
        before, after = ctypes.c_double(), ctypes.c_double()
        self.check(self.L.nwo_relax(self.h, int(sweeps), ctypes.byref(before), ctypes.byref(after)), 'nwo_relax')
        return float(before.value), float(after.value)

    def get_level(self, what):
        """An array of the level at hand, [z, y, x]: 'W' int64, 'V' (3, ...) int64, 'rhs', 'diag', 'chi' float64."""
        code = {'W': NWO_GET_W, 'V': NWO_GET_V, 'rhs': NWO_GET_RHS, 'diag': NWO_GET_DIAG, 'chi': NWO_GET_CHI}[what]
        n = 1 << self.level
        out = np.empty((3, n, n, n) if what == 'V' else (n, n, n), np.int64 if what in ('W', 'V') else np.float64)
        self.check(self.L.nwo_get_level(self.h, code, _p(out)), 'nwo_get_level')
        return out

    def set_chi(self, chi):
        n = 1 << self.level
        a = np.ascontiguousarray(chi, np.float64)
        if a.shape != (n, n, n):
            raise ValueError('set_chi: the array has the shape of the level at hand, [z, y, x]')
        self.check(self.L.nwo_set_chi(self.h, _p(a)), 'nwo_set_chi')

    def solve(self, pointweight=4.0, iters=8, coarse_iters=64):
        """Every level from the base to the depth used -> (alpha, {level: (residual before, after)})."""
        alpha = ctypes.c_double()
        res = np.zeros(NWO_RESIDUAL_WORDS)
        self.level = 0
        self.check(self.L.nwo_solve(self.h, float(pointweight), int(iters), int(coarse_iters), ctypes.byref(alpha), _p(res)), 'nwo_solve')
        self.level = self.depth_used
        return float(alpha.value), {l: (float(res[2 * l]), float(res[2 * l + 1])) for l in range(BASE_LEVEL, self.depth_used + 1)}

    def field(self, return_field=False):
        """Quantise the solution of the depth used -> dict(thr, E, sumW[, F uint64 [z, y, x]]); F stays on the device (field_pointer)."""
        thr, E, sw = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
        self.check(self.L.nwo_field(self.h, ctypes.byref(thr), ctypes.byref(E), ctypes.byref(sw)), 'nwo_field')
        out = dict(thr=int(thr.value), E=float(E.value), sumW=int(sw.value))
        if return_field:
            n = 1 << self.depth_used
            out['F'] = np.empty((n, n, n), np.uint64)
            self.check(self.L.nwo_get_field(self.h, _p(out['F'])), 'nwo_get_field')
        return out

    def field_pointer(self):
        """The device pointer of the last field's F, as an int (0 if there is none)."""
        return int(self.L.nwo_field_pointer(self.h) or 0)


def cube_for(points, depth, scale=1.1):
    """(lo (3,) float32, h float32) of the solver's cube: centre = the midpoint of the samples' bounding box, side = scale x its largest
    extent, h = side / 2^depth.  Computed in float64 and rounded once.  A cloud without extent raises."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    if p.shape[0] == 0 or not np.isfinite(p).all():
        raise ValueError('cube_for: the cloud is empty or holds a non-finite sample')
    mn, mx = p.min(0), p.max(0)
    side = float(scale) * float((mx - mn).max())
    if not (side > 0.0 and np.isfinite(side)):
        raise ValueError('cube_for: the cloud has no extent (or scale is not positive)')
    return (0.5 * (mn + mx) - 0.5 * side).astype(np.float32), np.float32(side / float(1 << int(depth)))


def orient_normals(points, normals, mesh, device=0):
    """(n,3) float32: each normal as it is, or negated where its dot product with the normal of the face of `mesh` nearest to its point is
    negative (distance.distance_to_mesh's faces, TriMesh.face_normals: host NumPy on device results).  Upstream propagates an orientation
    over the cloud; this stand-in propagates nothing and needs a start surface that is right about inside and outside: near a face whose
    own normal is wrong, or where the nearest face belongs to another sheet, it is wrong too."""
    from .distance import distance_to_mesh
    from .trimesh import TriMesh
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    N = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if P.shape != N.shape:
        raise ValueError('orient_normals: one normal a point')
    _, face = distance_to_mesh(P, mesh, signed=False, return_face=True, device=device)
    tm = mesh if hasattr(mesh, 'face_normals') else TriMesh(np.asarray(mesh.vertices, np.float32), np.asarray(mesh.faces, np.int32), vertex_normals=False, lazy_topology=True)
    fn = np.asarray(tm.face_normals, np.float64)[np.asarray(face, np.int64)]
    flip = (N.astype(np.float64) * fn).sum(1) < 0.0
    return np.where(flip[:, None], -N, N)


def _normals_for(points, k, flipflag, viewpos, orient, start, device):
    from . import structure
    radius = structure.radius_from_k(points, int(k), device=device)
    if flipflag:
        return structure.cloud_normals(points, radius, viewpoint=np.asarray(viewpos, np.float64).reshape(3), device=device)
    N = structure.cloud_normals(points, radius, device=device)
    if orient in (None, 'surface'):
        if start is None:
            from .isosurface import start_surface
            start = start_surface(points, device=device)
        return orient_normals(points, N, start, device=device)
    if orient == 'none':
        return N
    raise ValueError("screened_poisson: orient is 'surface' or 'none'")


def screened_poisson(points, normals=None, k=10, smoothiter=0, flipflag=False, viewpos=(0, 0, 0), depth=8, fulldepth=5, scale=1.1, samplespernode=1.5,
                     pointweight=4, iters=8, confidence=False, coarse_iters=64, orient=None, start=None, device=0, context=None, return_info=False,
                     visiblelayer=False, cgdepth=0, preclean=False, threads=8):
    """Upstream's screened_poisson(points, normals, ...) -> (vertices (V,3) float32, faces (F,3) int32) of a closed surface through an
    oriented cloud; with return_info a third value, dict(depth_used, h, occ, alpha, residuals, thr, E, n_used, n_skipped, seconds, lo).

    depth, fulldepth, samplespernode, pointweight, iters, scale, confidence: upstream's names, as csrc/nw_poisson_core.h defines them
    (depth 3..9; the lattice is refined while a level is at most fulldepth or holds samplespernode samples an occupied node).
    coarse_iters: the sweeps at the base level.  normals None: structure.cloud_normals at radius_from_k(points, k), made to face viewpos
    when flipflag (upstream's meaning), else turned by orient_normals against `start` (default: isosurface.start_surface(points));
    orient='none' leaves them as they come.  visiblelayer, cgdepth, preclean and threads are accepted and ignored: they have no meaning
    on a complete lattice.  smoothiter != 0 raises NotImplementedError.  context: a PoissonContext to use.  Normals that point inwards
    put the outside inside: the surface nets then meet the border of the lattice, and that error is re-raised in those words."""
    if int(smoothiter) != 0:
        raise NotImplementedError('screened_poisson: smoothiter (normal smoothing) is not implemented')
    if not MIN_DEPTH <= int(depth) <= MAX_DEPTH:
        raise ValueError('screened_poisson: depth must be in %d..%d' % (MIN_DEPTH, MAX_DEPTH))
    if not (float(pointweight) > 0 and np.isfinite(float(pointweight))):
        raise ValueError('screened_poisson: pointweight must be positive')
    if int(iters) < 0 or int(coarse_iters) < 0 or int(fulldepth) < 0 or not float(samplespernode) >= 0:
        raise ValueError('screened_poisson: iters, coarse_iters, fulldepth and samplespernode must not be negative')
    from . import isosurface
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if not 1 <= P.shape[0] <= MAX_N:
        raise ValueError('screened_poisson: 1 to 2^25 samples')
    lo, h = cube_for(P, depth, scale)
    t0 = time.time()
    if normals is None:
        normals = _normals_for(P, k, flipflag, viewpos, orient, start, device)
    own = context is None
    ctx = PoissonContext(device) if own else context
    try:
        n_used, n_skipped = ctx.set_samples(P, normals, use_lengths=confidence)
        used, occ = ctx.plan(lo, h, depth, fulldepth, samplespernode)
        alpha, residuals = ctx.solve(pointweight, iters, coarse_iters)
        fld = ctx.field()
        ictx = isosurface.IsosurfaceContext(device)
        try:
            n = 1 << used
            ictx.set_field(ctx.field_pointer(), lo, ctx.h_used, (n, n, n))
            nv, nf = ctypes.c_int64(), ctypes.c_int64()
            code = ictx.L.nwi_extract(ictx.h, int(fld['thr']), ctypes.byref(nv), ctypes.byref(nf))
            if code == isosurface.NWI_ERR_BORDER:
                raise RuntimeError('screened_poisson: the level set reaches the border of the lattice: the normals point inwards (or are not '
                                   'consistently oriented)')
            ictx.check(code, 'nwi_extract')
            v, f = np.empty((nv.value, 3), np.float32), np.empty((nf.value, 3), np.int32)
            ictx.check(ictx.L.nwi_get(ictx.h, _p(v), _p(f), None), 'nwi_get')
        finally:
            ictx.close()
    finally:
        if own:
            ctx.close()
    if not return_info:
        return v, f
    return v, f, dict(depth_used=used, h=float(np.float32(float(h) * float(1 << (int(depth) - used)))), occ=occ, alpha=alpha, residuals=residuals,
                      thr=fld['thr'], E=fld['E'], n_used=n_used, n_skipped=n_skipped, seconds=time.time() - t0, lo=lo)


# ---- recipe-module surface ----------------------------------------------------------------------------------------------------------------
class ScreenedPoissonMesh(object):
    """Mirror of the recipe module `ScreenedPoissonMesh` in the plain-attribute style of DensitySurface / ShrinkwrapMembrane: upstream's
    sixteen trait names and defaults, plus `device`.  The table with x y z under `input` -> a MembraneMesh under `output`.  use_normals
    reads the columns xn yn zn and falls back to computed normals when the table has none, as upstream.  The wall seconds are in
    mesh.spr_info['runtime'] (upstream's Processing.ScreenedPoissonMesh.Runtime), next to screened_poisson's info."""

    def __init__(self, **kw):
        self.input, self.output = 'filtered_localizations', 'membrane'
        self.k = 10
        self.smoothiter = 0
        self.flipflag = False
        self.viewpos = [0, 0, 0]
        self.visiblelayer = False
        self.depth = 8
        self.fulldepth = 5
        self.cgdepth = 0
        self.scale = 1.1
        self.samplespernode = 1.5
        self.pointweight = 4.0
        self.iters = 8
        self.confidence = False
        self.preclean = False
        self.threads = 8
        self.use_normals = False
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        from .membrane_mesh import MembraneMesh
        src = namespace[self.input]
        points = np.ascontiguousarray(np.vstack([src['x'], src['y'], src['z']]).T, np.float32)
        normals = None
        if self.use_normals:
            try:
                normals = np.ascontiguousarray(np.vstack([src['xn'], src['yn'], src['zn']]).T, np.float32)
            except KeyError:
                normals = None
        t0 = time.time()
        v, f, info = screened_poisson(points, normals, k=self.k, smoothiter=self.smoothiter, flipflag=self.flipflag, viewpos=np.array(self.viewpos),
                                      visiblelayer=self.visiblelayer, depth=self.depth, fulldepth=self.fulldepth, cgdepth=self.cgdepth, scale=self.scale,
                                      samplespernode=self.samplespernode, pointweight=self.pointweight, iters=self.iters, confidence=self.confidence,
                                      preclean=self.preclean, threads=self.threads, device=self.device, return_info=True)
        mesh = MembraneMesh(vertices=v, faces=f)
        info['runtime'] = time.time() - t0
        mesh.spr_info = info
        namespace[self.output] = mesh
        return mesh
