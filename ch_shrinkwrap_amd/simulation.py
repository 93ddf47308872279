"""
Simulated SMLM clouds from a shape, on the GPU: the first stage of the reference's evaluation recipe (ch_shrinkwrap/test_evaluation_recipe.yaml),

    PointcloudFromShape   recipe_modules/simulation.py:11-61 -> evaluation_utils.generate_smlm_pointcloud_from_shape (:182-263)

(paths relative to /root/reference/ch_shrinkwrap/).  The kernels are include/nw_simulation.h's (csrc/nw_simulation.hip, in libnanowrap_hip.so);
there is no host fallback: without a GPU every function here that computes something raises.

What is upstream's and what is not:
  * the shapes are shape.py's constructive solid geometry over sdf.py's primitives, compiled by `compile_shape` into a flat postfix program
    that the device evaluates in float64 (pinned against the reference's own values: tests/golden/sdf_shapes.npz, simulation_case.npz);
  * the localization model is util.loc_error's, the clusters are evaluation_utils.smlmify_points', the background is
    generate_smlm_pointcloud_from_shape's, each with upstream's quirks kept (a kept copy gets a fresh sigma, the background box is the
    cloud's box scaled by 1.2 about the ORIGIN);
  * the surface sampler is NOT PYME's `points_from_sdf` (PYME is not part of the reference tree).  `points_from_sdf` here is the project's own:
    a regular lattice of pitch dx_min = density^(-1/3) with a shell test (-dx/2 <= sdf < dx/2: area / dx^2 fluorophores whatever the surface's
    orientation), each node kept with probability p, and -- by default -- projected onto the zero level set by two Newton steps.  Its cube
    must enclose the shape, and shape.py's `_radius` does not always (TwoToruses(30, 100) reaches |x| = 230 with `_radius` 200), so
    `compile_shape` computes an enclosing box of its own;
  * the random numbers are counter-based (Philox4x32-10, include/nw_simulation.h) with a `seed` argument, not NumPy's global state: the same
    arguments give the same bytes, and no draw depends on how the work is laid out.
"""
import ast
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwg_abi_version', 'nwg_create', 'nwg_destroy', 'nwg_last_error', 'nwg_set_program', 'nwg_eval', 'nwg_normals', 'nwg_sample_surface',
           'nwg_get_points', 'nwg_loc_error', 'nwg_displace', 'nwg_smlmify', 'nwg_background']
ABI_VERSION = 1
(NWG_OK, NWG_ERR_BADARG, NWG_ERR_HIP, NWG_ERR_NONFINITE, NWG_ERR_NOMEM, NWG_ERR_NOPROGRAM, NWG_ERR_CAPACITY, NWG_ERR_TOOMANY,
 NWG_ERR_NOPOINTS) = 0, -1, -2, -3, -4, -5, -6, -7, -8
ERRORS = {NWG_ERR_BADARG: 'bad argument', NWG_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWG_ERR_NONFINITE: 'non-finite value',
          NWG_ERR_NOMEM: 'out of device memory', NWG_ERR_NOPROGRAM: 'no shape program is set', NWG_ERR_CAPACITY: 'more points than max_points',
          NWG_ERR_TOOMANY: 'too many lattice cells', NWG_ERR_NOPOINTS: 'the context holds no points'}
MAX_OPS, STACK_DEPTH, COORD_BITS, COPIES = 256, 8, 21, 10
(OP_FRAME, OP_SPHERE, OP_TORUS, OP_CAPSULE, OP_ROUND_BOX, OP_SHEET, OP_UNION, OP_DIFFERENCE, OP_INTERSECTION) = range(9)
(STREAM_THIN, STREAM_PHOTONS, STREAM_DISPLACE, STREAM_COPY_DISPLACE, STREAM_COPY_KEY, STREAM_COPY_PHOTONS, STREAM_BG_POSITION,
 STREAM_BG_PHOTONS, STREAM_BG_COPY_DISPLACE, STREAM_BG_COPY_KEY, STREAM_BG_COPY_PHOTONS) = range(11)
MODEL_CONSTANT, MODEL_EXPONENTIAL = 0, 1
OP_DTYPE = np.dtype([('code', '<i4'), ('reserved', '<i4'), ('a', '<f8', (12,))])              # nwg_op
LIPSCHITZ = 1.5                    # synth.isosurface_mesh's safety factor on the field's slope

_L = None


def load():
    """The library's nwg_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f64, u64, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_uint64, ctypes.c_uint32
        _L = _lib.load_entry_points(SYMBOLS, {
            'nwg_abi_version': [], 'nwg_create': [i32, ctypes.POINTER(vp)], 'nwg_destroy': [vp], 'nwg_last_error': [vp],
            'nwg_set_program': [vp, vp, i32],
            'nwg_eval': [vp, vp, i64, vp],
            'nwg_normals': [vp, vp, i64, vp],
            'nwg_sample_surface': [vp, vp, f64, f64, f64, u64, f64, i32, i32, i64, ctypes.POINTER(i64)],
            'nwg_get_points': [vp, vp, vp],
            'nwg_loc_error': [vp, i64, u64, u32, i32, vp, f64, f64, vp, vp],
            'nwg_displace': [vp, vp, vp, i64, u64, u32, vp],
            'nwg_smlmify': [vp, vp, vp, i64, i64, u64, u32, u32, u32, i32, vp, f64, f64, vp, vp, vp],
            'nwg_background': [vp, vp, vp, i64, u64, u32, vp]},
            'nwg_abi_version', ABI_VERSION, 'nw_simulation')
    return _L


_p = _lib.ptr


# ---- shapes -> programs -------------------------------------------------------------------------------------------------------------
_I3 = np.eye(3)


class _Node(object):
    """A shape of shape.py: `centroid` and `radius` follow the reference's constructors (they decide where a RotationShape turns and what
    upstream would hand to points_from_sdf); `box()` is this project's own enclosing box."""
    centroid = radius = None


def _vec(v):
    v = np.array(v, dtype=float).reshape(-1)
    if v.shape != (3,):
        raise ValueError('expected three numbers, got %r' % (v,))
    return v


class _Primitive(_Node):
    def __init__(self, code, args, centroid, radius, local_centre, local_radius, shift):
        self.code, self.args = code, [float(x) for x in args]
        self.centroid, self.radius = centroid, float(radius)
        self.local_centre, self.local_radius = _vec(local_centre), float(local_radius)
        self.shift = shift                                   # True: the reference evaluates it at p - centroid

    def frame(self, frame):
        M, t = frame
        return (M, t + M.T @ self.centroid) if self.shift else frame

    def emit(self, out, frame):
        out.append(('prim', self.code, self.args, self.frame(frame)))

    def box(self, frame):
        M, t = self.frame(frame)
        c = t + M.T @ self.local_centre
        return c - self.local_radius, c + self.local_radius


class _Combinator(_Node):
    def __init__(self, code, s0, s1, k, centroid, radius):
        self.code, self.s0, self.s1, self.k = code, s0, s1, float(k)
        self.centroid, self.radius = centroid, float(radius)
        if not self.k >= 0:
            raise ValueError('k must be >= 0')

    def emit(self, out, frame):
        self.s0.emit(out, frame)
        self.s1.emit(out, frame)
        out.append(('comb', self.code, self.k))

    def box(self, frame):
        (l0, h0), (l1, h1) = self.s0.box(frame), self.s1.box(frame)
        if self.code == OP_UNION:
            lo, hi = np.minimum(l0, l1), np.maximum(h0, h1)
        elif self.code == OP_DIFFERENCE:                     # s1 with s0 carved out
            lo, hi = l1, h1
        else:
            lo, hi = np.maximum(l0, l1), np.minimum(h0, h1)
            if (lo > hi).any():
                lo, hi = l0, h0
        return lo - 0.25 * self.k, hi + 0.25 * self.k        # (a smooth combination moves the surface by at most k / 4)


class _Rotation(_Node):
    """RotationShape (shape.py:446-480): s0 evaluated at inv(Rz Ry Rx) (p - centroid), with centroid = s0's."""

    def __init__(self, s0, rx=0.0, ry=0.0, rz=0.0):
        sx, cx, sy, cy, sz, cz = np.sin(rx), np.cos(rx), np.sin(ry), np.cos(ry), np.sin(rz), np.cos(rz)
        rot = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ (np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
        self.s0, self.inv = s0, rot.T
        self.centroid, self.radius = s0.centroid, s0.radius

    def child_frame(self, frame):
        M, t = frame
        return self.inv @ M, t + M.T @ self.centroid

    def emit(self, out, frame):
        self.s0.emit(out, self.child_frame(frame))

    def box(self, frame):
        return self.s0.box(self.child_frame(frame))


def _centroid(kw):
    c = _vec(kw.pop('centroid', (0.0, 0.0, 0.0)))
    if kw:
        raise TypeError('unknown shape parameter(s): %s' % ', '.join(sorted(kw)))
    return c


def Sphere(radius=2, **kw):
    return _Primitive(OP_SPHERE, [radius], _centroid(kw), radius, (0, 0, 0), radius, True)


def Torus(radius=2, r=0.05, **kw):
    """`radius` is the major radius, `r` the minor: shape.Torus.sdf passes them as sdf.torus's (r, R) (shape.py:125)."""
    return _Primitive(OP_TORUS, [radius, r], _centroid(kw), radius, (0, 0, 0), float(radius) + float(r), True)


def Capsule(start, end, radius=1, **kw):
    a, b = _vec(start), _vec(end)
    length = float(np.sqrt(((b - a) ** 2).sum()))
    if not ((b - a) ** 2).sum() > 0:                         # sdf.capsule (sdf.py:75) divides by it: NaN everywhere upstream, refused here
        raise ValueError('a capsule whose ends coincide has no axis: start %r, end %r' % (list(a), list(b)))
    return _Primitive(OP_CAPSULE, list(a) + list(b) + [radius], _centroid(kw) + 0.5 * (a + b), length / 2.0 + radius, 0.5 * (a + b),
                      length / 2.0 + float(radius), False)


def Box(halfwidth, r=0, **kw):
    w = _vec(halfwidth)
    return _Primitive(OP_ROUND_BOX, list(w) + [r], _centroid(kw), w.max(), (0, 0, 0), float(np.linalg.norm(w)) + float(r), True)


def Sheet(halfwidth, r=0, **kw):
    w = _vec(halfwidth)
    return _Primitive(OP_SHEET, list(w) + [r], _centroid(kw), w.max(), (0, 0, 0), float(np.linalg.norm([w[0], w[1], max(w[2], float(r))])) + float(r), True)


def _sub(s):
    """An operand of a combinator: a shape built by this module, (name, params), or {name: params}."""
    if isinstance(s, _Node):
        return s
    if isinstance(s, dict) and len(s) == 1:
        s = list(s.items())[0]
    if isinstance(s, (tuple, list)) and len(s) == 2 and isinstance(s[0], str):
        return build_shape(s[0], s[1])
    raise ValueError('an operand is a shape, (name, params) or {name: params}; got %r' % (s,))


def UnionShape(s0, s1, k=0, n=1, **kw):
    s0, s1 = _sub(s0), _sub(s1)
    _centroid(kw)                                            # (accepted and, as upstream, overwritten: shape.py:367)
    return _Combinator(OP_UNION, s0, s1, k, (1.0 / (n + 1)) * (s0.centroid + n * s1.centroid), s0.radius + s1.radius)


def DifferenceShape(s0, s1, k=0, **kw):
    s0, s1 = _sub(s0), _sub(s1)
    _centroid(kw)
    big = s0 if s0.radius > s1.radius else s1                # shape.py:396-401
    return _Combinator(OP_DIFFERENCE, s0, s1, k, big.centroid, big.radius)


def IntersectionShape(s0, s1, k=0, **kw):
    s0, s1 = _sub(s0), _sub(s1)
    _centroid(kw)
    small = s0 if s0.radius < s1.radius else s1              # shape.py:430-435
    return _Combinator(OP_INTERSECTION, s0, s1, k, small.centroid, small.radius)


def RotationShape(s0, rx=0.0, ry=0.0, rz=0.0, **kw):
    _centroid(kw)                                            # (overwritten by s0's, shape.py:477)
    return _Rotation(_sub(s0), rx, ry, rz)


def TwoToruses(r, R):
    return UnionShape(Torus(radius=R, r=r, centroid=[-R, 0, 0]), Torus(radius=R, r=r, centroid=[R, 0, 0]))      # shape.py:315


def NToruses(toruses, centroid=(0.0, 0.0, 0.0)):
    """shape.py:317-341: a chain of tori along x; `toruses` is a dict (or list) of {'r', 'R'} in chain order."""
    items = list(toruses.values()) if isinstance(toruses, dict) else list(toruses)
    if not items:
        raise ValueError('NToruses needs at least one torus')
    dt, rest = items[0], items[1:]
    c = _vec(centroid)
    if c[0] > 0:
        c[0] += float(dt['R'])
    torus = Torus(radius=float(dt['R']), r=float(dt['r']), centroid=c)
    if not rest:
        return torus
    return UnionShape(torus, NToruses(rest, c + np.array([float(dt['R']), 0, 0])), n=len(rest))


def DualCapsule(length, r, sep):
    return UnionShape(Capsule([-sep / 2, 0, 0], [-sep / 2, length, 0], r), Capsule([sep / 2, 0, 0], [sep / 2, length, 0], r))      # shape.py:343-345


def ThreeWayJunction(h, r, centroid=(0, 0, 0), k=0):
    c = _vec(centroid)
    q = h / np.sqrt(2)
    return UnionShape(Capsule(c, c + [0, -h, 0], r), UnionShape(Capsule(c, c + [-q, q, 0], r), Capsule(c, c + [q, q, 0], r), k), k=0)      # shape.py:252-261


def ERSim2(centroid=(0, 0, 0)):
    """shape.py:288-313; as upstream, `centroid` is not used, and the centroid given to the third sheet is discarded by RotationShape."""
    sh = 100
    a, b, c, d = [0, 0, 0], [400, -50, 0], [500, 250, 0], [0, 240, 0]
    e, f, g, h = [0, -600, 0], [-600, 0, 0], [-40, 0, -100], [-40, 0, 100]
    sheet0 = RotationShape(Sheet([226, 200, sh / 3], sh / 3), rz=np.pi / 4)
    sheet1 = Sheet([50, 50, sh / 3], 1, centroid=[0, 133, 0])
    sheet2 = RotationShape(Sheet([33, 33, sh / 3], sh / 2), rz=7 * np.pi / 3)
    cap = [Capsule(a, b, sh // 2), Capsule(b, c, sh // 2), Capsule(c, d, sh // 2), Capsule(a, e, sh // 2), Capsule(a, f, sh // 2), Capsule(g, h, 50)]
    k = sh / 4
    u = UnionShape(sheet0, UnionShape(cap[0], UnionShape(cap[1], UnionShape(sheet2, cap[2], k=k), k=k), k=k), k=k)
    return DifferenceShape(cap[5], UnionShape(UnionShape(UnionShape(u, sheet1, k=k), cap[3], k=k), cap[4], k=k), k=k)


SHAPES = {f.__name__: f for f in (Sphere, Torus, Capsule, Box, Sheet, TwoToruses, NToruses, DualCapsule, ThreeWayJunction, ERSim2, UnionShape,
                                  DifferenceShape, IntersectionShape, RotationShape)}
NOT_COMPILED = ('Tetrahedron', 'TaperedCapsule', 'TaperedEllipsoid', 'RoundCone', 'BentShape', 'ERSim')


def build_shape(shape_name, shape_params=None):
    if shape_name in NOT_COMPILED:
        raise NotImplementedError('shape %s is not compiled for the device' % shape_name)
    if shape_name not in SHAPES:
        raise ValueError('unknown shape %r' % (shape_name,))
    return SHAPES[shape_name](**dict(shape_params or {}))


class Program(object):
    """A compiled shape: `ops` (OP_DTYPE, the nwg_op array), the reference's `centroid` and `radius`, and this project's enclosing cube:
    `centre`, `r_max` (half its side), from the box [lo, hi]."""

    def __init__(self, ops, node):
        self.ops, self.centroid, self.radius = ops, node.centroid.copy(), node.radius
        self.lo, self.hi = node.box((_I3, np.zeros(3)))
        self.centre = 0.5 * (self.lo + self.hi)
        self.r_max = float(0.5 * (self.hi - self.lo).max())


def compile_shape(shape_name, shape_params=None):
    """getattr(shape, shape_name)(**shape_params) of the reference (evaluation_utils.py:210) as a postfix program for the device.
    `shape_name` may also be a shape built with this module's constructors."""
    node = shape_name if isinstance(shape_name, _Node) else build_shape(shape_name, shape_params)
    items = []
    node.emit(items, (_I3, np.zeros(3)))
    ops, cur, depth, deepest = [], (_I3, np.zeros(3)), 0, 0
    for it in items:
        if it[0] == 'comb':
            ops.append((it[1], [it[2]]))
            depth -= 1
            continue
        M, t = it[3]
        if not (np.array_equal(M, cur[0]) and np.array_equal(t, cur[1])):
            ops.append((OP_FRAME, list(M.ravel()) + list(t)))
            cur = (M, t)
        ops.append((it[1], it[2]))
        depth += 1
        deepest = max(deepest, depth)
    if deepest > STACK_DEPTH:
        raise ValueError('the shape needs a value stack of %d, the device keeps %d' % (deepest, STACK_DEPTH))
    if len(ops) > MAX_OPS:
        raise ValueError('the shape compiles to %d ops, more than %d' % (len(ops), MAX_OPS))
    arr = np.zeros(len(ops), OP_DTYPE)
    for i, (code, args) in enumerate(ops):
        arr['code'][i] = code
        arr['a'][i, :len(args)] = args
    return Program(arr, node)


def _program(shape, shape_params=None):
    return shape if isinstance(shape, Program) else compile_shape(shape, shape_params)


# ---- the context --------------------------------------------------------------------------------------------------------------------
def _cloud(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1, 3)


def _psf(psf_width):
    w = np.asarray(psf_width, np.float64)
    w = np.full(3, float(w)) if w.ndim == 0 else np.ascontiguousarray(w)
    if w.shape != (3,):
        raise ValueError('psf_width is a number or three numbers')
    return w


def _model(model):
    return MODEL_EXPONENTIAL if model == 'exponential' else MODEL_CONSTANT


class SimulationContext(_lib.QueryContext):
    """One nwg_ctx: a shape program, the surface lattice (whose points stay on the device until asked for) and the localization model."""
    prefix, errors, gpu_only, load = 'nwg_', ERRORS, 'the SMLM cloud simulator runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_points = 0
        self.program = None

    def set_program(self, program):
        ops = np.ascontiguousarray(program.ops, OP_DTYPE)
        self.check(self.L.nwg_set_program(self.h, _p(ops), ops.shape[0]), 'nwg_set_program')
        self.program = program

    def eval(self, xyz):
        xyz = _cloud(xyz)
        out = np.empty(xyz.shape[0], np.float64)
        if xyz.shape[0]:
            self.check(self.L.nwg_eval(self.h, _p(xyz), xyz.shape[0], _p(out)), 'nwg_eval')
        return out

    def normals(self, xyz):
        xyz = _cloud(xyz)
        out = np.empty(xyz.shape, np.float64)
        if xyz.shape[0]:
            self.check(self.L.nwg_normals(self.h, _p(xyz), xyz.shape[0], _p(out)), 'nwg_normals')
        return out

    def sample_surface(self, centre, r_max, dx, p, seed=0, lipschitz=LIPSCHITZ, start_level=-1, project=2, max_points=1 << 27, return_keys=False):
        """The lattice sampler; (n,3) float64 in ascending node key (and the keys, uint64)."""
        centre = np.ascontiguousarray(centre, np.float64).reshape(3)
        n = ctypes.c_int64()
        self.n_points = 0
        self.check(self.L.nwg_sample_surface(self.h, _p(centre), float(r_max), float(dx), float(p), int(seed), float(lipschitz), int(start_level),
                                             int(project), int(max_points), ctypes.byref(n)), 'nwg_sample_surface')
        self.n_points = int(n.value)
        xyz, keys = np.empty((self.n_points, 3), np.float64), np.empty(self.n_points, np.uint64)
        if self.n_points:
            self.check(self.L.nwg_get_points(self.h, _p(keys) if return_keys else None, _p(xyz)), 'nwg_get_points')
        return (xyz, keys) if return_keys else xyz

    def loc_error(self, n, seed=0, stream=STREAM_PHOTONS, model='exponential', psf_width=250.0, mean_photon_count=300, bg_photon_count=20,
                  return_photons=False):
        n = int(n)
        sigma = np.empty((n, 3), np.float64)
        photons = np.empty((n, 3), np.float64) if return_photons else None
        if n:
            self.check(self.L.nwg_loc_error(self.h, n, int(seed), int(stream), _model(model), _p(_psf(psf_width)), float(mean_photon_count),
                                            float(bg_photon_count), _p(sigma), _p(photons)), 'nwg_loc_error')
        return (sigma, photons) if return_photons else sigma

    def displace(self, xyz, sigma, seed=0, stream=STREAM_DISPLACE):
        xyz, sigma = _cloud(xyz), _cloud(sigma)
        if xyz.shape != sigma.shape:
            raise ValueError('points and sigma differ in shape')
        out = np.empty(xyz.shape, np.float64)
        if xyz.shape[0]:
            self.check(self.L.nwg_displace(self.h, _p(xyz), _p(sigma), xyz.shape[0], int(seed), int(stream), _p(out)), 'nwg_displace')
        return out

    def smlmify(self, xyz, sigma, sz=None, seed=0, streams=(STREAM_COPY_DISPLACE, STREAM_COPY_KEY, STREAM_COPY_PHOTONS), model='exponential',
                psf_width=250.0, mean_photon_count=300, bg_photon_count=20):
        """-> (points (sz,3), sigma (sz,3), copy (sz,) int64): copy j = c n + i is copy c of point i."""
        xyz, sigma = _cloud(xyz), _cloud(sigma)
        if xyz.shape != sigma.shape or xyz.shape[0] == 0:
            raise ValueError('points and sigma are two (n,3) arrays, n >= 1')
        sz = xyz.shape[0] if sz is None else int(sz)
        out, sig, copy = np.empty((sz, 3), np.float64), np.empty((sz, 3), np.float64), np.empty(sz, np.int64)
        self.check(self.L.nwg_smlmify(self.h, _p(xyz), _p(sigma), xyz.shape[0], sz, int(seed), int(streams[0]), int(streams[1]), int(streams[2]),
                                      _model(model), _p(_psf(psf_width)), float(mean_photon_count), float(bg_photon_count), _p(out), _p(sig), _p(copy)),
                   'nwg_smlmify')
        return out, sig, copy

    def background(self, lo, hi, n, seed=0, stream=STREAM_BG_POSITION):
        lo, hi = np.ascontiguousarray(lo, np.float64).reshape(3), np.ascontiguousarray(hi, np.float64).reshape(3)
        out = np.empty((int(n), 3), np.float64)
        if int(n):
            self.check(self.L.nwg_background(self.h, _p(lo), _p(hi), int(n), int(seed), int(stream), _p(out)), 'nwg_background')
        return out


class _borrowed(object):
    """`with _borrowed(context, device) as ctx`: the caller's context, or one of its own that is closed on the way out."""

    def __init__(self, context, device):
        self.own = context is None
        self.ctx = SimulationContext(device) if self.own else context

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        if self.own:
            self.ctx.close()


# ---- upstream's functions -----------------------------------------------------------------------------------------------------------
def points_from_sdf(shape, r_max=None, centre=None, dx_min=1.0, p=0.1, seed=0, project=2, lipschitz=LIPSCHITZ, start_level=-1,
                    max_points=1 << 27, return_keys=False, context=None, device=0):
    """In the place of PYME.simulation.locify.points_from_sdf(sdf, r_max, centre, dx_min, p) as Shape.points calls it (shape.py:75-76) --
    NOT PYME's octree sampler, see the module docstring.  `shape` is a Program (or a shape name / a shape of this module); r_max and centre
    default to the program's own enclosing cube (plus one lattice pitch).  Returns (n,3) float64 in ascending node key (upstream: (3,n))."""
    prog = _program(shape)
    centre = prog.centre if centre is None else centre
    r_max = prog.r_max + float(dx_min) if r_max is None else r_max
    with _borrowed(context, device) as ctx:
        ctx.set_program(prog)
        return ctx.sample_surface(centre, r_max, dx_min, p, seed=seed, lipschitz=lipschitz, start_level=start_level, project=project,
                                  max_points=max_points, return_keys=return_keys)


def loc_error(shape, model=None, seed=0, stream=STREAM_PHOTONS, context=None, device=0, **kw):
    """util.loc_error (util.py:37-47): sigma of shape (n,3).  model 'exponential': per localization and axis a photon number
    l = bg_photon_count + Exp(mean_photon_count) and sigma = (psf_width / 2.355) / sqrt(l); psf_width a number or three.  Upstream draws
    Exp(mean), drops every l <= bg and takes the first n: the same distribution, because the exponential is memoryless (l - bg, given
    l > bg, is again Exp(mean)).  Any other model: 10.0 everywhere, as upstream."""
    if len(shape) != 2 or int(shape[1]) != 3:
        raise ValueError('shape is (n, 3)')
    if model != 'exponential':
        return 10.0 * np.ones((int(shape[0]), 3))
    with _borrowed(context, device) as ctx:
        return ctx.loc_error(int(shape[0]), seed=seed, stream=stream, model=model, psf_width=kw['psf_width'],
                             mean_photon_count=kw['mean_photon_count'], bg_photon_count=kw['bg_photon_count'])


def smlmify_points(points, sigma, psf_width=250.0, mean_photon_count=300, bg_photon_count=20, max_points_per_cluster=10, max_points=None, seed=0,
                   streams=(STREAM_COPY_DISPLACE, STREAM_COPY_KEY, STREAM_COPY_PHOTONS), return_copies=False, context=None, device=0):
    """evaluation_utils.smlmify_points (:265-282): ten displaced copies of every point, `max_points` (default: as many as there were
    points) of them chosen uniformly without replacement -- in copy order here, in the order of the draw upstream --, and a freshly drawn
    sigma for each (not its source's: upstream's behaviour)."""
    if int(max_points_per_cluster) != COPIES:
        raise ValueError('max_points_per_cluster is %d on the device' % COPIES)
    with _borrowed(context, device) as ctx:
        out, sig, copy = ctx.smlmify(points, sigma, sz=max_points, seed=seed, streams=streams, psf_width=psf_width,
                                     mean_photon_count=mean_photon_count, bg_photon_count=bg_photon_count)
    return (out, sig, copy) if return_copies else (out, sig)


def generate_smlm_pointcloud_from_shape(shape_name, shape_params=None, density=1, p=1e-4, psf_width=250.0, mean_photon_count=300, bg_photon_count=20,
                                        noise_fraction=0.1, seed=0, return_truth=False, project=2, context=None, device=0):
    """evaluation_utils.generate_smlm_pointcloud_from_shape (:182-263) -> (points, normals, sigma), float64, upstream's control flow:
    fluorophores on the surface (`points_from_sdf`, lattice pitch density^(-1/3), shape.py:75-76), a localization error for each and a
    displacement by it (shape.py:77-79); psf_width None returns here with the undisturbed points, their normals and sigma None; else
    clusters (`smlmify_points`), then -- noise_fraction > 0 -- int(no n / (1 - no)) background points uniform in the cloud's box scaled
    by 1.2 about the origin, with their own sigma and clusters, stacked after the shape's; normals are sdf_normals at the final points.
    return_truth adds a dict: `source` (the fluorophore a point is a copy of; -1 - k for a copy of background point k), `clean` (the
    position the copy was displaced from) and `sigma_used` (the sigma it was displaced by -- not the point's own, fresh, sigma)."""
    prog = _program(shape_name, shape_params)
    dx = (1.0 / float(density)) ** (1.0 / 3.0)
    model = dict(psf_width=psf_width, mean_photon_count=mean_photon_count, bg_photon_count=bg_photon_count)
    with _borrowed(context, device) as ctx:
        ctx.set_program(prog)
        pts = ctx.sample_surface(prog.centre, prog.r_max + dx, dx, p, seed=seed, project=project)
        n = pts.shape[0]
        if n == 0:
            raise ValueError('no fluorophore was detected (density %g, p %g): nothing to simulate' % (density, p))
        if psf_width is None:
            out = (pts, ctx.normals(pts), None)
            return out + (dict(source=np.arange(n), clean=pts.copy(), sigma_used=None),) if return_truth else out
        sigma0 = ctx.loc_error(n, seed=seed, stream=STREAM_PHOTONS, **model)
        pts = ctx.displace(pts, sigma0, seed=seed, stream=STREAM_DISPLACE)
        points, sigma, copy = ctx.smlmify(pts, sigma0, seed=seed, **model)
        source = copy % n
        clean, used = pts[source], sigma0[source]
        if noise_fraction > 0:
            no, scale = float(noise_fraction), 1.2
            lo, hi = scale * points.min(0), scale * points.max(0)                    # evaluation_utils.py:233-238: about the origin
            ln = int(no * len(points) / (1.0 - no))
            if ln > 0:
                bg = ctx.background(lo, hi, ln, seed=seed, stream=STREAM_BG_POSITION)
                bg_sigma = ctx.loc_error(ln, seed=seed, stream=STREAM_BG_PHOTONS, **model)
                bp, bs, bcopy = ctx.smlmify(bg, bg_sigma, seed=seed, streams=(STREAM_BG_COPY_DISPLACE, STREAM_BG_COPY_KEY, STREAM_BG_COPY_PHOTONS), **model)
                points, sigma = np.vstack([points, bp]), np.vstack([sigma, bs])
                source = np.concatenate([source, -1 - bcopy % ln])
                clean, used = np.vstack([clean, bg[bcopy % ln]]), np.vstack([used, bg_sigma[bcopy % ln]])
        normals = ctx.normals(points)
    out = (points, normals, sigma)
    return out + (dict(source=source, clean=clean, sigma_used=used),) if return_truth else out


# ---- recipe-module mirror (recipe_modules/simulation.py:11-61) -----------------------------------------------------------------------
def parse_shape_params(shape_params):
    """A dict as it is; a string by ast.literal_eval, and by yaml (as upstream, :34) only if that fails and yaml can be imported."""
    if isinstance(shape_params, dict):
        return dict(shape_params)
    try:
        out = ast.literal_eval(str(shape_params))
    except (ValueError, SyntaxError):
        try:
            import yaml
        except ImportError:
            raise ValueError('shape_params %r is not a Python literal (and yaml is not installed)' % (shape_params,))
        out = yaml.safe_load(str(shape_params))
    if not isinstance(out, dict):
        raise ValueError('shape_params must describe a dict, got %r' % (shape_params,))
    return out


class PointcloudFromShape(object):
    """Mirror of the recipe module `PointcloudFromShape` (:11-61) in the plain-attribute style of ShrinkwrapMembrane: upstream's trait names
    and defaults (:13-25) -> under `output` a table like PointsFromMesh's: x y z xn yn zn and, unless no_jitter, sigma error_x error_y error_z."""

    def __init__(self, **kw):
        self.output = 'two_toruses'
        self.shape_name = 'TwoToruses'
        self.shape_params = "{'r': 30, 'R': 100}"
        self.density = 1.0
        self.p = 0.01
        self.psf_width_x, self.psf_width_y, self.psf_width_z = 280.0, 280.0, 840.0
        self.mean_photon_count = 600
        self.bg_photon_count = 20
        self.noise_fraction = 0.1
        self.no_jitter = False
        self.seed = 0                              # not a trait upstream (it draws from numpy's global state)
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        psf_width = None if self.no_jitter else (self.psf_width_x, self.psf_width_y, self.psf_width_z)
        points, normals, sigma = generate_smlm_pointcloud_from_shape(
            self.shape_name, parse_shape_params(self.shape_params), density=self.density, p=self.p, psf_width=psf_width,
            mean_photon_count=self.mean_photon_count, bg_photon_count=self.bg_photon_count, noise_fraction=self.noise_fraction, seed=self.seed,
            device=self.device)
        table = {'x': points[:, 0], 'y': points[:, 1], 'z': points[:, 2], 'xn': normals[:, 0], 'yn': normals[:, 1], 'zn': normals[:, 2]}
        if not self.no_jitter:
            table.update(sigma=np.sqrt((sigma * sigma).sum(1)), error_x=sigma[:, 0], error_y=sigma[:, 1], error_z=sigma[:, 2])
        namespace[self.output] = table
        return table
