"""
A fitted membrane as a volume: ctypes binding of include/nw_volume.h (kernels in libnanowrap_hip.so, csrc/nw_volume.hip) and what sits
on top of it.

The exact signed distance from the nodes of a voxel lattice to the mesh's triangles, clamped to a band +-d_cap: every node within the
band carries what distance_to_mesh gives there, bit for bit; every node beyond it carries +-d_cap with the sign of the side it lies
on, taken from its predecessor on a fixed path through the lattice (csrc/nw_volume_core.h says why that is right for a closed
embedded surface, and that for an open or self-crossing one the result is defined, not meaningful).  The nodes are made on the device;
no list of query points exists.

    VolumeContext            one nwv_ctx: set_mesh once, volume as often as needed
    signed_distance_volume   one call: a mesh and a voxel size (or another channel's voxel grid) in, sd / face / mask out
    voxelize                 the bool inside mask
    offset_surface           the level set sd = offset as a mesh: the field goes to the surface nets (isosurface.py) on the device
    MeshToVolume, OffsetSurface   the recipe-module surfaces

Everything runs on the device; there is no host fallback: without a GPU the context cannot be made and every entry raises.
"""
import ctypes

import numpy as np

from . import _lib

SYMBOLS = ['nwv_abi_version', 'nwv_create', 'nwv_destroy', 'nwv_last_error', 'nwv_set_mesh', 'nwv_volume', 'nwv_field_ptr',
           'nwv_get_field']
ABI_VERSION = 1
NWV_OK, NWV_ERR_BADARG, NWV_ERR_HIP, NWV_ERR_NONFINITE, NWV_ERR_NOMEM, NWV_ERR_NOMESH = 0, -1, -2, -3, -4, -5
ERRORS = {NWV_ERR_BADARG: 'bad argument', NWV_ERR_HIP: 'HIP runtime error (is a GPU visible?)', NWV_ERR_NONFINITE: 'non-finite coordinate',
          NWV_ERR_NOMEM: 'out of device memory', NWV_ERR_NOMESH: 'the context holds no mesh'}
NWV_SIGNED = 1
NWV_FIELD_SHIFT = 20                              # field = floor((d_cap - sd) * 2^20)
NWV_INFO_WORDS = 8
(NWV_INFO_FLAGS, NWV_INFO_IN_BAND, NWV_INFO_RINGS_NEAR, NWV_INFO_CENTROIDS_NEAR, NWV_INFO_RINGS_FAR, NWV_INFO_CENTROIDS_FAR, NWV_INFO_CELLS,
 NWV_INFO_SEED_FACE) = range(8)
NWV_FLAG_FAN_CAPPED = 1

_L = None


def load():
    """The library's nwv_ entry points."""
    global _L
    if _L is None:
        vp, i32, i64, f32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
        L = _lib.load_entry_points(SYMBOLS, {
            'nwv_abi_version': [], 'nwv_create': [i32, ctypes.POINTER(vp)], 'nwv_destroy': [vp], 'nwv_last_error': [vp],
            'nwv_set_mesh': [vp, vp, i64, vp, i64, vp],
            'nwv_volume': [vp, vp, f32, vp, f64, i32, vp, vp, vp, vp],
            'nwv_field_ptr': [vp], 'nwv_get_field': [vp, vp]}, 'nwv_abi_version', ABI_VERSION, 'nw_volume')
        L.nwv_field_ptr.restype = vp                      # (the one entry point that returns a pointer)
        _L = L
    return _L


_p = _lib.ptr


def field_threshold(d_cap, offset):
    """the level sd = offset in the field's units: floor((d_cap - offset) * 2^20)"""
    return int(np.floor((float(d_cap) - float(offset)) * float(1 << NWV_FIELD_SHIFT)))


class VolumeContext(_lib.QueryContext):
    """One nwv_ctx: a mesh taken in once by set_mesh, its face centroids kept on the device, and any number of volumes of it."""
    prefix, errors, gpu_only, load = 'nwv_', ERRORS, 'the signed-distance volume runs', staticmethod(load)

    def __init__(self, device=0):
        _lib.QueryContext.__init__(self, device)
        self.n_faces = 0
        self.has_twin = False
        self.info = self.dims = None

    def set_mesh(self, vertices, faces=None, signed=True):
        """Take a mesh in: a TriMesh / MembraneMesh (faces None) or float32 vertices and int32 faces.  With signed=True the twin table
        comes from the mesh's half-edge records or from nwr_halfedge_twins; a non-manifold edge has none and raises."""
        from .distance import _mesh_arrays
        pos, f, tw = _mesh_arrays(vertices if faces is None else (vertices, faces), bool(signed))
        self.n_faces, self.has_twin = 0, False
        self.check(self.L.nwv_set_mesh(self.h, _p(pos), pos.shape[0], _p(f), f.shape[0], _p(tw)), 'nwv_set_mesh')
        self.n_faces, self.has_twin = f.shape[0], tw is not None
        return self

    def volume(self, lo, h, dims, d_cap, signed=True, return_face=False, return_mask=False, return_sd=True):
        """The banded signed distance at the nodes lo + (index + 1/2) h of a dims[0] x dims[1] x dims[2] lattice: sd float64 [z, y, x]
        (None with return_sd=False), with return_face / return_mask a tuple (sd[, face int32][, mask bool]).  The arrays and the
        uint64 field stay on the device (field_pointer); self.info holds the call's counters."""
        lo = np.ascontiguousarray(lo, np.float32).reshape(3)
        dims = np.ascontiguousarray(dims, np.int32).reshape(3)
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        ok = min(shape) >= 1 and shape[0] * shape[1] * shape[2] <= 1 << 30                # (the library refuses the rest before it writes)
        sd = np.empty(shape, np.float64) if return_sd and ok else None
        face = np.empty(shape, np.int32) if return_face and ok else None
        mask = np.empty(shape, np.uint8) if return_mask and ok else None
        info = np.zeros(NWV_INFO_WORDS, np.int64)
        self.check(self.L.nwv_volume(self.h, _p(lo), float(h), _p(dims), float(d_cap), NWV_SIGNED if signed else 0, _p(sd), _p(face), _p(mask),
                                     _p(info)), 'nwv_volume')
        n = shape[0] * shape[1] * shape[2]
        self.dims = dims
        self.info = dict(fan_capped=bool(info[NWV_INFO_FLAGS] & NWV_FLAG_FAN_CAPPED), in_band=int(info[NWV_INFO_IN_BAND]), nodes=n,
                         rings_near=int(info[NWV_INFO_RINGS_NEAR]), centroids_near=int(info[NWV_INFO_CENTROIDS_NEAR]),
                         rings_far=int(info[NWV_INFO_RINGS_FAR]), centroids_far=int(info[NWV_INFO_CENTROIDS_FAR]), cells=int(info[NWV_INFO_CELLS]),
                         seed_face=int(info[NWV_INFO_SEED_FACE]))
        out = (sd,) + ((face,) if return_face else ()) + ((mask.view(bool),) if return_mask else ())
        return out if len(out) > 1 else sd

    def field(self):
        """A host copy of the last volume's uint64 field, [z, y, x]: floor((d_cap - sd) * 2^20)."""
        if self.dims is None:
            raise RuntimeError('VolumeContext.field: volume first')
        out = np.empty((int(self.dims[2]), int(self.dims[1]), int(self.dims[0])), np.uint64)
        self.check(self.L.nwv_get_field(self.h, _p(out)), 'nwv_get_field')
        return out

    def field_pointer(self):
        """The device pointer of the last volume's uint64 field, as an int (0 if there is none)."""
        return int(self.L.nwv_field_ptr(self.h) or 0)


def _vertices(mesh):
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return np.asarray(mesh[0], np.float32).reshape(-1, 3)
    return np.asarray(mesh.vertices if hasattr(mesh, 'vertices') else mesh._vertices['position'], np.float32).reshape(-1, 3)


def signed_distance_volume(mesh, voxel_size, band=None, pad=None, lo=None, dims=None, signed=True, context=None, device=0):
    """dict(sd [z, y, x] float64, face int32, mask bool, lo, h, dims, d_cap) of a TriMesh / MembraneMesh or (vertices, faces).
    band: d_cap in nm, default 3 h.  The lattice is isosurface.grid_for(vertices, h, pad) with pad = ceil(band / h) + 2 voxels of
    margin, unless lo and dims give one (another channel's voxel grid).  context: a VolumeContext to use (it holds this mesh
    afterwards); one is made and closed otherwise."""
    from .isosurface import grid_for
    h = float(np.float32(voxel_size))
    d_cap = 3.0 * h if band is None else float(band)
    if (lo is None) != (dims is None):
        raise ValueError('signed_distance_volume: give both lo and dims, or neither')
    if lo is None:
        if not (h > 0 and np.isfinite(h) and np.isfinite(d_cap)):
            raise ValueError('signed_distance_volume: the voxel size must be positive and the band finite')
        pad = int(np.ceil(d_cap / h)) + 2 if pad is None else int(pad)
        lo, dims = grid_for(_vertices(mesh), h, pad)
    lo = np.ascontiguousarray(lo, np.float32).reshape(3)
    dims = np.ascontiguousarray(dims, np.int32).reshape(3)
    own = context is None
    ctx = VolumeContext(device) if own else context
    try:
        ctx.set_mesh(mesh, signed=signed)
        sd, face, mask = ctx.volume(lo, h, dims, d_cap, signed=signed, return_face=True, return_mask=True)
        info = ctx.info
    finally:
        if own:
            ctx.close()
    return dict(sd=sd, face=face, mask=mask, lo=lo, h=h, dims=dims, d_cap=d_cap, info=info)


def voxelize(mesh, voxel_size, pad=None, lo=None, dims=None, context=None, device=0):
    """The bool mask [z, y, x] of the lattice nodes inside a closed mesh; the band is one voxel, the narrowest the sweep allows."""
    h = float(np.float32(voxel_size))
    return signed_distance_volume(mesh, h, band=h, pad=pad, lo=lo, dims=dims, signed=True, context=context, device=device)['mask']


def offset_surface(mesh, offset, voxel_size=None, remesh=True, device=0):
    """The surface at signed distance `offset` nm from a closed mesh (positive: outwards), as an isosurface.Surface: the level set
    sd = offset of the banded volume with band |offset| + 2 h on a lattice with ceil(max(offset, 0) / h) + 2 voxels of margin,
    meshed by the surface nets of isosurface.py at thr = floor((d_cap - offset) 2^20).  The field goes from its kernel to
    IsosurfaceContext.set_field on the device and never visits the host.  voxel_size None: the mesh's mean edge length.
    remesh=True: three passes of remesh_device at the result's own mean edge length, as start_surface does."""
    from .distance import _mesh_arrays
    from .isosurface import IsosurfaceContext, Surface, grid_for, mean_edge_length
    offset = float(offset)
    pos, faces, _ = _mesh_arrays(mesh, False)
    h = float(np.float32(mean_edge_length(pos, faces) if voxel_size is None else voxel_size))
    if not (h > 0 and np.isfinite(h) and np.isfinite(offset)):
        raise ValueError('offset_surface: the voxel size must be positive and the offset finite')
    d_cap = abs(offset) + 2.0 * h
    pad = int(np.ceil(max(offset, 0.0) / h)) + 2
    lo, dims = grid_for(pos, h, pad)
    thr = field_threshold(d_cap, offset)
    vctx = VolumeContext(device)
    try:
        vctx.set_mesh(mesh, signed=True)
        vctx.volume(lo, h, dims, d_cap, signed=True, return_sd=False)
        info = dict(vctx.info, lo=lo, h=h, dims=dims, d_cap=d_cap, pad=pad, thr=thr, offset=offset)
        ictx = IsosurfaceContext(device)
        try:
            ictx.set_field(vctx.field_pointer(), lo, h, dims)
            v, f, keys = ictx.extract(thr, return_keys=True)
        finally:
            ictx.close()
    finally:
        vctx.close()
    info['keys'] = keys
    if remesh:
        from .remesh import remesh_device
        target = mean_edge_length(v, f)
        v, f = remesh_device(v, f, 3, target, 0.5, 0, device=device)
        info['target_edge_length'] = target
        info['keys'] = None
    return Surface(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), info)


class MeshToVolume(object):
    """Recipe-module surface for the volume of a fitted surface, in the plain-attribute style of MeshThickness: the mesh under `input`
    -> under `output` signed_distance_volume's dict (sd, face, mask, lo, h, dims, d_cap).  PYME is not in the reference tree: the
    traits and the keys here are this project's own."""

    def __init__(self, **kw):
        self.input, self.output = 'membrane', 'membrane_sdf'
        self.voxel_size, self.band, self.pad, self.lo, self.dims, self.signed = 10.0, None, None, None, None, True
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        out = signed_distance_volume(namespace[self.input], float(self.voxel_size), band=self.band, pad=self.pad, lo=self.lo, dims=self.dims,
                                     signed=bool(self.signed), device=self.device)
        namespace[self.output] = out
        return out


class OffsetSurface(object):
    """Recipe-module surface for the surface at `offset` nm from a fitted one: the mesh under `input` -> under `output` a surface with
    .vertices / .faces / .info (offset_surface)."""

    def __init__(self, **kw):
        self.input, self.output = 'membrane', 'offset_membrane'
        self.offset, self.voxel_size, self.remesh = 20.0, None, True
        self.device = 0
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError('unknown parameter %s' % k)
            setattr(self, k, v)

    def execute(self, namespace):
        out = offset_surface(namespace[self.input], float(self.offset), voxel_size=self.voxel_size, remesh=bool(self.remesh), device=self.device)
        namespace[self.output] = out
        return out
