"""CPU test: libnanowrap_hip.so exports every function include/nw_rays.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction, its kernels stay within their budgets without scratch, and the calls check
their arguments before they touch a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_rc_first', 'k_rc_count', 'k_rc_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_rays.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwc_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_rays_header():
    from ch_shrinkwrap_amd import build, _lib, rays
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) == 7
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(rays.SYMBOLS) == names
    assert rays.load().nwc_abi_version() == rays.ABI_VERSION == 1
    # the constants the binding repeats
    txt = open(os.path.join(ROOT, 'include', 'nw_rays.h')).read()
    for name in ('NWC_COUNT', 'NWC_STATS', 'NWC_INFO_EXITS'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(rays, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH'):
        assert int(re.search(r'NWC_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(rays, 'NWC_ERR_' + name)
        assert getattr(rays, 'NWC_ERR_' + name) in rays.ERRORS
    # ... and the ones the core header and the restatement repeat
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_rays_core.h')).read()
    assert int(re.search(r'#define NWC_INFO_EXITS\s+(\d+)', core).group(1)) == rays.NWC_INFO_EXITS
    import mesh_rays_ref as R
    # (the enlargement of rho_f is the face grid's one constant, which the core header names)
    assert re.search(r'#define NWC_RHO_SLACK\s+(\S+)', core).group(1) == 'BQ_FACE_RHO_SLACK'
    bq_core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_bq_core.h')).read()
    assert float(re.search(r'#define BQ_FACE_RHO_SLACK\s+(\S+)', bq_core).group(1)) == R.RHO_SLACK and R.EXITS == rays.NWC_INFO_EXITS
    assert rays.MAX_RAYS_PER_CALL == 1 << 22


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_RAYS]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    deps = unit[0][2]
    for core in ('nw_rays_core.h', 'nw_intersections_core.h'):                              # rebuilt when either core changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_rays.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_RAYS in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_RAYS)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert not [k for k in build.KERNEL_BUDGETS if k.startswith('k_rc_') and k not in KERNELS]
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)


def test_the_core_reuses_the_intersection_core():
    """the vectors, the products and the centroid are nw_intersections_core.h's, included and not copied; the unit is its own object"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_rays_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_intersections_core.h']              # HIP-free
    assert not re.search(r'\b(struct\s+nwx_|nwx_\w+\s*\([^;{]*\)\s*\{)', core)                           # no nwx_ definition of its own
    assert not [k for k in build.kernel_resources(build.OBJ_INTERSECTIONS) if k.startswith('k_rc_')]
    assert not [k for k in build.kernel_resources(build.OBJ_RAYS) if k.startswith('k_mx_')]


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the mesh, the rays' sizes, t_max and the flags comes
    before the first use of the context."""
    from ch_shrinkwrap_amd import rays as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros((4, 3), np.float32)
    pos[1, 0] = pos[2, 1] = pos[3, 2] = 10.0
    faces = np.array([[0, 2, 1], [0, 1, 3]], np.int32)
    assert L.nwc_set_mesh(None, p(pos), 4, p(faces), 2) == C.NWC_ERR_BADARG                              # all is well but the context
    assert L.nwc_set_mesh(None, None, 4, p(faces), 2) == C.NWC_ERR_BADARG
    assert L.nwc_set_mesh(None, p(pos), 4, None, 2) == C.NWC_ERR_BADARG
    assert L.nwc_set_mesh(None, p(pos), 4, p(faces), 0) == C.NWC_ERR_BADARG
    assert L.nwc_set_mesh(None, p(pos), 2, p(faces), 2) == C.NWC_ERR_BADARG
    assert L.nwc_set_mesh(None, p(pos), 4, p(np.array([[0, 1, 4], [0, 1, 2]], np.int32)), 2) == C.NWC_ERR_BADARG
    assert L.nwc_set_mesh(None, p(pos), 4, p(np.array([[0, 1, -1], [0, 1, 2]], np.int32)), 2) == C.NWC_ERR_BADARG
    nan = pos.copy()
    nan[2, 1] = np.inf
    assert L.nwc_set_mesh(None, p(nan), 4, p(faces), 2) == C.NWC_ERR_NONFINITE
    o, d = np.zeros((2, 3)), np.ones((2, 3))
    t, hits = np.full(2, -7.0), np.full(2, -7, np.int32)
    cast = lambda o_, d_, n, t_max, flags, hits_=None: L.nwc_cast(None, o_, d_, n, None, None, t_max, flags, p(t), None, None, hits_)
    assert cast(p(o), p(d), 2, np.inf, 0) == C.NWC_ERR_BADARG                                            # all is well but the context
    assert cast(None, p(d), 2, np.inf, 0) == C.NWC_ERR_BADARG and cast(p(o), None, 2, np.inf, 0) == C.NWC_ERR_BADARG
    assert cast(p(o), p(d), 0, np.inf, 0) == C.NWC_ERR_BADARG and cast(p(o), p(d), (1 << 30) + 1, np.inf, 0) == C.NWC_ERR_BADARG
    assert cast(p(o), p(d), 2, np.inf, 4) == C.NWC_ERR_BADARG                                            # an unknown flag
    assert cast(p(o), p(d), 2, -1.0, 0) == C.NWC_ERR_BADARG and cast(p(o), p(d), 2, np.nan, 0) == C.NWC_ERR_BADARG
    assert cast(p(o), p(d), 2, np.inf, 0, p(hits)) == C.NWC_ERR_BADARG                                   # hits without NWC_COUNT
    assert (t == -7.0).all() and (hits == -7).all()
    assert L.nwc_get_stats(None, p(np.zeros(3, np.int64))) == C.NWC_ERR_BADARG
    h = ctypes.c_void_p()
    assert L.nwc_create(-1, ctypes.byref(h)) == C.NWC_ERR_BADARG and L.nwc_create(0, None) == C.NWC_ERR_BADARG


def test_the_cone_of_directions():
    """the spherical-Fibonacci cap of thickness(): unit vectors, inside the cone, the written-down angles, about any axis"""
    from ch_shrinkwrap_amd import rays as C
    rng = np.random.default_rng(2)
    axis = rng.normal(size=(50, 3))
    axis[:3] = np.eye(3)
    axis[3] = [0.0, 0.0, -1.0]
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    assert np.array_equal(C.cone_directions(axis, 1, 120.0)[:, 0], axis)
    K = 30
    d = C.cone_directions(axis, K, 120.0)
    assert d.shape == (50, K, 3) and np.abs(np.linalg.norm(d, axis=2) - 1.0).max() < 1e-12
    cos_t = (d * axis[:, None, :]).sum(2)
    want = 1.0 - (np.arange(K) + 0.5) / K * (1.0 - np.cos(np.radians(60.0)))
    assert np.abs(cos_t - want[None, :]).max() < 1e-12 and cos_t.min() > 0.5
    # the azimuth advances by the golden angle in the frame built from the axis's smallest component
    e = np.zeros_like(axis)
    e[np.arange(50), np.argmin(np.abs(axis), axis=1)] = 1.0
    u = e - (e * axis).sum(1)[:, None] * axis
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(axis, u)
    phi = np.arctan2((d * w[:, None, :]).sum(2), (d * u[:, None, :]).sum(2))
    want_phi = np.arange(K) * np.pi * (3.0 - np.sqrt(5.0))
    assert np.abs(np.angle(np.exp(1j * (phi - want_phi[None, :])))).max() < 1e-9


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import rays as C
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    with pytest.raises(RuntimeError):
        C.cast_rays((v, f), np.zeros((1, 3)), np.ones((1, 3)))
    with pytest.raises(RuntimeError):
        C.thickness(TriMesh(v, f))
    with pytest.raises(RuntimeError):
        TriMesh(v, f).thickness(n_rays=30)
    with pytest.raises(RuntimeError):
        C.inside(np.zeros((1, 3)), (v, f))
    with pytest.raises(RuntimeError):
        C.MeshThickness().execute({'membrane': TriMesh(v, f)})
