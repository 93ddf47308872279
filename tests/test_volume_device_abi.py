"""CPU test: libnanowrap_hip.so exports every function include/nw_volume.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on both core headers, its kernels stay within their
budgets without scratch, the calls check their arguments before they touch a GPU, and nothing falls back to the host."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_vx_nodes', 'k_vx_seed', 'k_vx_sweep', 'k_vx_finish', 'k_vx_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_volume.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwv_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_volume_header():
    from ch_shrinkwrap_amd import build, _lib, volume
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) == 8
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(volume.SYMBOLS) == names
    assert volume.load().nwv_abi_version() == volume.ABI_VERSION == 1
    # the constants the binding repeats
    txt = open(os.path.join(ROOT, 'include', 'nw_volume.h')).read()
    for name in ('NWV_SIGNED', 'NWV_FIELD_SHIFT', 'NWV_INFO_WORDS', 'NWV_INFO_FLAGS', 'NWV_INFO_IN_BAND', 'NWV_INFO_RINGS_NEAR', 'NWV_INFO_CENTROIDS_NEAR',
                 'NWV_INFO_RINGS_FAR', 'NWV_INFO_CENTROIDS_FAR', 'NWV_INFO_CELLS', 'NWV_INFO_SEED_FACE', 'NWV_FLAG_FAN_CAPPED'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(volume, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH'):
        assert int(re.search(r'NWV_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(volume, 'NWV_ERR_' + name)
        assert getattr(volume, 'NWV_ERR_' + name) in volume.ERRORS
    # ... and the ones the core header, the restatement and the k-NN field repeat
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_volume_core.h')).read()
    assert int(re.search(r'#define NWV_FIELD_SHIFT\s+(\d+)', core).group(1)) == volume.NWV_FIELD_SHIFT == 20
    import mesh_volume_ref as V
    from ch_shrinkwrap_amd import neighbours
    assert V.FIELD_SHIFT == volume.NWV_FIELD_SHIFT == neighbours.FIELD_SHIFT
    assert volume.field_threshold(5.0, 1.5) == int(3.5 * 2 ** 20) and volume.field_threshold(3.0, -1.0) == 4 << 20


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_VOLUME]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_volume.hip') and build.OBJ_VOLUME.endswith('nw_volume.o')
    deps = unit[0][2]
    for core in ('nw_volume_core.h', 'nw_distance_core.h'):                                  # rebuilt when either core changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_volume.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_VOLUME in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_VOLUME)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert not [k for k in build.KERNEL_BUDGETS if k.startswith('k_vx_') and k not in KERNELS]
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)
        assert build.KERNEL_BUDGETS[k][0] <= build.KERNEL_BUDGETS['k_md_query'][0] == 128


def test_the_unit_is_new_and_the_core_reuses_the_distance_core():
    """the point-triangle distance, the pseudonormal and the sign are nw_distance_core.h's, included and not copied; the kernels are in
    an object of their own, and neither the distance unit nor the shared grid has gained one"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_volume_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_distance_core.h']                    # HIP-free
    assert not re.search(r'\bnwd_\w+\s*\([^;{]*\)\s*\{', core)                                           # no nwd_ definition of its own
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_volume.hip')).read()
    assert '"nw_volume_core.h"' in src and '"nw_bq.h"' in src and 'atomic' not in re.sub(r'//.*', '', src)
    assert not [k for k in build.kernel_resources(build.OBJ_DISTANCE) if k.startswith('k_vx_')]
    assert not [k for k in build.kernel_resources(build.OBJ_BQ) if k.startswith('k_vx_')]
    assert not [k for k in build.kernel_resources(build.OBJ_VOLUME) if not k.startswith('k_vx_')]


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the mesh, the lattice, the band and the flags comes before
    the first use of the context."""
    from ch_shrinkwrap_amd import volume as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros((4, 3), np.float32)
    pos[1, 0] = pos[2, 1] = pos[3, 2] = 10.0
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    import mesh_distance_ref as D
    twin = D.twins(faces)
    assert (twin >= 0).all()
    assert L.nwv_set_mesh(None, p(pos), 4, p(faces), 4, p(twin)) == C.NWV_ERR_BADARG                     # all is well but the context
    assert L.nwv_set_mesh(None, None, 4, p(faces), 4, p(twin)) == C.NWV_ERR_BADARG
    assert L.nwv_set_mesh(None, p(pos), 4, None, 4, None) == C.NWV_ERR_BADARG
    assert L.nwv_set_mesh(None, p(pos), 4, p(faces), 0, None) == C.NWV_ERR_BADARG
    assert L.nwv_set_mesh(None, p(pos), 2, p(faces), 4, None) == C.NWV_ERR_BADARG
    assert L.nwv_set_mesh(None, p(pos), 4, p(np.array([[0, 1, 4], [0, 1, 2]], np.int32)), 2, None) == C.NWV_ERR_BADARG
    assert L.nwv_set_mesh(None, p(pos), 4, p(np.array([[0, 1, -1], [0, 1, 2]], np.int32)), 2, None) == C.NWV_ERR_BADARG
    bad_twin = twin.copy()
    bad_twin[0] = bad_twin[1]                                                                            # not an involution
    assert L.nwv_set_mesh(None, p(pos), 4, p(faces), 4, p(bad_twin)) == C.NWV_ERR_BADARG
    bad_twin[0] = 12                                                                                     # outside [0, 3F)
    assert L.nwv_set_mesh(None, p(pos), 4, p(faces), 4, p(bad_twin)) == C.NWV_ERR_BADARG
    nan = pos.copy()
    nan[2, 1] = np.inf
    assert L.nwv_set_mesh(None, p(nan), 4, p(faces), 4, None) == C.NWV_ERR_NONFINITE
    lo, dims = np.zeros(3, np.float32), np.array([4, 5, 6], np.int32)
    sd, face, mask, info = np.full(120, -7.0), np.full(120, -7, np.int32), np.full(120, 7, np.uint8), np.full(8, -7, np.int64)
    vol = lambda lo_, h, dims_, d_cap, flags: L.nwv_volume(None, lo_, h, dims_, d_cap, flags, p(sd), p(face), p(mask), p(info))
    assert vol(p(lo), 1.0, p(dims), 3.0, 1) == C.NWV_ERR_BADARG                                          # all is well but the context
    assert vol(p(lo), 1.0, p(dims), 3.0, 0) == C.NWV_ERR_BADARG                                          # (NWV_SIGNED without twins: no context, no twins)
    assert vol(None, 1.0, p(dims), 3.0, 1) == C.NWV_ERR_BADARG and vol(p(lo), 1.0, None, 3.0, 1) == C.NWV_ERR_BADARG
    assert vol(p(lo), 1.0, p(dims), 3.0, 2) == C.NWV_ERR_BADARG                                          # an unknown flag
    for h in (0.0, -1.0, np.nan, np.inf):
        assert vol(p(lo), h, p(dims), 3.0, 1) == C.NWV_ERR_BADARG
    for d_cap in (np.nextafter(1.0, 0.0), 0.0, -3.0, np.nan, np.inf, np.nextafter(2.0 ** 40, np.inf)):   # below h, not finite, above 2^40
        assert vol(p(lo), 1.0, p(dims), d_cap, 1) == C.NWV_ERR_BADARG
    for bad in ([2, 5, 6], [4, 5, 0], [4, -1, 6], [4, 5, (1 << 20) + 1], [1 << 11, 1 << 10, 1 << 10]):   # dims < 3, too large, over 2^30 nodes
        assert vol(p(lo), 1.0, p(np.array(bad, np.int32)), 3.0, 1) == C.NWV_ERR_BADARG
    assert vol(p(np.array([0.0, np.nan, 0.0], np.float32)), 1.0, p(dims), 3.0, 1) == C.NWV_ERR_BADARG
    assert (sd == -7.0).all() and (face == -7).all() and (mask == 7).all() and (info == -7).all()
    assert not L.nwv_field_ptr(None)
    assert L.nwv_get_field(None, p(info)) == C.NWV_ERR_BADARG and L.nwv_get_field(None, None) == C.NWV_ERR_BADARG
    h = ctypes.c_void_p()
    assert L.nwv_create(-1, ctypes.byref(h)) == C.NWV_ERR_BADARG and L.nwv_create(0, None) == C.NWV_ERR_BADARG
    assert L.nwv_last_error(None) == b'null ctx'


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import volume as C
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    with pytest.raises(RuntimeError):
        C.VolumeContext()
    with pytest.raises(RuntimeError):
        C.signed_distance_volume((v, f), 2.0)
    with pytest.raises(RuntimeError):
        C.signed_distance_volume(TriMesh(v, f), 2.0, lo=[-12, -12, -12], dims=[12, 12, 12], signed=False)
    with pytest.raises(RuntimeError):
        C.voxelize((v, f), 2.0)
    with pytest.raises(RuntimeError):
        C.offset_surface((v, f), 3.0, voxel_size=2.0)
    for call in (lambda m: m.signed_distance_volume(2.0), lambda m: m.voxelize(2.0), lambda m: m.offset_surface(-2.0)):
        with pytest.raises(RuntimeError):
            call(TriMesh(v, f))
    with pytest.raises(RuntimeError):
        C.MeshToVolume(voxel_size=2.0).execute({'membrane': TriMesh(v, f)})
    with pytest.raises(RuntimeError):
        C.OffsetSurface().execute({'membrane': TriMesh(v, f)})


def test_the_recipe_classes_have_the_written_down_defaults():
    from ch_shrinkwrap_amd import volume as C
    m, o = C.MeshToVolume(), C.OffsetSurface()
    assert (m.input, m.output) == ('membrane', 'membrane_sdf')
    assert (o.input, o.output, o.offset) == ('membrane', 'offset_membrane', 20.0)
    with pytest.raises(AttributeError):
        C.OffsetSurface(ofset=3.0)
