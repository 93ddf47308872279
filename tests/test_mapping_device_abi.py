"""CPU test: libnanowrap_hip.so exports every function include/nw_mapping.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header and the two under it, its kernels stay
within their budgets without scratch, the calls check their arguments before they touch a GPU, and nothing falls back to the host."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_lm_face_setup', 'k_lm_map', 'k_lm_totals']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_mapping.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwl_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_mapping_header():
    from ch_shrinkwrap_amd import build, _lib, mapping
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ['nwl_abi_version', 'nwl_create', 'nwl_destroy', 'nwl_get_areas', 'nwl_last_error', 'nwl_map', 'nwl_set_mesh']
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(mapping.SYMBOLS) == names
    assert mapping.load().nwl_abi_version() == mapping.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_mapping.h')).read()
    for name in ('NWL_ACCUMULATE', 'NWL_WALK_ONLY', 'NWL_INFO_WORDS', 'NWL_INFO_IN_BAND', 'NWL_INFO_RINGS', 'NWL_INFO_CENTROIDS', 'NWL_INFO_CELLS',
                 'NWL_INFO_CELL_SIZE'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(mapping, name)
    assert int(re.search(r'#define NWL_MAX_VALUE_COLUMNS\s+(\d+)', txt).group(1)) == mapping.MAX_COLUMNS == 8
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH', 'RANGE'):
        assert int(re.search(r'NWL_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(mapping, 'NWL_ERR_' + name)
        assert getattr(mapping, 'NWL_ERR_' + name) in mapping.ERRORS
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_mapping_core.h')).read()
    assert int(re.search(r'#define NWL_W_ONE\s+(\d+)', core).group(1)) == mapping.W_ONE == 1 << 20
    assert int(re.search(r'#define NWL_Q_SHIFT\s+(\d+)', core).group(1)) == 30 and mapping.Q_ONE == 1 << 30 and mapping.CHUNK == 1 << 22


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_MAPPING]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_mapping.hip') and build.OBJ_MAPPING.endswith('nw_mapping.o')
    deps = unit[0][2]
    for core in ('nw_mapping_core.h', 'nw_volume_core.h', 'nw_distance_core.h'):                  # rebuilt when any of the three changes
        assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', core) in deps
    assert os.path.join(ROOT, 'include', 'nw_mapping.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_MAPPING in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_MAPPING)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert not [k for k in build.KERNEL_BUDGETS if k.startswith('k_lm_') and k not in KERNELS]
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)
    assert build.KERNEL_BUDGETS['k_lm_map'][0] == build.KERNEL_BUDGETS['k_vx_nodes'][0] == 128      # four waves per SIMD


def test_the_unit_is_new_and_the_core_reuses_the_two_cores():
    """the capped walk and the band rule are nw_volume_core.h's and the point-triangle arithmetic nw_distance_core.h's: included and not
    copied; the kernels are in an object of their own, and no other unit has gained or lost one"""
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_mapping_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['nw_volume_core.h']                       # HIP-free
    assert not re.search(r'NWD_HD\s+[\w ]+\bnw[dv]_\w+\s*\(', core)                                      # no nwd_ / nwv_ definition of its own
    assert len(re.findall(r'NWD_HD\s+[\w ]+\bnwl_\w+\s*\(', core)) >= 8
    for name in ('nwv_walk', 'nwv_in_band', 'nwd_dot'):
        assert name + '(' in core
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_mapping.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert '"nw_mapping_core.h"' in src and '"nw_bq.h"' in src and 'nwl_locate(' in code and 'nwd_face_centroid(' in code
    assert '"nw_volume.h"' not in src and '"nw_distance.h"' not in src
    assert 'atomicAdd(' in code and not re.search(r'atomicAdd\(\s*\(?(float|double)', code) and 'atomicCAS' not in code      # integer adds only
    for obj in (build.OBJ_DISTANCE, build.OBJ_VOLUME, build.OBJ_PROXIMITY, build.OBJ_BQ):
        assert not [k for k in build.kernel_resources(obj) if k.startswith('k_lm_')]
    assert not [k for k in build.kernel_resources(build.OBJ_MAPPING) if not k.startswith('k_lm_')]
    for tree in ('include', 'ch_shrinkwrap_amd'):                                                         # the prefix is this unit's alone
        for d, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith(('.h', '.hip', '.cpp', '.py')) and 'mapping' not in fn and fn != 'build.py' and fn != 'trimesh.py':
                    assert not re.search(r'\bnwl_\w+\s*\(', open(os.path.join(d, fn), errors='replace').read()), fn


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the mesh, the cloud, the columns, the scales, the band and the
    flags comes before the first use of the context."""
    from ch_shrinkwrap_amd import mapping as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros((4, 3), np.float32)
    pos[1, 0] = pos[2, 1] = pos[3, 2] = 10.0
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    BAD = C.NWL_ERR_BADARG
    assert L.nwl_set_mesh(None, p(pos), 4, p(faces), 4) == BAD                                           # all is well but the context
    assert L.nwl_set_mesh(None, None, 4, p(faces), 4) == BAD and L.nwl_set_mesh(None, p(pos), 4, None, 4) == BAD
    assert L.nwl_set_mesh(None, p(pos), 4, p(faces), 0) == BAD and L.nwl_set_mesh(None, p(pos), 2, p(faces), 4) == BAD
    assert L.nwl_set_mesh(None, p(pos), 4, p(np.array([[0, 1, 4], [0, 1, 2]], np.int32)), 2) == BAD
    assert L.nwl_set_mesh(None, p(pos), 4, p(np.array([[0, 1, -1], [0, 1, 2]], np.int32)), 2) == BAD
    nan = pos.copy()
    nan[2, 1] = np.inf
    assert L.nwl_set_mesh(None, p(nan), 4, p(faces), 4) == C.NWL_ERR_NONFINITE
    assert L.nwl_get_areas(None, None) == BAD and L.nwl_get_areas(None, p(np.zeros(4, np.uint64))) == BAD
    xyz, vals, sc = np.ones((5, 3)), np.ones((5, 2)), np.array([1.0, 2.0])
    outs = [np.full(5, -7, np.int32), np.full(15, -7, np.int32), np.full(5, -7.0), np.full(15, -7.0), np.full(4, 7, np.uint64), np.full(4, -7, np.int32),
            np.full(8, -7, np.int64), np.full(8, 7, np.uint64), np.full(C.NWL_INFO_WORDS, -7, np.int64)]

    def m(xyz_=p(xyz), n=5, vals_=p(vals), ncol=2, sc_=p(sc), band=30.0, flags=0):
        return L.nwl_map(None, xyz_, n, vals_, ncol, sc_, band, flags, *[p(o) for o in outs])
    assert m() == BAD                                                                                    # all is well but the context
    assert m(xyz_=None) == BAD and m(n=0) == BAD and m(n=(1 << 30) + 1) == BAD
    assert m(ncol=-1) == BAD and m(ncol=9) == BAD and m(vals_=None) == BAD and m(sc_=None) == BAD
    assert m(flags=4) == BAD and m(flags=C.NWL_ACCUMULATE | C.NWL_WALK_ONLY) == BAD
    for bad in ([1.0, 3.0], [0.0, 1.0], [-2.0, 1.0], [np.inf, 1.0], [np.nan, 1.0], [1.0, 2.0 ** 950]):
        assert m(sc_=p(np.array(bad))) == BAD
    for band in (0.0, -3.0, np.nan, np.inf, -np.inf, 2.0 ** 40 * 1.5):
        assert m(band=band) == BAD
    assert all((o == o.flat[0]).all() and abs(int(o.flat[0])) == 7 for o in outs)                        # nothing was written
    h = ctypes.c_void_p()
    assert L.nwl_create(-1, ctypes.byref(h)) == BAD and L.nwl_create(0, None) == BAD
    assert L.nwl_last_error(None) == b'null ctx'


def test_the_scale_the_binding_picks():
    from ch_shrinkwrap_amd.mapping import column_scale
    assert column_scale([0.0, 0.0]) == 1.0 and column_scale([]) == 1.0
    assert column_scale([3.0, -5.0]) == 8.0 and column_scale([4.0]) == 4.0 and column_scale([-4.0, 1.0]) == 4.0
    assert column_scale([0.3]) == 0.5 and column_scale([0.25]) == 0.25 and column_scale([1e6]) == 2.0 ** 20
    assert column_scale([1.0, np.nan, np.inf]) == 1.0
    assert column_scale([np.nextafter(4.0, 5.0)]) == 8.0 and column_scale([5e-324]) == 5e-324


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import mapping as C
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    pts = (v[:40] * 1.01).astype(np.float64)
    with pytest.raises(RuntimeError):
        C.MappingContext()
    with pytest.raises(RuntimeError):
        C.map_to_surface(pts, (v, f))
    with pytest.raises(RuntimeError):
        C.surface_density(pts, TriMesh(v, f), band=3.0, values={'t': np.arange(40.0)})
    with pytest.raises(RuntimeError):
        TriMesh(v, f).surface_density(pts, band=3.0)
    with pytest.raises(RuntimeError):
        C.SurfaceDensity().execute({'membrane': TriMesh(v, f), 'filtered_localizations': {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2]}})
    assert not [n for n in dir(C) if 'scipy' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]


def test_the_recipe_class_has_the_written_down_defaults():
    from ch_shrinkwrap_amd import mapping as C
    m = C.SurfaceDensity()
    assert (m.input_mesh, m.input_points, m.band, m.columns, m.smooth, m.output, m.output_points) == (
        'membrane', 'filtered_localizations', 30.0, [], 0, 'membrane_density', 'mapped_localizations')
    assert C.SurfaceDensity(band=12.0).band == 12.0
    with pytest.raises(AttributeError):
        C.SurfaceDensity(bandd=3.0)
