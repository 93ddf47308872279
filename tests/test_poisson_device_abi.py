"""CPU test: libnanowrap_hip.so exports every function include/nw_poisson.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header, its kernels stay within their budgets
without scratch, the calls check their arguments before they touch a GPU, nothing falls back to the host, and the recipe module has
upstream's traits."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_sp_prepare', 'k_sp_mark', 'k_sp_count', 'k_sp_splat', 'k_sp_splat_lds', 'k_sp_splat_lds4', 'k_sp_system', 'k_sp_prolong', 'k_sp_relax', 'k_sp_residual', 'k_sp_absmax', 'k_sp_field']
# upstream's recipe_modules/surface_fitting.py ScreenedPoissonMesh, written out here: (trait, default)
UPSTREAM_TRAITS = [('k', 10), ('smoothiter', 0), ('flipflag', False), ('viewpos', [0, 0, 0]), ('visiblelayer', False), ('depth', 8), ('fulldepth', 5),
                   ('cgdepth', 0), ('scale', 1.1), ('samplespernode', 1.5), ('pointweight', 4), ('iters', 8), ('confidence', False), ('preclean', False),
                   ('threads', 8), ('use_normals', False)]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _declared():
    txt = re.sub(r'/\*.*?\*/', '', _read('include', 'nw_poisson.h'), flags=re.S)
    return sorted(set(re.findall(r'\b(nwo_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_poisson_header():
    from ch_shrinkwrap_amd import build, _lib, poisson
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == sorted(['nwo_abi_version', 'nwo_create', 'nwo_destroy', 'nwo_last_error', 'nwo_set_samples', 'nwo_plan', 'nwo_level_begin', 'nwo_relax',
                            'nwo_get_level', 'nwo_set_chi', 'nwo_solve', 'nwo_field', 'nwo_field_pointer', 'nwo_get_field'])
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(poisson.SYMBOLS) == names
    assert poisson.load().nwo_abi_version() == poisson.ABI_VERSION == 1
    txt, core = _read('include', 'nw_poisson.h'), _read('ch_shrinkwrap_amd', 'csrc', 'nw_poisson_core.h')
    for name in ('NWO_GET_W', 'NWO_GET_V', 'NWO_GET_RHS', 'NWO_GET_DIAG', 'NWO_GET_CHI', 'NWO_RESIDUAL_WORDS'):
        assert int(re.search(r'#define %s\s+(\d+)' % name, txt).group(1)) == getattr(poisson, name)
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'STATE', 'EMPTY'):
        assert int(re.search(r'NWO_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(poisson, 'NWO_ERR_' + name)
        assert getattr(poisson, 'NWO_ERR_' + name) in poisson.ERRORS


def test_the_constants_agree_in_the_three_places():
    """the core header, the binding and the restatement: NWO_MAX_N, the three quantisation exponents, the base level and the depth limits"""
    import screened_poisson_ref as R
    from ch_shrinkwrap_amd import poisson
    core = _read('ch_shrinkwrap_amd', 'csrc', 'nw_poisson_core.h')
    assert '#define NWO_MAX_N (1ll << 25)' in core and poisson.MAX_N == R.MAX_N == 1 << 25
    for name, attr in (('NWO_NORMAL_BITS', 'NORMAL_BITS'), ('NWO_WEIGHT_BITS', 'WEIGHT_BITS'), ('NWO_FIELD_BITS', 'FIELD_BITS'), ('NWO_BASE_LEVEL', 'BASE_LEVEL'),
                       ('NWO_MIN_DEPTH', 'MIN_DEPTH'), ('NWO_MAX_DEPTH', 'MAX_DEPTH')):
        assert int(re.search(r'#define %s\s+(\d+)' % name, core).group(1)) == getattr(poisson, attr) == getattr(R, attr), name
    assert (poisson.NORMAL_BITS, poisson.WEIGHT_BITS, poisson.FIELD_BITS, poisson.BASE_LEVEL, poisson.MIN_DEPTH, poisson.MAX_DEPTH) == (12, 7, 31, 2, 3, 9)
    assert float(re.search(r'#define NWO_W_ONE\s+([0-9.]+)', core).group(1)) == 2.0 ** 21 == float(R.W_ONE)
    assert float(re.search(r'#define NWO_V_ONE\s+([0-9.]+)', core).group(1)) == 2.0 ** 33 == R.V_ONE
    assert float(re.search(r'#define NWO_F_HALF\s+([0-9.]+)', core).group(1)) == 2.0 ** 31
    assert poisson.NWO_RESIDUAL_WORDS == 2 * (poisson.MAX_DEPTH + 1)
    for word in ('Proof', '2^58', '2^46', '2^62', 'NOT Kazhdan'):
        assert word in core
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['cmath', 'cstdint'] and 'fma(' not in core                 # HIP-free
    assert 'GiB at depth 9' in _read('include', 'nw_poisson.h')                                                              # the peak is stated


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_POISSON]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_poisson.hip') and build.OBJ_POISSON.endswith('nw_poisson.o')
    deps = unit[0][2]
    assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_poisson_core.h') in deps
    assert os.path.join(ROOT, 'include', 'nw_poisson.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_POISSON in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_POISSON)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert sorted(k for k in build.KERNEL_BUDGETS if k.startswith('k_sp_')) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] <= 64 and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)      # eight waves per SIMD
        assert build.KERNEL_BUDGETS[k][0] % 8 == 0 and build.KERNEL_BUDGETS[k][0] - r['vgpr'] < 8, (k, r)            # the budget is the next multiple of 8
    assert res['k_sp_splat_lds']['lds'] == 4 * 512 * 8 and res['k_sp_splat_lds4']['lds'] == 4 * 4096 * 8 and res['k_sp_splat']['lds'] == 0 and res['k_sp_relax']['lds'] == 0


def test_the_unit_is_new_and_has_no_float_atomics():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    src = _read('ch_shrinkwrap_amd', 'csrc', 'nw_poisson.hip')
    code = re.sub(r'//.*', '', src)
    assert '"nw_poisson_core.h"' in src and '"nw_bq.h"' in src
    for fn in ('nwo_normal(', 'nwo_axis(', 'nwo_home(', 'nwo_system_node(', 'nwo_prolong_node(', 'nwo_update(', 'nwo_neighbour_sum(', 'nwo_residual(',
               'nwo_quantise(', 'nwo_level(', 'nwo_depth_used(', 'nwo_alpha(', 'nwo_pow2_above('):
        assert fn in code, fn
    for m in re.finditer(r'atomic(Add|Max|Or)\(([^,]+),', code):                      # every atomic is on an integer, and its result is dropped
        line = code[code.rfind('\n', 0, m.start()) + 1:m.start()]
        assert not re.search(r'(=|return|\()\s*$', line), line
    assert 'atomicCAS' not in code and 'atomicExch' not in code and 'double *at' not in code and 'float *at' not in code
    for obj in build.BUDGETED_OBJECTS:
        names = build.kernel_resources(obj)
        if obj == build.OBJ_POISSON:
            assert not [k for k in names if not k.startswith('k_sp_')]
        else:
            assert not [k for k in names if k.startswith('k_sp_')], obj
    for tree in ('include', 'ch_shrinkwrap_amd'):                                     # the prefix is this unit's alone
        for d, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith(('.h', '.hip', '.cpp', '.py')) and 'poisson' not in fn and fn != 'build.py':
                    assert not re.search(r'\bnwo_\w+\s*\(', open(os.path.join(d, fn), errors='replace').read()), fn


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check comes before the first use of the context."""
    from ch_shrinkwrap_amd import poisson as C
    L = C.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    BAD = C.NWO_ERR_BADARG
    xyz, nrm = np.ones((5, 3), np.float32), np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (5, 1))
    used, skipped = ctypes.c_int64(-7), ctypes.c_int64(-7)

    def s(x=p(xyz), m=p(nrm), n=5, dev=0, lengths=0):
        return L.nwo_set_samples(None, x, m, n, dev, lengths, ctypes.byref(used), ctypes.byref(skipped))
    assert s() == BAD and s(lengths=1) == BAD                                                     # all is well but the context
    assert s(x=None) == BAD and s(m=None) == BAD and s(n=0) == BAD and s(n=(1 << 25) + 1) == BAD and s(dev=2) == BAD and s(lengths=2) == BAD
    for bad in (np.nan, np.inf, -np.inf):
        q = xyz.copy()
        q[3, 1] = bad
        assert s(x=p(q)) == C.NWO_ERR_NONFINITE
        q = nrm.copy()
        q[2, 0] = bad
        assert s(m=p(q)) == C.NWO_ERR_NONFINITE
    q = nrm.copy()
    q[4, 1] = 1.5
    assert s(m=p(q), lengths=0) == BAD and s(m=p(q), lengths=1) == BAD                            # (the first for the context, the second for the length)
    assert used.value == -7 and skipped.value == -7

    lo, du, occ = np.zeros(3, np.float32), ctypes.c_int(-7), np.full(10, -7, np.int64)

    def plan(lo_=p(lo), h=1.0, depth=5, full=5, spn=1.5, out=ctypes.byref(du)):
        return L.nwo_plan(None, lo_, h, depth, full, spn, out, p(occ))
    assert plan() == BAD and plan(depth=2) == BAD and plan(depth=10) == BAD and plan(lo_=None) == BAD and plan(out=None) == BAD
    for h in (0.0, -1.0, np.nan, np.inf):
        assert plan(h=h) == BAD
    assert plan(full=-1) == BAD and plan(spn=-1.0) == BAD and plan(spn=np.nan) == BAD
    bad_lo = lo.copy()
    bad_lo[1] = np.nan
    assert plan(lo_=p(bad_lo)) == C.NWO_ERR_NONFINITE
    assert du.value == -7 and (occ == -7).all()

    alpha, res = ctypes.c_double(-7.0), np.full(C.NWO_RESIDUAL_WORDS, -7.0)
    for pw in (0.0, -4.0, np.nan, np.inf):
        assert L.nwo_solve(None, pw, 8, 64, ctypes.byref(alpha), p(res)) == BAD
    assert L.nwo_solve(None, 4.0, -1, 64, ctypes.byref(alpha), p(res)) == BAD and L.nwo_solve(None, 4.0, 8, -1, ctypes.byref(alpha), p(res)) == BAD
    assert L.nwo_solve(None, 4.0, 8, 64, ctypes.byref(alpha), p(res)) == BAD
    assert alpha.value == -7.0 and (res == -7.0).all()
    assert L.nwo_level_begin(None, 1, 1.0) == BAD and L.nwo_level_begin(None, 10, 1.0) == BAD and L.nwo_level_begin(None, 3, 0.0) == BAD
    assert L.nwo_relax(None, -1, None, None) == BAD and L.nwo_get_level(None, 5, p(res)) == BAD and L.nwo_get_level(None, 0, None) == BAD
    assert L.nwo_set_chi(None, None) == BAD and L.nwo_field(None, None, None, None) == BAD and L.nwo_get_field(None, None) == BAD
    assert not L.nwo_field_pointer(None)
    h = ctypes.c_void_p()
    assert L.nwo_create(-1, ctypes.byref(h)) == BAD and L.nwo_create(0, None) == BAD
    assert L.nwo_last_error(None) == b'null ctx'


def test_the_python_surface_checks_before_it_touches_a_gpu():
    import inspect
    from ch_shrinkwrap_amd import poisson as C
    sig = inspect.signature(C.screened_poisson).parameters
    assert list(sig)[:19] == ['points', 'normals', 'k', 'smoothiter', 'flipflag', 'viewpos', 'depth', 'fulldepth', 'scale', 'samplespernode', 'pointweight',
                              'iters', 'confidence', 'coarse_iters', 'orient', 'start', 'device', 'context', 'return_info']
    assert (sig['k'].default, sig['depth'].default, sig['fulldepth'].default, sig['scale'].default, sig['samplespernode'].default, sig['pointweight'].default,
            sig['iters'].default, sig['coarse_iters'].default) == (10, 8, 5, 1.1, 1.5, 4, 8, 64)
    for name in C.IGNORED:
        assert name in sig and name in C.screened_poisson.__doc__
    assert 'ignored' in C.screened_poisson.__doc__ and 'right about inside and outside' in C.orient_normals.__doc__
    P = np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32)
    with pytest.raises(NotImplementedError):
        C.screened_poisson(P, P, smoothiter=1)
    for kw in (dict(depth=2), dict(depth=10), dict(pointweight=0), dict(pointweight=-1.0), dict(iters=-1)):
        with pytest.raises(ValueError):
            C.screened_poisson(P, P, **kw)
    with pytest.raises(ValueError):
        C.screened_poisson(np.ones((9, 3), np.float32), P[:9])                    # no extent
    with pytest.raises(ValueError):
        C.cube_for(np.array([[0.0, np.nan, 0.0]]), 5)
    lo, h = C.cube_for(np.array([[0.0, 0.0, 0.0], [10.0, 4.0, 2.0]], np.float32), 3, 1.1)
    assert lo.dtype == np.float32 and np.allclose(lo, [-0.5, -3.5, -4.5]) and h == np.float32(11.0 / 8)
    import screened_poisson_ref as R
    for depth in (3, 7):
        a, b = C.cube_for(P, depth), R.cube_for(P, depth)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_the_recipe_module_has_upstreams_traits():
    from ch_shrinkwrap_amd import poisson as C
    m = C.ScreenedPoissonMesh()
    assert (m.input, m.output, m.device) == ('filtered_localizations', 'membrane', 0)
    assert len(UPSTREAM_TRAITS) == 16
    for name, default in UPSTREAM_TRAITS:
        assert getattr(m, name) == default and type(getattr(m, name)) is type(default) or (name == 'pointweight' and m.pointweight == 4.0), name
    assert sorted(vars(m)) == sorted([n for n, _ in UPSTREAM_TRAITS] + ['input', 'output', 'device'])
    assert C.ScreenedPoissonMesh(depth=6, use_normals=True).depth == 6
    with pytest.raises(AttributeError):
        C.ScreenedPoissonMesh(depht=6)


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import poisson as C
    rng = np.random.default_rng(0)
    N = rng.normal(size=(60, 3)).astype(np.float32)
    P = (10 * N).astype(np.float32)
    table = {'x': P[:, 0], 'y': P[:, 1], 'z': P[:, 2], 'xn': N[:, 0], 'yn': N[:, 1], 'zn': N[:, 2]}
    with pytest.raises(RuntimeError):
        C.PoissonContext()
    with pytest.raises(RuntimeError):
        C.screened_poisson(P, N, depth=4)
    with pytest.raises(RuntimeError):
        C.screened_poisson(P, depth=4)
    with pytest.raises(RuntimeError):
        C.orient_normals(P, N, type('M', (), dict(vertices=P[:4], faces=np.array([[0, 1, 2], [0, 2, 3]], np.int32)))())
    with pytest.raises(RuntimeError):
        C.ScreenedPoissonMesh(use_normals=True, depth=4).execute({'filtered_localizations': table})
    assert not [n for n in dir(C) if 'pymeshlab' in n.lower() or 'scipy' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]
    src = open(C.__file__).read()
    assert 'import pymeshlab' not in src and 'scipy' not in src and 'linalg' not in src
