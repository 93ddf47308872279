"""CPU tests of the SMLM cloud simulator (include/nw_simulation.h, ch_shrinkwrap_amd/simulation.py): the NumPy restatement
(tests/simulation_ref.py) against Random123's known answers, the reference's shapes and the reference's loc_error; the shape compiler; the
exports, budgets and argument checks of the cross-compiled library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simulation_ref as R                                        # noqa: E402
from ch_shrinkwrap_amd import simulation as S                     # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
KERNELS = ['k_sim_eval', 'k_sim_normals', 'k_sim_cell_test', 'k_sim_cell_split', 'k_sim_leaf_test', 'k_sim_leaf_emit', 'k_sim_project',
           'k_sim_loc_error', 'k_sim_displace', 'k_sim_background', 'k_sim_copy_hist', 'k_sim_copy_equal', 'k_sim_copy_keep', 'k_sim_copy_emit']

# the shapes of tests/golden/sdf_shapes.npz (make_golden.py: golden_sdf_shapes) and simulation_case.npz (make_golden_simulation.py)
SDF_SHAPES = {
    'sphere_r100': ('Sphere', dict(radius=100.0)),
    'capsule_c2': ('Capsule', dict(start=[0, -500, 0], end=[0, 500, 0], radius=50.0)),
    'two_lobe_c3': ('UnionShape', dict(s0=('Sphere', dict(radius=300, centroid=[-250.0, 0, 0])), s1=('Sphere', dict(radius=300, centroid=[250.0, 0, 0])), k=50)),
    'round_box': ('Box', dict(halfwidth=[66, 83, 25.0], r=25.0)),
    'sheet': ('Sheet', dict(halfwidth=[226, 200, 100 / 3], r=100 / 3)),
    'three_way_junction': ('ThreeWayJunction', dict(h=300, r=50, k=20)),
    'er_sim2': ('ERSim2', {}),
    'difference': ('DifferenceShape', dict(s0=('Capsule', dict(start=[-40, 0, -100], end=[-40, 0, 100], radius=50.0)), s1=('Sphere', dict(radius=200.0)), k=25)),
}
CASE_SHAPES = {
    'torus': ('Torus', dict(radius=100.0, r=30.0, centroid=[10.0, -20.0, 5.0])),
    'two_toruses': ('TwoToruses', dict(r=30, R=100)),
    'n_toruses': ('NToruses', dict(toruses={'one': {'r': 30.0, 'R': 100.0}, 'two': {'r': 10.0, 'R': 75.0}, 'three': {'r': 30.0, 'R': 150.0}})),
    'dual_capsule': ('DualCapsule', dict(length=400.0, r=40.0, sep=150.0)),
    'intersection': ('IntersectionShape', dict(s0=('Sphere', dict(radius=150.0)), s1=('Box', dict(halfwidth=[100.0, 120.0, 80.0], r=10.0)), k=15.0)),
}
SIGMA_KW = dict(psf_width=(280, 280, 840), mean_photon_count=600, bg_photon_count=20)


def dkw_bound(n, alpha=1e-6):
    """two-sample Dvoretzky-Kiefer-Wolfowitz: each empirical CDF is within sqrt(ln(2 / alpha) / (2 n)) of the truth with probability 1 - alpha"""
    return 2.0 * np.sqrt(np.log(2.0 / alpha) / (2.0 * n))


def cdf_gap(sample, quantiles):
    """the largest |F_sample(q_k) - k / 1000| over the golden quantiles q_k, k = 1..999"""
    s = np.sort(sample)
    return float(np.abs(np.searchsorted(s, quantiles, side='right') / float(s.size) - np.arange(1, 1000) / 1000.0).max())


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10.  Both vectors quoted in the issue agree with the restatement written from the published
    round function; nothing had to be decided between a quoted vector and the definition."""
    w = R.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(x[0]) for x in w] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    w = R.philox4x32_10(f, f, f, f, f, f)
    assert [int(x[0]) for x in w] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_uniform_and_normal_maps():
    u = R.uniform(np.arange(200000), 3, 1, 99)
    assert u.min() > 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12.0 / u.size)
    z = R.normal(np.arange(200000), 4, 2, 99)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / z.size)
    # item, stream, draw and seed all reach the counter or the key
    base = R.key64(np.arange(4), 1, 7)
    assert len(set(base.tolist())) == 4
    assert (R.key64(np.arange(4), 2, 7) != base).all() and (R.key64(np.arange(4), 1, 8) != base).all()
    assert (R.key64(np.arange(4) + (1 << 32), 1, 7) != base).all() and (R.key64(np.arange(4), 1, 7 + (1 << 32)) != base).all()


@pytest.mark.parametrize('name', sorted(SDF_SHAPES))
def test_programs_match_the_reference_shapes(name):
    g = np.load(os.path.join(GOLDEN, 'sdf_shapes.npz'))
    prog = S.compile_shape(*SDF_SHAPES[name])
    assert np.abs(R.eval_program(prog.ops, g['points']) - g[name]).max() <= 1e-9


@pytest.mark.parametrize('name', sorted(CASE_SHAPES))
def test_programs_match_the_reference_shapes_and_normals(name):
    g = np.load(os.path.join(GOLDEN, 'simulation_case.npz'))
    prog = S.compile_shape(*CASE_SHAPES[name])
    assert np.abs(R.eval_program(prog.ops, g['points']) - g['sdf_' + name]).max() <= 1e-9
    assert np.abs(R.normals(prog.ops, g['points']) - g['normals_' + name]).max() <= 1e-6
    # the enclosing cube encloses: no point outside it is inside the shape
    outside = (np.abs(g['points'] - prog.centre[None, :]) > prog.r_max).any(1)
    assert (g['sdf_' + name][outside] > 0).all()


def test_sigma_distribution_against_the_reference():
    g = np.load(os.path.join(GOLDEN, 'simulation_case.npz'))
    n = int(g['sigma_n'])
    assert n == 200000
    sigma, photons = R.loc_error(n, 1, S.STREAM_PHOTONS, **SIGMA_KW)
    assert photons.min() >= 20.0
    for a in range(3):
        gap = cdf_gap(sigma[:, a], g['sigma_quantiles'][:, a])
        assert gap < dkw_bound(n), (a, gap)


def test_compiler_refuses_what_it_cannot_compile():
    for name in S.NOT_COMPILED:
        with pytest.raises(NotImplementedError, match=name):
            S.compile_shape(name, {})
    with pytest.raises(ValueError):
        S.compile_shape('Dodecahedron', {})
    deep = S.Sphere(radius=1.0)
    for _ in range(S.STACK_DEPTH):
        deep = S.UnionShape(S.Sphere(radius=1.0), deep)                      # right-nested: every operand waits on the stack
    with pytest.raises(ValueError, match='stack'):
        S.compile_shape(deep)
    assert S.parse_shape_params("{'r': 30, 'R': 100}") == {'r': 30, 'R': 100}
    assert S.compile_shape('ERSim2').ops.dtype.itemsize == 104                 # sizeof(nwg_op)


def test_lattice_does_not_depend_on_the_traversal():
    """brute force over every node of the cube = the refinement from any starting level; another cube decides every shared node alike"""
    prog = S.compile_shape('DualCapsule', dict(length=60.0, r=12.0, sep=40.0))
    centre, dx = prog.centre + np.array([0.21, 0.13, 0.37]), 2.0
    want = R.lattice(prog.ops, centre, prog.r_max + dx, dx, 0.3, 5, brute_force=True)
    assert want['margin'] > 1e-9 and want['keys'].size > 100
    assert (np.diff(want['keys'].astype(np.int64)) > 0).all()
    for level in (-1, 0, 1, 3, 6):
        got = R.lattice(prog.ops, centre, prog.r_max + dx, dx, 0.3, 5, start_level=level)
        assert np.array_equal(got['keys'], want['keys']) and np.array_equal(got['points'], want['points'])
    wide = R.lattice(prog.ops, centre, prog.r_max + 17 * dx, dx, 0.3, 5)
    assert np.array_equal(wide['keys'], want['keys'])
    assert np.abs(R.eval_program(prog.ops, want['points'])).max() < 1e-6       # two Newton steps reach the surface


def test_copy_selection_is_uniform_without_replacement():
    n = 5000
    copy = R.select_copies(n, n, 11, S.STREAM_COPY_KEY)
    assert copy.size == n and (np.diff(copy) > 0).all() and copy.max() < S.COPIES * n
    mult = np.bincount(copy % n, minlength=n)
    assert mult.max() <= S.COPIES and mult.mean() == 1.0


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_simulation.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwg_[a-z0-9_]+)\s*\(', txt)))


def test_library_exports_the_simulation_header():
    from ch_shrinkwrap_amd import build, _lib
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) == 13
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(S.SYMBOLS) == names
    assert S.load().nwg_abi_version() == S.ABI_VERSION == 1


def test_simulation_kernels_are_budgeted_and_use_no_scratch():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    assert build.OBJ_SIMULATION in build.BUDGETED_OBJECTS
    assert any(u[1] == build.OBJ_SIMULATION and '-ffp-contract=off' in u[3] for u in build.UNITS)
    in_object = build.kernel_resources(build.OBJ_SIMULATION)
    assert sorted(in_object) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] and r['lds'] <= build.KERNEL_BUDGETS[k][1], (k, r)


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every argument check comes before the first use of the context."""
    L = S.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ops = S.compile_shape('TwoToruses', dict(r=30, R=100)).ops
    bad = ops.copy()
    bad['code'][0] = 77
    assert L.nwg_set_program(None, p(bad), bad.shape[0]) == S.NWG_ERR_BADARG
    assert L.nwg_set_program(None, p(ops[:-1].copy()), ops.shape[0] - 1) == S.NWG_ERR_BADARG          # two values left
    assert L.nwg_set_program(None, p(ops[-1:].copy()), 1) == S.NWG_ERR_BADARG                          # a combinator on an empty stack
    assert L.nwg_set_program(None, p(ops), 0) == S.NWG_ERR_BADARG
    assert L.nwg_set_program(None, p(ops), ops.shape[0]) == S.NWG_ERR_BADARG                           # a good program, no context
    xyz, out = np.zeros((4, 3)), np.zeros((4, 3))
    assert L.nwg_eval(None, p(xyz), 4, p(out)) == S.NWG_ERR_BADARG
    assert L.nwg_eval(None, p(xyz), 0, p(out)) == S.NWG_ERR_BADARG
    assert L.nwg_normals(None, None, 4, p(out)) == S.NWG_ERR_BADARG
    n = ctypes.c_int64()
    c = np.zeros(3)
    for r_max, dx, prob, lip, lvl, proj, cap in ((0.0, 1.0, 0.5, 1.5, -1, 2, 10), (10.0, 0.0, 0.5, 1.5, -1, 2, 10), (10.0, 1.0, -0.1, 1.5, -1, 2, 10),
                                                  (10.0, 1.0, 0.5, 0.5, -1, 2, 10), (10.0, 1.0, 0.5, 1.5, 21, 2, 10), (10.0, 1.0, 0.5, 1.5, -1, -1, 10),
                                                  (10.0, 1.0, 0.5, 1.5, -1, 2, 0), (1e9, 1.0, 0.5, 1.5, -1, 2, 10), (float('nan'), 1.0, 0.5, 1.5, -1, 2, 10)):
        assert L.nwg_sample_surface(None, p(c), r_max, dx, prob, 0, lip, lvl, proj, cap, ctypes.byref(n)) == S.NWG_ERR_BADARG
    assert L.nwg_sample_surface(None, p(c), 10.0, 1.0, 0.5, 0, 1.5, -1, 2, 10, None) == S.NWG_ERR_BADARG
    assert L.nwg_get_points(None, None, None) == S.NWG_ERR_BADARG
    psf = np.array([280.0, 280.0, 840.0])
    assert L.nwg_loc_error(None, 4, 0, 1, S.MODEL_EXPONENTIAL, p(psf), 600.0, 20.0, p(out), None) == S.NWG_ERR_BADARG
    assert L.nwg_loc_error(None, 4, 0, 1, S.MODEL_EXPONENTIAL, None, 600.0, 20.0, p(out), None) == S.NWG_ERR_BADARG
    assert L.nwg_loc_error(None, 4, 0, 1, 5, p(psf), 600.0, 20.0, p(out), None) == S.NWG_ERR_BADARG
    assert L.nwg_displace(None, p(xyz), p(xyz), 4, 0, 2, None) == S.NWG_ERR_BADARG
    assert L.nwg_smlmify(None, p(xyz), p(xyz), 4, 41, 0, 3, 4, 5, S.MODEL_EXPONENTIAL, p(psf), 600.0, 20.0, p(out), p(out), None) == S.NWG_ERR_BADARG
    assert L.nwg_smlmify(None, p(xyz), p(xyz), 4, 4, 0, 3, 4, 5, S.MODEL_EXPONENTIAL, p(psf), 600.0, 20.0, p(out), p(out), None) == S.NWG_ERR_BADARG
    assert L.nwg_background(None, p(c), p(c), 0, 0, 6, p(out)) == S.NWG_ERR_BADARG
    h = ctypes.c_void_p()
    assert L.nwg_create(-1, ctypes.byref(h)) == S.NWG_ERR_BADARG and L.nwg_create(0, None) == S.NWG_ERR_BADARG


def test_the_simulator_never_falls_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(RuntimeError):
        S.generate_smlm_pointcloud_from_shape('TwoToruses', dict(r=30, R=100), p=0.01)
    with pytest.raises(RuntimeError):
        S.PointcloudFromShape().execute({})
    assert (S.loc_error((5, 3), model=None) == 10.0).all()                     # upstream's other branch needs no device
