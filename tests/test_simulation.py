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
    for good in (R.chain('union', 0.0, S.STACK_DEPTH).ops, R.long_program()[0].ops):                     # the deepest and the longest: the same
        assert R.stack_depth(good) == S.STACK_DEPTH or good.shape[0] == S.MAX_OPS
        assert L.nwg_set_program(None, p(good), good.shape[0]) == S.NWG_ERR_BADARG
    nine = np.zeros(2 * S.STACK_DEPTH + 1, S.OP_DTYPE)                                                   # nine spheres, then eight unions
    nine['code'][:S.STACK_DEPTH + 1], nine['code'][S.STACK_DEPTH + 1:] = S.OP_SPHERE, S.OP_UNION
    nine['a'][:S.STACK_DEPTH + 1, 0] = 1.0
    assert R.stack_depth(nine) == S.STACK_DEPTH + 1 and L.nwg_set_program(None, p(nine), nine.shape[0]) == S.NWG_ERR_BADARG
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
    widest = R.lattice_case('widest')['r_max']
    for r_max, proj in ((widest, 64), (widest + 1.0, 2), (10.0, 65)):                                    # (the first: a good call, no context)
        assert L.nwg_sample_surface(None, p(c), r_max, 1.0, 0.5, 0, 1.5, -1, proj, 10, ctypes.byref(n)) == S.NWG_ERR_BADARG
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


def test_a_capsule_without_length_is_refused():
    """sdf.capsule divides by |b - a|^2: upstream's value for a == b is NaN at every point (so is the restatement's), where the device's
    fmax(NaN, 0) would give a sphere's distance.  Neither is computed: the constructor and nwg_set_program refuse the shape."""
    ops = np.zeros(1, S.OP_DTYPE)
    ops['code'][0] = S.OP_CAPSULE
    ops['a'][0, :7] = [1.0, 2.0, 3.0, 1.0, 2.0, 3.0, 1.0]
    with np.errstate(all='ignore'):
        assert np.isnan(R.eval_program(ops, np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]))).all()
    for start, end in (([1.0, 2.0, 3.0], [1.0, 2.0, 3.0]), ([0.0, 0.0, 0.0], [0.0, 0.0, 1e-200])):        # (the second: |b - a|^2 underflows to 0)
        with pytest.raises(ValueError, match='coincide'):
            S.Capsule(start, end, 1.0)
        with pytest.raises(ValueError, match='coincide'):
            S.compile_shape('Capsule', dict(start=start, end=end, radius=1.0))
    assert S.compile_shape('Capsule', dict(start=[0.0, 0.0, 0.0], end=[0.0, 0.0, 1e-150], radius=1.0)).ops.shape == (1,)
    # the library's own check, before the context is used: a status, and with a context (tests/test_hip_simulation_edges.py) a text
    L = S.load()
    assert L.nwg_set_program(None, ops.ctypes.data_as(ctypes.c_void_p), 1) == S.NWG_ERR_BADARG
    header = open(os.path.join(ROOT, 'include', 'nw_simulation.h')).read()
    assert "a capsule's two ends apart" in header


# ---- the premises of tests/test_hip_simulation_edges.py, on the restatement alone ------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(R.COMBINATORS))
def test_chain_builders_use_every_stack_slot(kind):
    for k in (0.0, 0.5):
        for n in range(2, S.STACK_DEPTH + 1):
            prog = R.chain(kind, k, n)
            pts = R.chain_points(prog.ops)
            assert R.stack_depth(prog.ops) == n and (prog.ops['code'] == S.OP_SPHERE).sum() == n
            assert R.deciding_operands(prog.ops, pts).any(1).all(), (kind, k, n)
            if k == 0:                                                     # every operand is the chain's value somewhere
                won = np.bincount(R.chain_winner(kind, prog.ops, pts), minlength=n)
                assert won.min() > 0, (kind, n, won)
                v = R.operand_values(prog.ops, pts)
                v[:-1] = -v[:-1] if kind == 'difference' else v[:-1]
                assert np.array_equal(R.eval_program(prog.ops, pts), v.min(0) if kind == 'union' else v.max(0))
        assert len(prog.ops) == 22                                         # 7 frames (the first sphere needs none), 8 spheres, 7 combinators


def test_mixed_and_long_builders():
    prog = R.mixed_chain()
    pts = R.chain_points(prog.ops)
    assert R.stack_depth(prog.ops) == S.STACK_DEPTH and sorted(set(prog.ops['code'].tolist())) == list(range(9))
    assert R.deciding_operands(prog.ops, pts).any(1).all() and np.isfinite(R.eval_program(prog.ops, pts)).all()
    frames = prog.ops['a'][prog.ops['code'] == S.OP_FRAME][:, :9]
    assert (np.abs(frames - np.eye(3).ravel()) > 0.1).any()               # one operand under a rotation
    assert pts.shape[0] > max(R.COUNTS)
    prog, pts = R.long_program()
    assert prog.ops.shape[0] == S.MAX_OPS == 256 and R.stack_depth(prog.ops) == 2 and (prog.ops['code'] == S.OP_FRAME).sum() == 1
    assert R.deciding_operands(prog.ops, pts, which=(0, 1, 126, 127)).any(1).all()          # the first and the last ops matter
    with pytest.raises(ValueError, match='more than 256'):
        S.compile_shape(S.UnionShape(S.Sphere(radius=1.0, centroid=[1.0, 0.0, 0.0]), _node_of_255_ops()))


def _node_of_255_ops():
    """128 capsules and 127 unions at a stack of 2"""
    node = S.Capsule([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 1.0)
    for i in range(127):
        node = S.UnionShape(node, S.Capsule([0.0, 0.0, 0.0], [1.0, 0.0, float(i)], 1.0))
    return node


def test_primitive_and_tie_builders():
    for name, (shape, pts) in R.primitive_edge_cases().items():
        prog = S.compile_shape(shape)
        with np.errstate(all='ignore'):
            d, nrm = R.eval_program(prog.ops, pts), R.normals(prog.ops, pts)
        assert np.isfinite(d).all() and (d == 0).any() and np.isnan(nrm).any(), name
        assert np.isfinite(nrm).all(1).sum() > pts.shape[0] // 2, name
    # what the points are named for
    cases = R.primitive_edge_cases()
    cap, pts = cases['capsule']
    a, b = np.array(cap.args[0:3]), np.array(cap.args[3:6])
    h = ((pts - a) @ (b - a)) / ((b - a) @ (b - a))
    assert (h < 0).any() and (h == 0).any() and (h == 1).any() and (h > 1).any() and ((h > 0) & (h < 1)).any()
    tor, pts = cases['torus']
    q = pts - tor.centroid
    ring = np.sqrt(q[:, 0] ** 2 + q[:, 2] ** 2)
    assert ((ring == 0) & (q[:, 1] == 0)).any() and ((ring == 0) & (q[:, 1] != 0)).any() and ((ring == 100.0) & (q[:, 1] == 0)).sum() >= 4
    box, pts = cases['box']
    on = (np.abs(pts - box.centroid) == np.array(box.args[:3])).sum(1)
    assert (on == 1).sum() >= 6 and (on == 2).sum() >= 12 and (on == 3).sum() >= 8
    for kind in R.COMBINATORS:
        prog, pts, d0, d1 = R.tie_case(kind, 0.0)
        assert ((-d0 if kind == 'difference' else d0) == d1).all() and pts.shape[0] >= 5
        prog, pts, d0, d1 = R.tie_case(kind, 1.5)
        gap = np.abs((-d0 if kind == 'difference' else d0) - d1) - 1.5
        assert (gap == 0).sum() == 2 and (gap > 0).sum() == 2 and (gap < 0).sum() == 2 and np.abs(gap).max() < 1e-10
        h = np.maximum(1.5 - np.abs((-d0 if kind == 'difference' else d0) - d1), 0.0)
        assert (h > 0).sum() == 2                                          # the smooth term is live on one side only


def test_lattice_edge_cases_on_the_restatement():
    """the table of the edge tests: counts, margins and what decides each case, from every start level"""
    for name, count in (('shell_edge', 1352), ('cube_cut', 815), ('flat_spot', 289), ('widest', 5753), ('one_node', 1), ('outside', 0)):
        case = R.lattice_case(name)
        runs = [R.run_lattice_case(case, level)[1] for level in case['levels']]
        for w in runs:
            assert w['keys'].size == count and np.array_equal(w['keys'], runs[0]['keys']) and np.array_equal(w['points'], runs[0]['points']), name
            assert (np.diff(w['keys'].astype(np.int64)) > 0).all()
    prog, w = R.run_lattice_case(R.lattice_case('shell_edge'), -1)
    d = R.eval_program(prog.ops, w['lattice'])
    assert w['margin'] == 0.0 and d.min() == -0.5 and d.max() == -0.5 and np.abs(w['lattice']).max() == 7.5
    outer = np.array([[8.5, 0.5, 0.5], [0.5, -8.5, 0.5], [0.5, 0.5, 8.5]])
    assert (R.eval_program(prog.ops, outer) == 0.5).all()                  # the next layer sits on d == +dx/2 exactly, and is left out
    case = R.lattice_case('cube_cut')
    prog, w = R.run_lattice_case(case, -1)
    _, wide = R.run_lattice_case(case, -1, r_max=40.0)
    inside = (np.abs(wide['nodes'] - R.BIAS) <= 20).all(1)
    assert wide['keys'].size > 815 and np.array_equal(wide['keys'][inside], w['keys']) and np.array_equal(wide['points'][inside], w['points'])
    assert (np.abs(w['nodes'] - R.BIAS) == 20).any(1).sum() == 470 and w['margin'] > 1e-9
    assert w['n_fluorophores'] == 815 and R.run_lattice_case(case, -1, p=0.0)[1]['keys'].size == 0 and R.run_lattice_case(case, -1, p=1.5)[1]['keys'].size == 815
    prog, w = R.run_lattice_case(R.lattice_case('flat_spot'), -1)
    g = R.gradient(prog.ops, w['lattice'])
    flat = (g == 0).all(1)
    assert flat.sum() == 225 and (R.eval_program(prog.ops, w['lattice'][flat]) == -0.25).all()
    assert np.isfinite(w['points']).all() and np.array_equal(w['points'], w['lattice'])
    prog, w = R.run_lattice_case(R.lattice_case('widest'), -1)
    assert w['nodes'].min() == 11 and w['nodes'].max() == 2097141 and 1e-9 < w['margin'] < 1e-3 and int(w['keys'].max()) >> 62 == 1
    assert np.abs(R.eval_program(prog.ops, w['points'])).max() < 1e-6
    prog, w = R.run_lattice_case(R.lattice_case('one_node'), -1)
    assert np.array_equal(w['nodes'], [[R.BIAS] * 3]) and np.array_equal(w['points'], np.zeros((1, 3)))
    case = R.lattice_case('outside')
    assert [np.isfinite(R.run_lattice_case(case, level)[1]['margin']) for level in case['levels']] == [False, True, False]      # culled as cells, and as nodes


def test_every_seed_gives_its_own_draws():
    assert R.SEEDS[0] < 1 << 32 and R.SEEDS[1] & 0xFFFFFFFF == R.SEEDS[0] and R.SEEDS[2] == 2 ** 64 - 1
    case = R.lattice_case('cube_cut')
    rng = np.random.default_rng(2)
    xyz, sigma = rng.uniform(-500, 500, (300, 3)), rng.uniform(2, 20, (300, 3))
    seen = []
    for seed in R.SEEDS:
        keys = R.run_lattice_case(case, -1, p=0.5, seed=seed)[1]['keys']
        assert 300 < keys.size < 515
        seen.append((keys, R.loc_error(300, seed, S.STREAM_PHOTONS, **SIGMA_KW)[0], R.displace(xyz, sigma, seed, S.STREAM_DISPLACE),
                     R.background([-1.0, 2.0, 3.0], [5.0, 7.0, 11.0], 300, seed, S.STREAM_BG_POSITION))
                    + R.smlmify(xyz, sigma, seed, (S.STREAM_COPY_DISPLACE, S.STREAM_COPY_KEY, S.STREAM_COPY_PHOTONS), **SIGMA_KW))
    for a in range(3):
        for b in range(a + 1, 3):
            for x, y in zip(seen[a], seen[b]):
                assert x.shape != y.shape or not np.array_equal(x, y)


def test_the_simulator_never_falls_back():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(RuntimeError):
        S.generate_smlm_pointcloud_from_shape('TwoToruses', dict(r=30, R=100), p=0.01)
    with pytest.raises(RuntimeError):
        S.PointcloudFromShape().execute({})
    assert (S.loc_error((5, 3), model=None) == 10.0).all()                     # upstream's other branch needs no device
