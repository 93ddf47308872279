"""The screened Poisson grid solver on the device (csrc/nw_poisson.hip) against the NumPy restatement (tests/screened_poisson_ref.py), phase
by phase and for equality: every integer of W, V, the occupancy and thr, every bit of rhs, diag, chi after each level, the residuals and
F -- on sample counts around the wave and the workgroups, from host arrays and device pointers, with 5 000 samples in one cell, on node
centres, cell boundaries, weight ties and the outermost half cells, with axis, zero, tiny and huge normals and with lengths as weights, at
the smallest depth, without sweeps, at the samplespernode threshold, 10^6 from the origin, with a crafted solution whose largest value is
a power of two, all through one context whose depth grows and shrinks; then the surface of a torus at depth 7 against the isosurface
restatement, orient_normals, and the recipe module on a simulated cloud."""
import functools

import numpy as np
import pytest

import isosurface_ref as I
import screened_poisson_ref as R
from ch_shrinkwrap_amd import poisson as C

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1025, 4097]
LO, H4 = np.full(3, -110.0, np.float32), np.float32(220.0 / 16)                # the cube of the size cases at depth 4


@pytest.fixture(scope='module')
def ctx():
    c = C.PoissonContext()
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def sized_cloud(n):
    P, N = R.sphere_cloud(n, 100.0, 3.0, seed=n)
    return P, N


def to_device(*arrays):
    import torch
    keep = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to('cuda') for a in arrays]
    torch.cuda.synchronize()
    return keep, [(t.data_ptr(), len(a)) for t, a in zip(keep, arrays)]


def check(ctx, P, N, lo, h, depth, on_device=False, ref=None, fulldepth=5, samples_per_node=1.5, pointweight=4.0, iters=8, coarse_iters=64,
          use_lengths=False):
    """the phases one by one, then the driver: the restatement's integers and bits both times"""
    kw = dict(fulldepth=fulldepth, samples_per_node=samples_per_node, pointweight=pointweight, iters=iters, coarse_iters=coarse_iters, use_lengths=use_lengths)
    if ref is None:
        ref = R.solve(P, N, lo, h, depth, **kw)
    keep = None
    if on_device:
        keep, (dp, dn) = to_device(P, N)
        assert ctx.set_samples(dp, dn, use_lengths) == (ref['n_used'], ref['n_skipped'])
    else:
        assert ctx.set_samples(P, N, use_lengths) == (ref['n_used'], ref['n_skipped'])
    used, occ = ctx.plan(lo, h, depth, fulldepth, samples_per_node)
    assert used == ref['depth_used'] and occ == ref['occ'] and ctx.h_used == ref['h_used']
    alpha = ctx.alpha(pointweight)
    assert alpha == ref['alpha']
    for l in range(2, used + 1):
        L = ref['levels'][l]
        ctx.level_begin(l, alpha)
        assert np.array_equal(ctx.get_level('W'), L['W']) and np.array_equal(ctx.get_level('V'), L['V'])
        assert np.array_equal(bits(ctx.get_level('rhs')), bits(L['rhs'])) and np.array_equal(bits(ctx.get_level('diag')), bits(L['diag']))
        res = ctx.relax(coarse_iters if l == 2 else iters)
        assert np.array_equal(bits(ctx.get_level('chi')), bits(L['chi'])), l
        assert bits(np.array(res)).tolist() == bits(np.array(ref['residuals'][l])).tolist()
    assert ctx.field_pointer() == 0
    fld = ctx.field(return_field=True)
    assert fld['thr'] == ref['thr'] and fld['E'] == ref['E'] and fld['sumW'] == ref['sumW'] == ref['n_used'] << 21 and np.array_equal(fld['F'], ref['F'])
    assert ctx.field_pointer() != 0
    a2, res2 = ctx.solve(pointweight, iters, coarse_iters)
    assert a2 == alpha and res2 == ref['residuals'] and ctx.field_pointer() == 0
    assert np.array_equal(bits(ctx.get_level('chi')), bits(ref['chi']))
    fld = ctx.field(return_field=True)
    assert fld['thr'] == ref['thr'] and np.array_equal(fld['F'], ref['F'])
    del keep
    return ref


@pytest.mark.parametrize('n', SIZES)
def test_sample_counts_from_host_arrays_and_device_pointers(ctx, n):
    P, N = sized_cloud(n)
    ref = check(ctx, P, N, LO, H4, 4, fulldepth=4)
    check(ctx, P, N, LO, H4, 4, fulldepth=4, on_device=True, ref=ref)
    assert ref['depth_used'] == 4


def test_more_samples_than_one_pass_of_the_aggregating_splat(ctx):
    """levels 2 to 4 are summed in LDS by at most 64 workgroups of 256 lanes: beyond 16 384 samples a lane takes more than one"""
    P, N = R.sphere_cloud(40001, 100.0, 3.0, seed=9)
    N[::7] = 0.0
    ref = check(ctx, P, N, LO, H4, 4, fulldepth=4)
    check(ctx, P, N, LO, H4, 4, fulldepth=4, on_device=True, ref=ref)


def test_five_thousand_samples_in_one_cell(ctx):
    rng = np.random.default_rng(7)
    lo, h = np.zeros(3, np.float32), np.float32(1.0)
    P = (np.array([13.0, 20.0, 7.0]) + rng.uniform(0.0, 1.0, (5000, 3))).astype(np.float32)           # one cell of the 32^3 level
    N = rng.normal(size=(5000, 3)).astype(np.float32)
    N[:2500] = [0.0, 0.0, 1.0]                                                                         # half of them agree: the sums are large
    ref = check(ctx, P, N, lo, h, 5, fulldepth=5)
    assert ref['occ'] == {2: 1, 3: 1, 4: 1, 5: 1} and int(np.abs(ref['levels'][2]['V']).max()) > 1000 << 33 and int(ref['levels'][5]['W'].max()) > 2000 << 21
    check(ctx, P, N, lo, h, 5, fulldepth=5, on_device=True, ref=ref)


def test_splat_positions(ctx):
    """node centres, cell boundaries and one float32 step either side, the ties of the weight, the outermost half cells of all six faces, a
    corner, and samples outside the cube"""
    rng = np.random.default_rng(11)
    lo, h, depth = np.array([-8.0, 3.0, 100.0], np.float32), np.float32(0.75), 4
    rows = []
    for d in range(3):
        for x in R.special_positions(lo[d], float(h), 16):
            p = (lo + rng.uniform(1.0, 15.0, 3) * float(h)).astype(np.float32)
            p[d] = x
            rows.append(p)
    for corner in range(8):
        rows.append(np.array([lo[d] + (0.2 if (corner >> d) & 1 == 0 else 15.8) * float(h) for d in range(3)], np.float32))
    P = np.array(rows, np.float32)
    N = rng.normal(size=P.shape).astype(np.float32)
    for d in range(3):                                                # the weights the positions are meant to reach, per axis
        ia, ib, wa, wb = R.axis_weights(P[:, d], lo[d], float(h), 16)
        assert (wb == 64).any() and (wb == 0).any() and (ia == ib).any() and (ia == 0).any() and (ib == 15).any()
    ref = check(ctx, P, N, lo, h, depth, fulldepth=4)
    check(ctx, P, N, lo, h, depth, fulldepth=4, on_device=True, ref=ref)
    centres = (lo + (rng.integers(0, 16, (40, 3)) + 0.5) * float(h)).astype(np.float32)              # exactly on node centres: one node a sample
    ref = check(ctx, centres, N[:40], lo, h, depth, fulldepth=4)
    assert np.count_nonzero(ref['levels'][4]['W']) <= 40 and set(np.unique(ref['levels'][4]['W'])) <= {k << 21 for k in range(41)}


def test_normals(ctx):
    rng = np.random.default_rng(13)
    P, N = sized_cloud(257)
    N = N.copy()
    N[:6] = np.concatenate([np.eye(3), -np.eye(3)])
    N[6:10] = 0.0                                                     # skipped and counted
    N[10:20] *= np.float32(1e-30)
    N[20:30] *= np.float32(1e30)
    ref = check(ctx, P, N, LO, H4, 4, fulldepth=4)
    assert ref['n_skipped'] == 4 and ref['n_used'] == 253
    check(ctx, P, N, LO, H4, 4, fulldepth=4, on_device=True, ref=ref)
    Q = (sized_cloud(257)[1] * np.float32(0.25)).astype(np.float32)   # lengths as weights
    Q[::9] = 0.0
    ref = check(ctx, P, Q, LO, H4, 4, fulldepth=4, use_lengths=True)
    assert int(np.abs(R.quantise_normals(Q, True)[0]).max()) <= 1024
    check(ctx, P, Q, LO, H4, 4, fulldepth=4, use_lengths=True, on_device=True, ref=ref)
    bad = Q.copy()
    bad[100, 1] = 1.5
    keep, on_dev = to_device(P, bad)
    for args in ((P, bad), on_dev):                                   # refused on the host, and by the kernel
        with pytest.raises(RuntimeError, match='above 1'):
            ctx.set_samples(args[0], args[1], use_lengths=True)
    bad = N.copy()
    bad[200, 2] = np.nan
    keep, (dp, dn) = to_device(P, bad)
    with pytest.raises(RuntimeError, match='not finite'):
        ctx.set_samples(dp, dn)
    with pytest.raises(RuntimeError):                                 # a failed call leaves no samples
        ctx.plan(LO, H4, 4)
    with pytest.raises(RuntimeError):
        ctx.set_samples(P, np.zeros_like(P))                          # nothing to use


def test_levels(ctx):
    P, N = sized_cloud(1025)
    lo3, h3 = R.cube_for(P, 3)
    ref = check(ctx, P, N, lo3, h3, 3, fulldepth=3)                   # the base and one level: 3-, 4-, 5- and 6-valent nodes within a wave
    assert ref['depth_used'] == 3 and set(np.unique(ref['levels'][3]['diag'] - (ref['alpha'] * (ref['levels'][3]['W'] / 2.0 ** 21)))) >= {3.0, 6.0}
    ref = check(ctx, P, N, LO, H4, 4, fulldepth=4, iters=0, coarse_iters=1)
    assert ref['residuals'][4][0] == ref['residuals'][4][1]
    check(ctx, P, N, lo3, h3, 3, fulldepth=0, samples_per_node=1e9)   # the rule stops at once: the base level alone
    far = (P.astype(np.float64) + 1.0e6).astype(np.float32)           # float32 steps of 1/16 out there
    lo, h = R.cube_for(far, 5)
    ref = check(ctx, far, N, lo, h, 5, fulldepth=5)
    check(ctx, far, N, lo, h, 5, fulldepth=5, on_device=True, ref=ref)


def test_samplespernode_at_the_threshold(ctx):
    P, N = sized_cloud(4097)
    lo, h = R.cube_for(P, 5)
    nq, used = R.quantise_normals(N)
    occ4 = R.occupancy(P, used, lo, h, 5, 4)
    at = float(len(P)) / float(occ4)
    seen = set()
    for spn in (at * (1.0 - 1e-12), at, at * (1.0 + 1e-12)):          # both sides of N < samplespernode * occ_4, and the quotient itself
        ref = R.solve(P, N, lo, h, 5, fulldepth=3, samples_per_node=float(spn), keep_levels=False)
        ctx.set_samples(P, N)
        got, occ = ctx.plan(lo, h, 5, 3, float(spn))
        assert got == ref['depth_used'] and occ == ref['occ']
        seen.add(got)
    assert len(seen) == 2 and 3 in seen                               # below the quotient level 4 is taken, above it the rule stops at 3


def test_the_field_at_a_power_of_two_and_a_single_node(ctx):
    P, N = sized_cloud(256)
    ref = check(ctx, P, N, LO, H4, 4, fulldepth=4)
    chi = ref['chi'].copy()
    chi[3, 4, 5], chi[9, 2, 11] = 2.0, -2.0                            # M = 2 exactly: chi / E = +-1, F reaches 2^32 and 0
    assert np.abs(ref['chi']).max() < 2.0
    ctx.set_chi(chi)
    fld = ctx.field(return_field=True)
    want = R.field(chi, ref['W'])
    assert want['E'] == 2.0 and int(want['F'].max()) == 1 << 32 and int(want['F'].min()) == 0
    assert fld['E'] == 2.0 and fld['thr'] == want['thr'] and np.array_equal(fld['F'], want['F'])
    ctx.set_chi(np.zeros_like(chi))
    with pytest.raises(RuntimeError, match='zero everywhere'):
        ctx.field()
    one = (LO + (np.array([[5, 9, 3]]) + 0.5) * float(H4)).astype(np.float32)                          # a single occupied node
    ref = check(ctx, one, np.array([[0.0, 0.6, 0.8]], np.float32), LO, H4, 4, fulldepth=4)
    assert np.count_nonzero(ref['W']) == 1 and ref['occ'] == {2: 1, 3: 1, 4: 1}


def test_one_context_grows_and_shrinks(ctx):
    P, N = sized_cloud(1025)
    for depth in (3, 5, 6, 4, 3, 6):
        lo, h = R.cube_for(P, depth)
        check(ctx, P, N, lo, h, depth, fulldepth=depth)
    with pytest.raises(RuntimeError):                                  # the level below first
        ctx.level_begin(4, 1.0)
    with pytest.raises(RuntimeError):
        ctx.plan(LO, H4, 2)
    with pytest.raises(RuntimeError):
        ctx.solve(0.0)


@functools.lru_cache(maxsize=None)
def torus():
    return R.torus_cloud(8000, 100.0, 30.0, 5.0, seed=2)


def test_the_torus_at_depth_7(ctx):
    """the table's torus: depth 7 asked (the occupancy is counted on 128^3), 5 used.  The device's mesh is the restatement's surface nets
    of its own field, and Euler 0 and manifold"""
    P, N = torus()
    ref = R.reconstruct(P, N, depth=7, fulldepth=4)
    v, f, info = C.screened_poisson(P, N, depth=7, fulldepth=4, context=ctx, return_info=True)
    assert info['depth_used'] == ref['depth_used'] == 5 and info['thr'] == ref['thr'] and info['occ'] == ref['occ'] and info['residuals'] == ref['residuals']
    assert info['h'] == float(ref['h_used']) and info['E'] == ref['E'] and info['alpha'] == ref['alpha'] and (info['n_used'], info['n_skipped']) == (8000, 0)
    ictx_keys = None
    from ch_shrinkwrap_amd import isosurface
    ic = isosurface.IsosurfaceContext()
    try:
        ctx.field()
        ic.set_field(ctx.field_pointer(), ref['lo'], ctx.h_used, (32, 32, 32))
        dv, df, ictx_keys = ic.extract(info['thr'], return_keys=True)
    finally:
        ic.close()
    I.compare_mesh('torus', dv, df, ictx_keys, ref['vertices'], ref['faces'], ref['keys'])
    assert np.array_equal(f, df) and np.array_equal(v, dv)
    rep = R.mesh_report(v, f)
    assert len(rep['components']) == 1 and rep['components'][0][1] == 0 and rep['manifold'] and rep['balanced'] and rep['components'][0][2] > 0
    assert np.abs(R.torus_sdf(v)).max() <= 0.5 * info['h']


def test_a_lattice_of_128_nodes_an_axis(ctx):
    """every level up to 128^3 through the driver, undisturbed samples: the restatement's residuals, field and level"""
    P, N = R.torus_cloud(8000, 100.0, 30.0, 0.0, seed=3)
    lo, h = R.cube_for(P, 7)
    ref = R.solve(P, N, lo, h, 7, fulldepth=7, iters=2, keep_levels=False)
    ctx.set_samples(P, N)
    used, occ = ctx.plan(lo, h, 7, 7, 1.5)
    alpha, res = ctx.solve(4.0, 2, 64)
    fld = ctx.field(return_field=True)
    assert used == 7 and occ == ref['occ'] and alpha == ref['alpha'] and res == ref['residuals']
    assert np.array_equal(bits(ctx.get_level('chi')), bits(ref['chi']))
    assert fld['thr'] == ref['thr'] and fld['E'] == ref['E'] and np.array_equal(fld['F'], ref['F'])


def test_inverted_normals_are_named(ctx):
    P, N = sized_cloud(4097)
    with pytest.raises(RuntimeError, match='the normals point inwards'):
        C.screened_poisson(P, -N, depth=5, fulldepth=5, context=ctx)


def test_orient_normals():
    P, N = torus()
    rng = np.random.default_rng(5)
    sign = np.where(rng.random(len(P)) < 0.5, -1.0, 1.0).astype(np.float32)
    v, f = C.screened_poisson(P, N, depth=7, fulldepth=4)
    mesh = type('Mesh', (), dict(vertices=v, faces=f))()
    out = C.orient_normals(P, N * sign[:, None], mesh)
    assert out.dtype == np.float32 and out.shape == N.shape
    same, turned = (out == N * sign[:, None]).all(1), (out == -(N * sign[:, None])).all(1)
    assert (same | turned).all()
    from ch_shrinkwrap_amd.distance import distance_to_mesh
    _, face = distance_to_mesh(P, mesh, signed=False, return_face=True)
    a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
    fn = np.cross(b - a, c - a)
    dots = (out.astype(np.float64) * fn).sum(1)
    # >= 0 up to the rounding of TriMesh's float32 face normals, which decided the sign: 8 float32 ulp of |normal| |face normal|
    assert (dots >= -8 * 2.0 ** -23 * np.linalg.norm(out, axis=1) * np.linalg.norm(fn, axis=1)).all()
    right = float(((out * N).sum(1) > 0).mean())
    print('orient_normals on the torus, true normals with random signs: %.4f come out outward' % right)
    assert right > 0.9


def test_the_recipe_module_on_a_simulated_cloud():
    from ch_shrinkwrap_amd.evaluation import mesh_properties, mesh_topology
    from ch_shrinkwrap_amd.membrane_mesh import MembraneMesh
    from ch_shrinkwrap_amd.simulation import PointcloudFromShape
    ns = {}
    PointcloudFromShape(output='filtered_localizations', shape_name='Torus', shape_params="{'radius': 100, 'r': 30}", density=0.004, p=1.0,
                        no_jitter=True).execute(ns)
    mesh = C.ScreenedPoissonMesh(use_normals=True, depth=6).execute(ns)
    assert isinstance(mesh, MembraneMesh) and ns['membrane'] is mesh and mesh.spr_info['runtime'] > 0 and 3 <= mesh.spr_info['depth_used'] <= 6
    q = mesh_properties(mesh)
    assert q['manifold'] and q['euler'] == 0 and q['genus'] == 1 and q['components'] == 1 and q['volume'] > 0
    assert mesh_topology(mesh.faces, len(mesh.vertices))['border_loops'] == 0                          # closed
    print('ScreenedPoissonMesh on the torus: %d vertices, %d faces, depth used %d, volume %.4g (true %.4g)' %
          (len(mesh.vertices), len(mesh.faces), mesh.spr_info['depth_used'], q['volume'], 2 * np.pi ** 2 * 100 * 30 ** 2))
