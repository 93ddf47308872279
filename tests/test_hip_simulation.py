"""GPU tests of the SMLM cloud simulator (include/nw_simulation.h) against the reference's goldens, the NumPy restatement
(tests/simulation_ref.py) and the statistics the model promises.  Every test needs the nwg_ entry points: none passes without them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simulation_ref as R                                        # noqa: E402
from test_simulation import SDF_SHAPES, CASE_SHAPES, SIGMA_KW, dkw_bound, cdf_gap      # noqa: E402
from ch_shrinkwrap_amd import simulation as S                     # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
OFFSET = np.array([0.21, 0.13, 0.37])          # the lattice origin, in pitches off the cube's centre: no node sits on the shell's edge


@pytest.fixture(scope='module')
def ctx():
    c = S.SimulationContext(0)
    yield c
    c.close()


def _set(ctx, name, params):
    prog = S.compile_shape(name, params)
    ctx.set_program(prog)
    return prog


def test_sdf_and_normals_on_the_device(ctx):
    g = np.load(os.path.join(GOLDEN, 'sdf_shapes.npz'))
    for name in sorted(SDF_SHAPES):
        _set(ctx, *SDF_SHAPES[name])
        err = float(np.abs(ctx.eval(g['points']) - g[name]).max())
        print('sdf_shapes %-20s max |device - reference| = %.3e' % (name, err))
        assert err <= 1e-9, name
    g = np.load(os.path.join(GOLDEN, 'simulation_case.npz'))
    for name in sorted(CASE_SHAPES):
        _set(ctx, *CASE_SHAPES[name])
        err = float(np.abs(ctx.eval(g['points']) - g['sdf_' + name]).max())
        nerr = float(np.abs(ctx.normals(g['points']) - g['normals_' + name]).max())
        print('simulation_case %-14s sdf %.3e normals %.3e' % (name, err, nerr))
        assert err <= 1e-9 and nerr <= 1e-6, name


LATTICE_CASES = [('Sphere', dict(radius=100.0), 1.0), ('Sphere', dict(radius=100.0), 5.0), ('TwoToruses', dict(r=30, R=100), 1.0),
                 ('TwoToruses', dict(r=30, R=100), 5.0), ('ERSim2', {}, 4.0)]


@pytest.mark.parametrize('name,params,dx', LATTICE_CASES)
def test_lattice_matches_the_restatement(ctx, name, params, dx):
    prog = _set(ctx, name, params)
    centre, r_max, p, seed = prog.centre + OFFSET * dx, prog.r_max + 2 * dx, 0.25, 17
    want = R.lattice(prog.ops, centre, r_max, dx, p, seed)
    assert want['margin'] >= 1e-9, want['margin']              # the condition: no node within 1e-9 of the shell's edge, so no node is left out
    xyz, keys = ctx.sample_surface(centre, r_max, dx, p, seed=seed, return_keys=True)
    print('%s dx %g: %d detected of %d fluorophores, margin %.3e' % (name, dx, keys.size, want['n_fluorophores'], want['margin']))
    assert keys.size > 500 and np.array_equal(keys, want['keys'])
    assert float(np.abs(xyz - want['points']).max()) <= 1e-9
    lat = ctx.sample_surface(centre, r_max, dx, p, seed=seed, project=0)
    assert np.array_equal(lat, want['lattice'])


def test_fluorophore_count_is_the_area(ctx):
    """count x dx^2 within 1 % of the area at p = 1.  dx = 1: with the restatement the ratio is within 0.12 % of 1 at six lattice origins,
    for both shapes (at dx = 2 a lattice centred on the sphere is 1 % off: the aligned poles; a coarser pitch is not a fair case)."""
    dx = 1.0
    prog = _set(ctx, 'Sphere', dict(radius=100.0))
    n = ctx.sample_surface(prog.centre + OFFSET * dx, prog.r_max + 2 * dx, dx, 1.0, project=0).shape[0]
    ratio = n * dx * dx / (4 * np.pi * 100.0 ** 2)
    print('sphere: %d fluorophores, count dx^2 / area = %.5f' % (n, ratio))
    assert abs(ratio - 1.0) < 0.01
    prog = _set(ctx, 'UnionShape', dict(s0=('Torus', dict(radius=120.0, r=30.0, centroid=[-150.0, 0, 0])),
                                        s1=('Torus', dict(radius=120.0, r=30.0, centroid=[150.0, 0, 0]))))
    n = ctx.sample_surface(prog.centre + OFFSET * dx, prog.r_max + 2 * dx, dx, 1.0, project=0).shape[0]
    ratio = n * dx * dx / (2 * 4 * np.pi ** 2 * 120.0 * 30.0)          # the tori reach |x| = 300 and 0 from +-150: they do not overlap
    print('two tori: %d fluorophores, count dx^2 / area = %.5f' % (n, ratio))
    assert abs(ratio - 1.0) < 0.01


def test_thinning(ctx):
    prog = _set(ctx, 'TwoToruses', dict(r=30, R=100))
    dx, p = 1.0, 0.1
    centre, r_max = prog.centre + OFFSET * dx, prog.r_max + 2 * dx
    _, all_keys = ctx.sample_surface(centre, r_max, dx, 1.0, seed=3, project=0, return_keys=True)
    _, keys = ctx.sample_surface(centre, r_max, dx, p, seed=3, project=0, return_keys=True)
    big = all_keys.size
    print('thinning: %d of %d, expected %.0f +- %.0f' % (keys.size, big, p * big, np.sqrt(big * p * (1 - p))))
    assert abs(keys.size - p * big) < 5 * np.sqrt(big * p * (1 - p))
    assert np.isin(keys, all_keys).all()
    # another bounding cube (wider, its refinement starts a level higher): every node both hold is decided alike
    xyz = ctx.sample_surface(centre, r_max, dx, p, seed=3, project=0)
    xyz2, keys2 = ctx.sample_surface(centre, r_max + 300 * dx, dx, p, seed=3, project=0, return_keys=True)
    assert np.array_equal(keys2, keys) and np.array_equal(xyz2, xyz)


def test_localization_model(ctx):
    g = np.load(os.path.join(GOLDEN, 'simulation_case.npz'))
    n = int(g['sigma_n'])
    sigma, photons = ctx.loc_error(n, seed=5, return_photons=True, **SIGMA_KW)
    assert photons.min() >= 20.0
    mean = photons.mean(0)
    print('photons: min %.3f, mean per axis %s (expected 620 +- %.2f)' % (photons.min(), mean, 600 / np.sqrt(n)))
    assert (np.abs(mean - 620.0) < 5 * 600.0 / np.sqrt(n)).all()
    for a in range(3):
        gap = cdf_gap(sigma[:, a], g['sigma_quantiles'][:, a])
        print('sigma axis %d: CDF gap %.5f (bound %.5f)' % (a, gap, dkw_bound(n)))
        assert gap < dkw_bound(n)
    want, wl = R.loc_error(n, 5, S.STREAM_PHOTONS, **SIGMA_KW)
    assert np.allclose(sigma, want, rtol=1e-12, atol=0) and np.allclose(photons, wl, rtol=1e-12, atol=0)
    assert (ctx.loc_error(10, model=None) == 10.0).all()
    # float psf_width = the same width on every axis
    s1 = ctx.loc_error(1000, seed=5, psf_width=250.0)
    s3 = ctx.loc_error(1000, seed=5, psf_width=(250.0, 250.0, 250.0))
    assert np.array_equal(s1, s3)


def test_displacement_is_standard_normal_in_units_of_sigma():
    pts, nrm, sig, truth = S.generate_smlm_pointcloud_from_shape('TwoToruses', dict(r=30, R=100), density=1, p=0.2, psf_width=(280.0, 280.0, 840.0),
                                                                 mean_photon_count=600, bg_photon_count=20, noise_fraction=0.1, seed=9, return_truth=True)
    z = (pts - truth['clean']) / truth['sigma_used']
    n = z.shape[0]
    print('n = %d, mean %s, var %s' % (n, z.mean(0), z.var(0)))
    assert (np.abs(z.mean(0)) < 5 / np.sqrt(n)).all()
    assert (np.abs(z.var(0) - 1.0) < 5 * np.sqrt(2.0 / n)).all()
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-9 and sig.shape == pts.shape
    assert not np.array_equal(sig, truth['sigma_used'])        # a kept copy has a fresh sigma, not the one it was displaced by


def test_clusters(ctx):
    from scipy.stats import hypergeom
    n = 40000
    rng = np.random.default_rng(3)
    xyz, sigma = rng.uniform(-500, 500, (n, 3)), rng.uniform(2, 20, (n, 3))
    out, sig, copy = ctx.smlmify(xyz, sigma, seed=21, **SIGMA_KW)
    assert out.shape == (n, 3) and sig.shape == (n, 3) and copy.shape == (n,)
    assert (np.diff(copy) > 0).all() and copy.min() >= 0 and copy.max() < S.COPIES * n          # distinct, in copy order
    mult = np.bincount(copy % n, minlength=n)
    assert mult.mean() == 1.0 and mult.max() <= S.COPIES
    hist = np.bincount(mult, minlength=S.COPIES + 1)
    for k in range(S.COPIES + 1):
        pk = hypergeom.pmf(k, S.COPIES * n, S.COPIES, n)      # copies of one source among the n kept
        if n * pk >= 50:
            print('multiplicity %d: %d sources, expected %.1f' % (k, hist[k], n * pk))
            assert abs(hist[k] - n * pk) < 5 * np.sqrt(n * pk * (1 - pk))
    want_out, want_sig, want_copy = R.smlmify(xyz, sigma, 21, (S.STREAM_COPY_DISPLACE, S.STREAM_COPY_KEY, S.STREAM_COPY_PHOTONS), **SIGMA_KW)
    assert np.array_equal(copy, want_copy)
    assert np.abs(out - want_out).max() < 1e-9 and np.allclose(sig, want_sig, rtol=1e-12, atol=0)
    # fewer and more than n
    for sz in (1, 777, S.COPIES * 100):
        o, s, c = ctx.smlmify(xyz[:100], sigma[:100], sz=sz, seed=4, **SIGMA_KW)
        assert c.size == sz and (np.diff(c) > 0).all() and np.array_equal(c, R.select_copies(100, sz, 4, S.STREAM_COPY_KEY))


SCAN_TILE, SCAN_CHUNK = 2048, 1024          # csrc/nw_bq.hip: elements a workgroup scans, tile sums k_bq_scan_bsums takes before it carries


@pytest.mark.parametrize('n,tiles,last_tile', [(1024, 5, 2048), (209715, 1024, 2046), (209716, 1025, 8)])
def test_clusters_at_the_edges_of_the_scan(ctx, n, tiles, last_tile):
    """nwg_smlmify scans COPIES * n flags, twice: exactly five tiles; one chunk of tile sums with its last tile partial; the first
    tile beyond the chunk, whose offset is the carry."""
    nc = S.COPIES * n
    assert -(-nc // SCAN_TILE) == tiles and nc - (tiles - 1) * SCAN_TILE == last_tile and (tiles > SCAN_CHUNK) == (n == 209716)
    rng = np.random.default_rng(8)
    xyz, sigma = rng.uniform(-500, 500, (n, 3)), rng.uniform(2, 20, (n, 3))
    want_out, want_sig, want_copy = R.smlmify(xyz, sigma, 33, (S.STREAM_COPY_DISPLACE, S.STREAM_COPY_KEY, S.STREAM_COPY_PHOTONS), **SIGMA_KW)
    # (want_copy is R.select_copies(n, n, ...))
    assert want_copy.max() >= (tiles - 1) * SCAN_TILE          # (a copy of the last tile is kept: its slot needs every tile sum before it)
    out, sig, copy = ctx.smlmify(xyz, sigma, seed=33, **SIGMA_KW)
    assert out.shape == (n, 3) and sig.shape == (n, 3) and copy.shape == (n,)
    assert np.array_equal(copy, want_copy)
    assert np.abs(out - want_out).max() < 1e-9 and np.allclose(sig, want_sig, rtol=1e-12, atol=0)


def test_background(ctx):
    kw = dict(density=1, p=0.05, psf_width=(280.0, 280.0, 840.0), mean_photon_count=600, bg_photon_count=20, seed=2, context=ctx)
    shape = ('Torus', dict(radius=100.0, r=30.0, centroid=[600.0, 500.0, 900.0]))
    pts0, _, _ = S.generate_smlm_pointcloud_from_shape(*shape, noise_fraction=0, **kw)
    pts, _, sig, truth = S.generate_smlm_pointcloud_from_shape(*shape, noise_fraction=0.2, return_truth=True, **kw)
    n = pts0.shape[0]
    ln = int(0.2 * n / (1.0 - 0.2))
    assert pts.shape[0] == n + ln and np.array_equal(pts[:n], pts0) and sig.shape == pts.shape
    assert (truth['source'][:n] >= 0).all() and (truth['source'][n:] < 0).all()
    lo, hi = 1.2 * pts0.min(0), 1.2 * pts0.max(0)             # scaled about the origin: the box does not contain the cloud's lower corner
    bg = truth['clean'][n:]
    assert (bg >= lo).all() and (bg <= hi).all()
    assert (lo > pts0.min(0)).all()


def test_determinism(ctx):
    kw = dict(density=0.125, p=0.1, psf_width=(280.0, 280.0, 840.0), mean_photon_count=600, bg_photon_count=20, noise_fraction=0.1)
    a = S.generate_smlm_pointcloud_from_shape('ERSim2', {}, seed=1, **kw)
    b = S.generate_smlm_pointcloud_from_shape('ERSim2', {}, seed=1, context=ctx, **kw)
    c = S.generate_smlm_pointcloud_from_shape('ERSim2', {}, seed=2, **kw)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[0].shape != c[0].shape or not np.array_equal(a[0], c[0])
    prog = _set(ctx, 'ERSim2', {})
    ref = ctx.sample_surface(prog.centre + OFFSET, prog.r_max + 4.0, 2.0, 0.1, seed=1, return_keys=True)
    for level in (2, 3, 5, 9):                                  # (687 nodes an axis: levels 0 and 1 would list more start cells than the call accepts)
        got = ctx.sample_surface(prog.centre + OFFSET, prog.r_max + 4.0, 2.0, 0.1, seed=1, start_level=level, return_keys=True)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
    with pytest.raises(RuntimeError, match='start cells'):
        ctx.sample_surface(prog.centre + OFFSET, prog.r_max + 4.0, 2.0, 0.1, seed=1, start_level=0)
    # down to single nodes as start cells, on a cube small enough for that (45 nodes an axis)
    prog = _set(ctx, 'Sphere', dict(radius=100.0))
    ref = ctx.sample_surface(prog.centre + OFFSET, prog.r_max + 10.0, 5.0, 0.5, seed=1, return_keys=True)
    assert ref[1].size > 1000
    for level in (0, 1, 2, 4, 7, 20):
        got = ctx.sample_surface(prog.centre + OFFSET, prog.r_max + 10.0, 5.0, 0.5, seed=1, start_level=level, return_keys=True)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


def test_capacity(ctx):
    prog = _set(ctx, 'Sphere', dict(radius=100.0))
    n = ctx.sample_surface(prog.centre, prog.r_max + 2.0, 2.0, 1.0).shape[0]
    with pytest.raises(RuntimeError, match='max_points'):
        ctx.sample_surface(prog.centre, prog.r_max + 2.0, 2.0, 1.0, max_points=n - 1)
    assert ctx.n_points == 0
    assert ctx.L.nwg_get_points(ctx.h, None, None) == S.NWG_ERR_NOPOINTS
    assert ctx.sample_surface(prog.centre, prog.r_max + 2.0, 2.0, 1.0, max_points=n).shape[0] == n


def test_recipe_end_to_end():
    """The reference's evaluation recipe (test_evaluation_recipe.yaml) with DensitySurface in the place of Octree and DualMarchingCubes.
    The start surface's and the fit's mse_rms are printed (run with -s); no bound tighter than fit < start is fixed in advance."""
    from ch_shrinkwrap_amd.isosurface import DensitySurface
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    from ch_shrinkwrap_amd.evaluation import PointsFromMesh, AverageSquaredDistance, mesh_properties, mesh_topology
    from ch_shrinkwrap_amd.trimesh import TriMesh
    ns = {}
    S.PointcloudFromShape(output='filtered_localizations', shape_name='TwoToruses', p=0.1, noise_fraction=0, psf_width_z=280.0).execute(ns)
    S.PointcloudFromShape(output='raw', shape_name='TwoToruses', density=0.008, p=1.0, no_jitter=True).execute(ns)
    assert sorted(ns['raw']) == ['x', 'xn', 'y', 'yn', 'z', 'zn'] and 'error_z' in ns['filtered_localizations']
    surf = DensitySurface().execute(ns)

    def score(mesh, name):
        ns[name] = mesh
        PointsFromMesh(input=name, output=name + '_points', backend='device').execute(ns)
        return float(AverageSquaredDistance(input=name + '_points', input2='raw', backend='device').execute(ns)['mse_rms'][0])
    start = score(TriMesh(surf.vertices, surf.faces), 'start')
    mesh = ShrinkwrapMembrane(max_iters=29, neck_first_iter=0).execute(ns)
    fit = score(mesh, 'membrane0')
    q = mesh_properties(mesh)
    print('recipe: %d localizations, %d raw points; start surface mse_rms %.3f nm, fit %.3f nm; fit: %s'
          % (ns['filtered_localizations']['x'].size, ns['raw']['x'].size, start, fit, q))
    top = mesh_topology(mesh.faces, mesh.vertices.shape[0])
    assert top['manifold'] and top['border_loops'] == 0 and (top['twin'] >= 0).all()             # closed and manifold
    assert fit < start
