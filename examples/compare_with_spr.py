"""
Both arms of the reference's evaluation (ch_shrinkwrap/evaluation.py: compute_shrinkwrap and compute_spr on the same simulated cloud) in
one process, every stage on the GPU:

    python examples/compare_with_spr.py [shape] [p]
        (shape: a name of examples/evaluate_shape.py's PARAMS, default TwoToruses; p: the share of the fluorophores that is detected,
        default 0.1)

    PointcloudFromShape (the noisy cloud) and PointcloudFromShape (the raw truth cloud: density 0.008, p = 1, no_jitter)
      (a) -> DensitySurface -> ShrinkwrapMembrane(max_iters=29, neck_first_iter=0)
      (b) -> ScreenedPoissonMesh(use_normals=True): the shape's own normals at the noisy positions
      each -> PointsFromMesh -> AverageSquaredDistance(backend='device')

It prints mse_rms of both arms against the truth cloud.  The screened Poisson arm is this project's grid solver, not pymeshlab's octree
solver (ch_shrinkwrap_amd/poisson.py says what it is).
"""
import sys
import time

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd.evaluation import AverageSquaredDistance, PointsFromMesh       # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface                               # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane                         # noqa: E402
from ch_shrinkwrap_amd.poisson import ScreenedPoissonMesh                              # noqa: E402
from ch_shrinkwrap_amd.simulation import PointcloudFromShape                           # noqa: E402
from examples.evaluate_shape import PARAMS                                             # noqa: E402


def score(ns, mesh_key, tag):
    PointsFromMesh(input=mesh_key, output=mesh_key + '_localizations', backend='device').execute(ns)
    q = AverageSquaredDistance(input=mesh_key + '_localizations', input2='raw', backend='device').execute(ns)
    print('%-12s mse01 %.3f nm^2   mse10 %.3f nm^2   mse_rms %.3f nm' % (tag, q['mse01'][0], q['mse10'][0], q['mse_rms'][0]))
    return q


def main(shape='TwoToruses', p=0.1, seed=0):
    if shape not in PARAMS:
        raise SystemExit('shape is one of %s' % ', '.join(sorted(PARAMS)))
    ns = {}
    cloud = PointcloudFromShape(output='filtered_localizations', shape_name=shape, shape_params=PARAMS[shape], p=p, noise_fraction=0,
                                psf_width_z=280.0, seed=seed).execute(ns)
    raw = PointcloudFromShape(output='raw', shape_name=shape, shape_params=PARAMS[shape], density=0.008, p=1.0, no_jitter=True, seed=seed).execute(ns)
    print('%s: %d localizations, %d truth points' % (shape, cloud['x'].size, raw['x'].size))
    t0 = time.time()
    DensitySurface().execute(ns)
    sw = ShrinkwrapMembrane(max_iters=29, neck_first_iter=0).execute(ns)
    t_sw = time.time() - t0
    ns['shrinkwrap'] = sw
    spr = ScreenedPoissonMesh(use_normals=True, output='spr').execute(ns)
    info = spr.spr_info
    print('shrink-wrap:      %d vertices / %d faces in %.2f s (start surface included)' % (sw.vertices.shape[0], sw.faces.shape[0], t_sw))
    print('screened Poisson: %d vertices / %d faces in %.2f s, depth used %d of 8, h %.2f nm, residuals of the last level %.3g -> %.3g' %
          (spr.vertices.shape[0], spr.faces.shape[0], info['runtime'], info['depth_used'], info['h'], *info['residuals'][info['depth_used']]))
    return score(ns, 'shrinkwrap', 'shrink-wrap'), score(ns, 'spr', 'SPR')


if __name__ == '__main__':
    args = sys.argv[1:]
    main(args[0] if len(args) > 0 else 'TwoToruses', float(args[1]) if len(args) > 1 else 0.1)
