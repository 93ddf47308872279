"""
The reference's evaluation recipe (ch_shrinkwrap/test_evaluation_recipe.yaml in the reference) end to end, every stage on the GPU:

    python examples/evaluate_shape.py [shape] [p] [knn]
        (shape: a name of ch_shrinkwrap_amd.simulation.SHAPES with the parameters below, default TwoToruses; p: the share of the
        fluorophores that is detected, default 0.1; a trailing `knn` makes the start surface the level set of the k-NN density,
        DensitySurface(method='knn'), which is what lets p go down towards upstream's sweep)

    PointcloudFromShape (the noisy cloud) and PointcloudFromShape (the raw truth cloud: density 0.008, p = 1, no_jitter)
      -> DensitySurface (in the place of upstream's Octree -> DualMarchingCubes) -> ShrinkwrapMembrane(max_iters=29, neck_first_iter=0)
      -> PointsFromMesh -> AverageSquaredDistance(backend='device')

It prints the recipe's three numbers: mse01, mse10 and mse_rms of the fitted membrane against the truth cloud.
"""
import sys
import time

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd.evaluation import AverageSquaredDistance, PointsFromMesh       # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface                               # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane                         # noqa: E402
from ch_shrinkwrap_amd.simulation import PointcloudFromShape                           # noqa: E402

PARAMS = {'TwoToruses': "{'r': 30, 'R': 100}", 'Sphere': "{'radius': 100}", 'DualCapsule': "{'length': 400, 'r': 40, 'sep': 150}",
          'ThreeWayJunction': "{'h': 300, 'r': 50, 'k': 20}", 'ERSim2': '{}',
          'NToruses': "{'toruses': {'one': {'r': 30, 'R': 100}, 'two': {'r': 10, 'R': 75}, 'three': {'r': 30, 'R': 150}}}"}


def main(shape='TwoToruses', p=0.1, seed=0, method='grid'):
    if shape not in PARAMS:
        raise SystemExit('shape is one of %s' % ', '.join(sorted(PARAMS)))
    ns = {}
    t0 = time.time()
    cloud = PointcloudFromShape(output='filtered_localizations', shape_name=shape, shape_params=PARAMS[shape], p=p, noise_fraction=0,
                                psf_width_z=280.0, seed=seed).execute(ns)
    raw = PointcloudFromShape(output='raw', shape_name=shape, shape_params=PARAMS[shape], density=0.008, p=1.0, no_jitter=True, seed=seed).execute(ns)
    t_sim = time.time() - t0
    print('%s: %d localizations, %d truth points in %.2f s' % (shape, cloud['x'].size, raw['x'].size, t_sim))
    surf = DensitySurface(method=method).execute(ns)
    print('start surface: %d vertices / %d faces' % (surf.vertices.shape[0], surf.faces.shape[0]))
    t0 = time.time()
    mesh = ShrinkwrapMembrane(max_iters=29, neck_first_iter=0).execute(ns)
    print('fitted membrane: %d vertices / %d faces in %.2f s' % (mesh.vertices.shape[0], mesh.faces.shape[0], time.time() - t0))
    PointsFromMesh(input='membrane', output='membrane_localizations', backend='device').execute(ns)
    q = AverageSquaredDistance(input='membrane_localizations', input2='raw', backend='device').execute(ns)
    print('mse01 %.3f nm^2   mse10 %.3f nm^2   mse_rms %.3f nm' % (q['mse01'][0], q['mse10'][0], q['mse_rms'][0]))
    return q


if __name__ == '__main__':
    args = sys.argv[1:]
    method = 'knn' if args and args[-1] == 'knn' else 'grid'
    args = args[:-1] if method == 'knn' else args
    main(args[0] if len(args) > 0 else 'TwoToruses', float(args[1]) if len(args) > 1 else 0.1, method=method)
