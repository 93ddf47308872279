"""
End-to-end example from the localizations alone: the start surface is made from the cloud, not handed in.

    python examples/fit_from_cloud.py [scale] [host | device] [knn]
        (scale 0.1 = 500 000 localizations, default; 1.0 = 5 000 000; the second argument is where the fit is scored:
        evaluation.fit_quality's backend, default host; a trailing `knn` makes the start surface the level set of the k-NN density,
        DensitySurface(method='knn'), whose bandwidth follows the cloud instead of the voxel size)

Upstream's recipe (ch_shrinkwrap/test_evaluation_recipe.yaml:25-38 in the reference) is Octree -> DualMarchingCubes -> ShrinkwrapMembrane;
here `DensitySurface` stands in for the first two (a regular-grid density isosurface on the GPU: it is not PYME's algorithm, see
ch_shrinkwrap_amd/isosurface.py) and `ShrinkwrapMembrane` is the third.  The scene is config C4 (the ER-like network with a fenestration);
the generator's own mesh is used for scoring only, never as input.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.evaluation import fit_quality              # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.surgery import euler_characteristic        # noqa: E402


def main(scale=0.1, score_backend='host', method='grid'):
    cfg = synth.make_config('c4', scale=scale, seed=0)
    pts = cfg['points']
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2],
             'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    ns = {'filtered_localizations': table}                        # no 'surf': DensitySurface makes it
    # a sparser cloud needs a coarser grid: 8 nm at full size, 12 nm below (the sizes profiles/isosurface_c4.txt and the tests use)
    voxel = 8.0 if scale >= 1.0 else 12.0
    t0 = time.time()
    surf = DensitySurface(voxel_size=voxel, method=method).execute(ns)
    t_surf = time.time() - t0
    chi = euler_characteristic(surf.faces)
    print('%d localizations -> start surface of %d vertices / %d faces in %.2f s (voxel %.1f nm, %d components found, %d removed), genus %d'
          % (pts.shape[0], surf.vertices.shape[0], surf.faces.shape[0], t_surf, voxel, surf.info['n_components'], len(surf.info['removed']),
             (2 - chi) // 2))
    t0 = time.time()
    mesh = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)
    dt = time.time() - t0
    q = fit_quality(mesh, synth.truth_cloud(cfg), backend=score_backend)
    print('fitted mesh %d vertices / %d faces in %.2f s, genus %d, mse_rms against the true surface %.2f nm'
          % (mesh.vertices.shape[0], mesh.faces.shape[0], dt, (2 - euler_characteristic(mesh.faces)) // 2, q['mse_rms']))
    return surf, mesh, q


if __name__ == '__main__':
    args = sys.argv[1:]
    method = 'knn' if args and args[-1] == 'knn' else 'grid'
    args = args[:-1] if method == 'knn' else args
    main(float(args[0]) if len(args) > 0 else 0.1, args[1] if len(args) > 1 else 'host', method)
