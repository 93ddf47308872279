"""
How far do the localizations lie from the surface that was fitted to them, and on which side?

    python examples/distance_to_fit.py [scale]
        (scale 0.1 = 500 000 localizations, default; 1.0 = 5 000 000)

Runs the pipeline of examples/fit_from_cloud.py (DensitySurface -> ShrinkwrapMembrane on config C4, the start surface made from the
cloud) and then `DistanceToMesh`: the exact distance of every localization from the fitted triangles on the GPU, negative inside
(include/nw_distance.h).  A good fit leaves the localizations scattered to both sides by about their localization error.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.distance import DistanceToMesh             # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402


def main(scale=0.1):
    cfg = synth.make_config('c4', scale=scale, seed=0)
    pts = cfg['points']
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2],
             'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    ns = {'filtered_localizations': table}
    DensitySurface(voxel_size=8.0 if scale >= 1.0 else 12.0).execute(ns)
    mesh = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)
    t0 = time.time()
    out = DistanceToMesh().execute(ns)
    dt = time.time() - t0
    d = out['distance_to_mesh']
    qs = [1, 5, 25, 50, 75, 95, 99]
    print('%d localizations against %d faces in %.3f s' % (d.size, mesh.faces.shape[0], dt))
    print('signed distance to the fit, nm (negative inside): ' + '  '.join('q%02d %+.2f' % (q, v) for q, v in zip(qs, np.percentile(d, qs))))
    print('%.1f %% inside; median |distance| %.2f nm against a median localization error of %.2f nm'
          % (100.0 * (d < 0).mean(), np.median(np.abs(d)), np.median(cfg['sigma'])))
    return out


if __name__ == '__main__':
    main(float(sys.argv[1]) if len(sys.argv) > 1 else 0.1)
