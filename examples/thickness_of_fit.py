"""
How wide is the fitted structure -- a tube's diameter, a sheet's thickness?

    python examples/thickness_of_fit.py [scale] [n_rays]
        (scale 0.1 = 500 000 localizations, default; 1.0 = 5 000 000; n_rays 1, default: the inward normal alone; 30: a cone about it)

Runs the pipeline of examples/fit_from_cloud.py (DensitySurface -> ShrinkwrapMembrane on config C4, the start surface made from the
cloud) and then `MeshThickness`: from every vertex of the fit a ray along the inward normal (or a cone of rays about it) to the
first face it meets, cast exactly on the GPU (include/nw_rays.h).  C4 is a network of tubes of 50 nm radius and a sheet 50 nm
thick, so the quantiles should lie between the sheet's thickness and the tubes' diameter.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.rays import MeshThickness                  # noqa: E402


def main(scale=0.1, n_rays=1):
    cfg = synth.make_config('c4', scale=scale, seed=0)
    pts = cfg['points']
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2],
             'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    ns = {'filtered_localizations': table}
    DensitySurface(voxel_size=8.0 if scale >= 1.0 else 12.0).execute(ns)
    mesh = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)
    t0 = time.time()
    out = MeshThickness(n_rays=n_rays).execute(ns)
    dt = time.time() - t0
    th = out['thickness']
    ok = np.isfinite(th)
    qs = [1, 5, 25, 50, 75, 95, 99]
    print('%d vertices x %d rays against %d faces in %.3f s; %d vertices (%.2f %%) without a valid ray'
          % (th.size, n_rays, mesh.faces.shape[0], dt, (~ok).sum(), 100.0 * (~ok).mean()))
    print('local thickness of the fit, nm: ' + '  '.join('q%02d %.1f' % (q, v) for q, v in zip(qs, np.percentile(th[ok], qs))))
    return out


if __name__ == '__main__':
    main(float(sys.argv[1]) if len(sys.argv) > 1 else 0.1, int(sys.argv[2]) if len(sys.argv) > 2 else 1)
