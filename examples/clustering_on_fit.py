"""
The clustering index of the localizations on a fitted membrane: the mesh coloured by the local Ripley L of the localizations near each
vertex, next to their density, and H(r) of the whole cloud.

    python examples/clustering_on_fit.py [scale] [radius_nm] [band_nm]
        (scale 0.25 = 250 000 localizations, default; radius 30 nm, default: where the local L is read; band 30 nm, default)

Config C3's two-lobe vesicle goes through the pipeline of examples/fit_from_cloud.py (DensitySurface -> ShrinkwrapMembrane, the start
surface made from the cloud).  Then `RipleysK` counts, for every localization, the localizations within `radius` of it (exact integers:
include/nw_pairs.h) and turns the count into the Getis-Franklin local L; that column goes into `SurfaceDensity` as a value column, so
every vertex gets the mean local L of the localizations mapped onto it.  The simulated cloud is uniform ON THE SURFACE, not in the
volume: in three dimensions it is strongly clustered, so H(r) = L(r) - r of the whole cloud is far above 0 at every radius below the
structure's size, and the per-vertex index is even over the surface.  No edge correction is applied anywhere.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.mapping import SurfaceDensity              # noqa: E402
from ch_shrinkwrap_amd.pairs import RipleysK                      # noqa: E402


def main(scale=0.25, radius=30.0, band=30.0):
    cfg = synth.make_config('c3', scale=scale, seed=0)
    points, sigma = cfg['points'], cfg['sigma']
    table = {'x': points[:, 0], 'y': points[:, 1], 'z': points[:, 2], 'error_x': sigma[:, 0], 'error_y': sigma[:, 1], 'error_z': sigma[:, 2]}
    ns = {'filtered_localizations': table}
    t0 = time.time()
    DensitySurface(voxel_size=12.0).execute(ns)
    mesh = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)
    t1 = time.time()
    k = RipleysK(r_max=4.0 * radius, n_steps=16, local_radius=radius).execute(ns)
    t2 = time.time()
    t = SurfaceDensity(input_points='ripley_localizations', band=band, columns=['ripley_local_L']).execute(ns)
    t3 = time.time()
    md = t['metadata']
    print('fit in %.2f s: %d vertices, %d faces' % (t1 - t0, t['x'].size, mesh.faces.shape[0]))
    print('pair counts in %.3f s: %d localizations, 16 radii up to %g nm and the local L at %g nm (%.0f distance tests a localization)'
          % (t2 - t1, len(points), 4.0 * radius, radius, k['metadata']['info']['tests'] / len(points)))
    print('mapping in %.3f s: %d of %d localizations within %g nm of the surface' % (t3 - t2, md['n_in_band'], md['n_total'], band))
    seen = np.isfinite(t['density']) & np.isfinite(t['mean_ripley_local_L'])
    qd, ql = np.percentile(t['density'][seen], [5, 50, 95]), np.percentile(t['mean_ripley_local_L'][seen], [5, 50, 95])
    print('  per vertex: density 5 %% %.3g, median %.3g, 95 %% %.3g per nm^2; clustering index (mean local L at %g nm) 5 %% %.1f, median %.1f, 95 %% %.1f nm'
          % (qd[0], qd[1], qd[2], radius, ql[0], ql[1], ql[2]))
    print('  the whole cloud, no edge correction:   r (nm)   K (nm^3)   L (nm)   H (nm)')
    for r, K, L, H in zip(k['r'], k['K'], k['L'], k['H']):
        print('  %40.0f %10.4g %8.1f %8.1f' % (r, K, L, H))
    return t, k


if __name__ == '__main__':
    main(*(float(x) for x in sys.argv[1:4]))
