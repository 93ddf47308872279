"""
The density of localizations on a fitted membrane: the mesh coloured by localizations per nm^2, and a column's mean per vertex.

    python examples/density_on_fit.py [scale] [band_nm] [smooth]
        (scale 0.25 = 250 000 localizations, default; band 30 nm, default; smooth 1, default: rounds of summing over a vertex's ring)

Config C3's two-lobe vesicle goes through the pipeline of examples/fit_from_cloud.py (DensitySurface -> ShrinkwrapMembrane, the start
surface made from the cloud), then `SurfaceDensity` takes the fit and the cloud: every localization within `band` of the surface is
split between the three corners of its closest face (include/nw_mapping.h), in integers, so the table does not depend on the order of
the cloud.  The simulated cloud is uniform on the surface: the per-vertex densities scatter about localizations / area as Poisson
counts do.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.mapping import SurfaceDensity              # noqa: E402


def main(scale=0.25, band=30.0, smooth=1):
    cfg = synth.make_config('c3', scale=scale, seed=0)
    points, sigma = cfg['points'], cfg['sigma']
    table = {'x': points[:, 0], 'y': points[:, 1], 'z': points[:, 2], 'error_x': sigma[:, 0], 'error_y': sigma[:, 1], 'error_z': sigma[:, 2]}
    ns = {'filtered_localizations': table}
    t0 = time.time()
    DensitySurface(voxel_size=12.0).execute(ns)
    mesh = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)
    t1 = time.time()
    t = SurfaceDensity(band=band, columns=['error_x'], smooth=int(smooth)).execute(ns)
    t2 = time.time()
    md, mapped = t['metadata'], ns['mapped_localizations']
    seen = np.isfinite(t['density'])
    raw = SurfaceDensity(band=band, output='raw_density', output_points='raw_points').execute(ns)
    total_area = raw['area'].sum()
    print('fit in %.2f s: %d vertices, %d faces, %.0f nm^2' % (t1 - t0, t['x'].size, mesh.faces.shape[0], total_area))
    print('density in %.3f s: %d of %d localizations within %g nm of the surface; %.3g per nm^2 overall'
          % (t2 - t1, md['n_in_band'], md['n_total'], band, md['n_in_band'] / total_area))
    q = np.percentile(t['density'][seen], [5, 50, 95])
    print('  per vertex after %d round(s) of smoothing: 5 %% %.3g, median %.3g, 95 %% %.3g per nm^2; mean error_x per vertex: median %.2f nm'
          % (int(smooth), q[0], q[1], q[2], np.nanmedian(t['mean_error_x'])))
    d = mapped['surface_distance']
    print('  distance of the in-band localizations from the surface: median %.2f nm, 95 %% %.2f nm' % (np.median(d[np.isfinite(d)]), np.percentile(d[np.isfinite(d)], 95)))
    return t


if __name__ == '__main__':
    main(*(float(x) for x in sys.argv[1:4]))
