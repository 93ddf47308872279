"""
The local shape of a cloud before any fit: which localizations sit on a tubule, which on a sheet, which in a blob, and the normals.

    python examples/shape_of_cloud.py [shape] [radius_nm]
        (shape ThreeWayJunction, default, TwoToruses or ERSim2; radius 0, default: 1.5 x the median distance to the 20th neighbour)

`PointcloudFromShape` simulates an SMLM cloud of the shape, `LocalShape` adds to its table, per localization, the neighbour count, the
three shape features (linearity, planarity, scattering: they add up to 1), the normal xn yn zn, the axis xa ya za and shape_class
(0 line, 1 plane, 2 blob, -1 where fewer than three neighbours).  The moments behind them are exact integers (include/nw_structure.h), so
the table does not depend on the order of the cloud.  Seen from a radius well below the tube's, a tubule's wall is a sheet; from a radius
above it, a line: the class shares printed here move with the radius.  The simulated table carries the shape's own normals, so the angle
between the two is printed as well.

With a fit at hand (examples/fit_from_cloud.py), the output table is a table of localizations like any other:
`SurfaceDensity(input_points='shape_localizations', columns=['linearity', 'planarity'])` takes the two columns to the fitted surface, the
tubule / sheet map of the network per vertex (replace the NaN of the localizations that are not valid first).  This example does not
fit: the sparse clouds it simulates are below what DensitySurface's defaults make a closed start surface from.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd.simulation import PointcloudFromShape      # noqa: E402
from ch_shrinkwrap_amd.structure import LocalShape                # noqa: E402

SHAPES = {'ThreeWayJunction': ("{'h': 300, 'r': 40}", 0.02), 'TwoToruses': ("{'r': 30, 'R': 100}", 0.02), 'ERSim2': ('{}', 0.004)}


def main(shape='ThreeWayJunction', radius=0.0):
    params, p = SHAPES[shape]
    ns = {}
    src = PointcloudFromShape(output='filtered_localizations', shape_name=shape, shape_params=params, p=p, psf_width_x=140.0, psf_width_y=140.0,
                              psf_width_z=280.0, noise_fraction=0.1).execute(ns)
    t0 = time.time()
    t = LocalShape(radius=float(radius) if float(radius) > 0 else None).execute(ns)
    t1 = time.time()
    n, cls = t['x'].size, t['shape_class']
    print('%s: %d localizations; radius %.1f nm, %.1f neighbours in the median; local shape in %.3f s'
          % (shape, n, t['metadata']['radius'], np.median(t['n_neighbours']), t1 - t0))
    print('  line %.1f %%, plane %.1f %%, blob %.1f %%, too few neighbours %.1f %%'
          % tuple(100.0 * float((cls == c).mean()) for c in (0, 1, 2, -1)))
    truth = np.stack([src['xn'], src['yn'], src['zn']], 1).astype(np.float64)
    mine = np.stack([t['xn'], t['yn'], t['zn']], 1)
    ok = (cls >= 0) & (np.linalg.norm(truth, axis=1) > 0)
    cos = np.abs((mine[ok] * truth[ok]).sum(1)) / np.linalg.norm(truth[ok], axis=1)
    ang = np.degrees(np.arccos(np.minimum(1.0, cos)))
    print('  normal against the shape\'s own, up to sign (the background included): median %.1f deg, 90 %% below %.1f deg' % (np.median(ang), np.percentile(ang, 90)))
    return t


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if len(a) > 0 else 'ThreeWayJunction', float(a[1]) if len(a) > 1 else 0.0)
