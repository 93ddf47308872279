"""
Distance along a fitted membrane: how the localization density of one fit falls off with the distance from its contact sites with
another fit, measured along the surface and, next to it, through space.

    python examples/distance_along_fit.py [scale] [gap_nm] [contact_distance_nm] [bin_nm]
        (scale 0.25 = 250 000 + 50 000 localizations, default; gap 40 nm; contact distance 60 nm; bins of 100 nm)

The scene of examples/contacts_of_two_fits.py: config C3's two-lobe vesicle and config C2's capped tube passing its right lobe.  Each
cloud goes through the pipeline of examples/fit_from_cloud.py, `contact_sites` finds the patches of the vesicle within the contact
distance of the tube, `sources_from_faces` turns them into source vertices and `geodesic_distance` gives every vertex of the vesicle
its distance from the nearest patch ALONG the fit (include/nw_geodesic.h: a graph distance over edges and unfolded face diagonals, an
upper bound of the geodesic).  `surface_density` maps the vesicle's cloud onto its fit, and `surface_profile` prints the area-weighted
density in bins of that distance -- and the same profile against the straight-line distance from the patch centroids, which reaches the
far lobe through the lumen and the neck much sooner than the membrane does.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.proximity import contact_sites             # noqa: E402
from ch_shrinkwrap_amd.mapping import surface_density             # noqa: E402
from ch_shrinkwrap_amd.geodesic import geodesic_distance, sources_from_faces, surface_profile      # noqa: E402


def fit(points, sigma, scale):
    table = {'x': points[:, 0], 'y': points[:, 1], 'z': points[:, 2], 'error_x': sigma[:, 0], 'error_y': sigma[:, 1], 'error_z': sigma[:, 2]}
    ns = {'filtered_localizations': table}
    DensitySurface(voxel_size=12.0).execute(ns)
    return ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)


def main(scale=0.25, gap=40.0, contact_distance=60.0, bin_nm=100.0):
    vesicle, tube = synth.make_config('c3', scale=scale, seed=0), synth.make_config('c2', scale=scale, seed=1)
    shift = np.array([550.0 + gap + 50.0, 0.0, 0.0], np.float32)
    a = fit(vesicle['points'], vesicle['sigma'], scale)
    b = fit((tube['points'] + shift).astype(np.float32), tube['sigma'], scale)
    sites = contact_sites(a, b, distance=contact_distance)
    ids, patch = sources_from_faces(a.faces, sites['patches_a'])
    if ids.size == 0:
        print('no face of the vesicle within %g nm of the tube: nothing to measure from' % contact_distance)
        return None
    t0 = time.time()
    field = geodesic_distance(a, ids, labels=True)
    t1 = time.time()
    i = field['info']
    print('vesicle %d vertices; %d contact patch(es), %d source vertices; distance along the fit in %.3f s: %d + %d rounds, %d launches, %d diagonals'
          % (a.vertices.shape[0], len(sites['patch_area_a']), ids.size, t1 - t0, i['rounds'], i['label_rounds'], i['launches'], i['diagonals']))
    dens = surface_density(vesicle['points'], a, band=30.0, smooth=1)
    P = np.asarray(a.vertices, np.float64)
    centroids = np.stack([P[ids[patch == k]].mean(0) for k in np.unique(patch)])
    straight = np.linalg.norm(P[:, None, :] - centroids[None, :, :], axis=2).min(1)
    reach = field['distance'][np.isfinite(field['distance'])].max()
    edges = np.arange(0.0, reach + bin_nm, bin_nm)
    along = surface_profile(field['distance'], dens['density'], dens['area'], edges)
    through = surface_profile(straight, dens['density'], dens['area'], edges)
    print('farthest vertex: %.0f nm along the fit, %.0f nm through space' % (reach, straight.max()))
    print('  distance nm     along the fit: area nm^2  density /nm^2     through space: area nm^2  density /nm^2')
    for r, m1, a1, m2, a2 in zip(along[0], along[1], along[2], through[1], through[2]):
        print('  %8.0f       %20.0f  %12.4g       %20.0f  %12.4g' % (r, a1, m1, a2, m2))
    return field


if __name__ == '__main__':
    main(*(float(x) for x in sys.argv[1:5]))
