"""
Contact sites between two fitted membranes: where a tube comes within 30 nm of a vesicle, how large the patch is and what the gap is.

    python examples/contacts_of_two_fits.py [scale] [gap_nm] [contact_distance_nm]
        (scale 0.25 = 250 000 + 50 000 localizations, default; gap 40 nm, default: the distance between the two true surfaces)

Two structures as a two-colour experiment would give them: config C3's two-lobe vesicle and config C2's capped tube, the tube moved so
that it passes the vesicle's right lobe at `gap` nm.  Each cloud goes through the pipeline of examples/fit_from_cloud.py on its own
(DensitySurface -> ShrinkwrapMembrane, the start surface made from the cloud), then `MembraneContacts` takes the two fits: the exact
distance of every face of one mesh from the other mesh (include/nw_proximity.h), the faces within the contact distance, their
edge-connected patches and areas.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.proximity import MembraneContacts          # noqa: E402


def fit(points, sigma, scale):
    table = {'x': points[:, 0], 'y': points[:, 1], 'z': points[:, 2], 'error_x': sigma[:, 0], 'error_y': sigma[:, 1], 'error_z': sigma[:, 2]}
    ns = {'filtered_localizations': table}
    DensitySurface(voxel_size=12.0).execute(ns)
    return ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)


def main(scale=0.25, gap=40.0, contact_distance=30.0):
    vesicle, tube = synth.make_config('c3', scale=scale, seed=0), synth.make_config('c2', scale=scale, seed=1)
    # the vesicle's right lobe ends at x = 550, the tube has radius 50 about the y axis
    shift = np.array([550.0 + gap + 50.0, 0.0, 0.0], np.float32)
    t0 = time.time()
    a = fit(vesicle['points'], vesicle['sigma'], scale)
    b = fit((tube['points'] + shift).astype(np.float32), tube['sigma'], scale)
    t1 = time.time()
    ns = {'membrane': a, 'membrane2': b}
    t = MembraneContacts(contact_distance=contact_distance).execute(ns)
    t2 = time.time()
    md = t['metadata']
    print('two fits in %.2f s: vesicle %d faces, tube %d faces; true gap %g nm' % (t1 - t0, a.faces.shape[0], b.faces.shape[0], gap))
    print('contacts within %g nm in %.3f s: %d faces of the vesicle (%.0f nm^2) in %d patch(es), %.0f nm^2 of the tube in %d patch(es); '
          'crossing faces %d / %d' % (contact_distance, t2 - t1, t['distance'].size, md['area_a'], len(md['patch_area_a']), md['area_b'],
                                      len(md['patch_area_b']), md['n_crossing_a'], md['n_crossing_b']))
    for k, area in enumerate(md['patch_area_a']):
        rows = t['patch'] == k
        i = np.flatnonzero(rows)[np.argmin(t['distance'][rows])]
        print('  patch %d of the vesicle: %d faces, %.0f nm^2, smallest gap %.2f nm at (%.1f, %.1f, %.1f), mean gap %.2f nm'
              % (k, rows.sum(), area, t['distance'][i], t['x'][i], t['y'][i], t['z'][i], t['distance'][rows].mean()))
    return t


if __name__ == '__main__':
    main(*(float(x) for x in sys.argv[1:4]))
