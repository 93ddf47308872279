"""
The surface 20 nm outside a fit, and the fit as an inside mask on a voxel grid.

    python examples/offset_of_fit.py [scale] [offset_nm]
        (scale 0.1 = 500 000 localizations, default; 1.0 = 5 000 000; offset 20 nm, default; negative: inwards)

Runs the pipeline of examples/fit_from_cloud.py (DensitySurface -> ShrinkwrapMembrane on config C4, the start surface made from the
cloud) and then `OffsetSurface`: the level set of the fit's exact signed distance at `offset`, meshed on the GPU without the field
leaving the device (include/nw_volume.h, include/nw_isosurface.h) -- and `MeshToVolume`: the signed distance image and the inside
mask on an 8 nm lattice, as another channel's analysis would take them.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.volume import MeshToVolume, OffsetSurface  # noqa: E402


def main(scale=0.1, offset=20.0):
    cfg = synth.make_config('c4', scale=scale, seed=0)
    pts = cfg['points']
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2],
             'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    ns = {'filtered_localizations': table}
    DensitySurface(voxel_size=8.0 if scale >= 1.0 else 12.0).execute(ns)
    mesh = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)
    t0 = time.time()
    surf = OffsetSurface(offset=offset, voxel_size=8.0).execute(ns)
    t1 = time.time()
    vol = MeshToVolume(voxel_size=8.0).execute(ns)
    t2 = time.time()
    print('fit: %d faces; surface at %+g nm: %d vertices, %d faces in %.3f s (lattice %s, %d of %d nodes in band)'
          % (mesh.faces.shape[0], offset, surf.vertices.shape[0], surf.faces.shape[0], t1 - t0, surf.info['dims'], surf.info['in_band'], surf.info['nodes']))
    print('volume: lattice %s at 8 nm, band %g nm, in %.3f s; %.2f %% of the nodes inside, %.2f %% in band'
          % (vol['dims'], vol['d_cap'], t2 - t1, 100.0 * vol['mask'].mean(), 100.0 * (vol['face'] >= 0).mean()))
    return surf, vol


if __name__ == '__main__':
    main(float(sys.argv[1]) if len(sys.argv) > 1 else 0.1, float(sys.argv[2]) if len(sys.argv) > 2 else 20.0)
