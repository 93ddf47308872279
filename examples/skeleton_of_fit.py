"""
The centreline graph of a fitted network: how many branches, how long, how thick, how many loops.

    python examples/skeleton_of_fit.py [scale] [band_width_in_mean_edges] [prune]
        (scale 0.1 = 500 000 localizations, default; band width 2 mean edge lengths; prune 1.0: end branches shorter than their
        junction's radius are dropped)

The pipeline of examples/fit_from_cloud.py on config C4 (the ER-like network with a fenestration): `DensitySurface` makes the start
surface from the cloud, `ShrinkwrapMembrane` fits it.  `level_set_skeleton` then cuts the fit into bands of the geodesic graph distance
from a double sweep (include/nw_skeleton.h: every connected piece of a band is a node, the node sits at the centre of its contour, the
contour's perimeter gives the radius) and `skeleton_graph` reads branches, junctions and loops off the graph.

THIS IS A LEVEL-SET DIAGRAM OF ONE FIELD, not a medial axis: it depends on the source, a sheet becomes a chain, and a loop narrower than a
band vanishes -- which is why the loop count is printed next to the genus the mesh's Euler characteristic gives.
"""
import sys
import time
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd import synth                               # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface, mean_edge_length         # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402
from ch_shrinkwrap_amd.surgery import euler_characteristic        # noqa: E402
from ch_shrinkwrap_amd.distance import _mesh_arrays               # noqa: E402
from ch_shrinkwrap_amd.skeleton import level_set_skeleton, skeleton_graph, branch_of_vertex       # noqa: E402


def main(scale=0.1, bands=2.0, prune=1.0):
    cfg = synth.make_config('c4', scale=scale, seed=0)
    pts = cfg['points']
    ns = {'filtered_localizations': {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1],
                                     'error_z': cfg['sigma'][:, 2]}}
    DensitySurface(voxel_size=8.0 if scale >= 1.0 else 12.0).execute(ns)
    mesh = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale))).execute(ns)
    pos, faces, _ = _mesh_arrays(mesh, False)
    edge = mean_edge_length(pos, faces)
    t0 = time.time()
    r = level_set_skeleton(mesh, band_width=bands * edge)
    dt = time.time() - t0
    g = skeleton_graph(r, prune=prune)
    i = r['info']
    print('fit of %d vertices / %d faces, mean edge %.1f nm; bands of %.1f nm: %d pieces, %d nodes, %d arcs in %.3f s (two distance fields included)'
          % (pos.shape[0], faces.shape[0], edge, r['band_width'], i['pieces'], i['nodes'], i['arcs'], dt))
    print('branches %d (pruned at %.1f x the junction radius: %d of %d nodes kept), junctions %d, ends %d, components %d'
          % (g['n_branches'], prune, int(g['kept'].sum()), g['kept'].size, g['junctions'].size, g['ends'].size, g['n_components']))
    print('total length %.0f nm; loops of the graph %d, genus of the mesh %d (a loop narrower than a band of %.0f nm is not in the graph)'
          % (g['total_length'], g['n_loops'], (2 - euler_characteristic(faces)) // 2, r['band_width']))
    radius = r['nodes']['radius'][g['kept'] & (r['nodes']['perimeter'] > 0)]
    if radius.size:
        hist, edges = np.histogram(radius, bins=8)
        print('node radius (contour perimeter / 2 pi), nm:')
        for lo, hi, n in zip(edges[:-1], edges[1:], hist):
            print('  %7.1f .. %7.1f   %5d %s' % (lo, hi, n, '#' * int(round(40.0 * n / max(1, hist.max())))))
    for k, b in sorted(enumerate(g['branches']), key=lambda kb: -kb[1]['length'])[:10]:
        print('  branch %3d: nodes %4d .. %4d, %3d nodes, length %7.0f nm, mean radius %6.1f nm' % (k, b['ends'][0], b['ends'][1], b['nodes'].size, b['length'], b['mean_radius']))
    on_branch = branch_of_vertex(r, g)
    print('%d of %d vertices lie on a branch, %d on a junction, a pruned node or nothing' % (int((on_branch >= 0).sum()), on_branch.size, int((on_branch < 0).sum())))
    return r, g


if __name__ == '__main__':
    main(*(float(x) for x in sys.argv[1:4]))
