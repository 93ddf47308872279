"""
One table of localizations split into objects, and a membrane fitted to each.

    python examples/fit_objects.py [eps_nm] [min_points] [min_size]
        (eps 25 nm, min_points 10, min_size 100: the defaults; they are this scene's, read eps off clustering.k_distance_curve for another)

Two vesicles (R = 100 nm, centres 400 nm apart, 1 500 localizations each, 5 nm localization error) and 300 uniform background
localizations are simulated as one table.  `DBSCANClustering` labels it (include/nw_clustering.h: exact DBSCAN, a border point goes to its
nearest core point's clump), and every clump of at least `min_size` localizations goes through DensitySurface -> ShrinkwrapMembrane ->
fit_quality on its own.  The same fit on the raw table as one object is printed for comparison: the background is meshed with it, and the
two vesicles are one "surface" of two components.
"""
import sys
import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from ch_shrinkwrap_amd.clustering import DBSCANClustering         # noqa: E402
from ch_shrinkwrap_amd.evaluation import fit_quality, mesh_topology  # noqa: E402
from ch_shrinkwrap_amd.isosurface import DensitySurface           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane     # noqa: E402

R, GAP, SIGMA = 100.0, 400.0, 5.0


def sphere(rng, n, centre, sigma):
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u * R + np.asarray(centre) + rng.normal(0.0, sigma, (n, 3))


def simulate(seed=0):
    rng = np.random.default_rng(seed)
    P = np.concatenate([sphere(rng, 1500, (0.0, 0.0, 0.0), SIGMA), sphere(rng, 1500, (GAP, 0.0, 0.0), SIGMA)])
    lo, hi = P.min(0), P.max(0)
    c, half = 0.5 * (lo + hi), 0.6 * (hi - lo)
    return np.concatenate([P, rng.uniform(c - half, c + half, (300, 3))]).astype(np.float32)


def fit(table):
    ns = {'filtered_localizations': table}
    DensitySurface(method='knn', voxel_size=10.0).execute(ns)
    return ShrinkwrapMembrane().execute(ns)


def describe(mesh, truth):
    t = mesh_topology(mesh.faces, mesh.vertices.shape[0])
    return '%d faces, euler %d, %s, mse_rms %.2f nm' % (len(mesh.faces), t['euler'], 'closed' if t['border_loops'] == 0 else 'open',
                                                        fit_quality(mesh, truth)['mse_rms'])


def main(eps=25.0, min_points=10, min_size=100):
    P = simulate()
    sig = np.full(len(P), SIGMA, np.float32)
    table = {'x': P[:, 0], 'y': P[:, 1], 'z': P[:, 2], 'error_x': sig, 'error_y': sig, 'error_z': sig}
    ns = {'filtered_localizations': table}
    out = DBSCANClustering(search_radius=float(eps), min_clump_size=int(min_points)).execute(ns)
    md = out['metadata']
    print('%d localizations: %d clumps, %d core, %d border, %d noise' % (len(P), md['n_clusters'], md['info']['n_core'], md['info']['n_border'],
                                                                        md['info']['n_noise']))
    rng = np.random.default_rng(99)
    truths = [sphere(rng, 20000, (0.0, 0.0, 0.0), 0.0), sphere(rng, 20000, (GAP, 0.0, 0.0), 0.0)]
    n_objects = 0
    for c in range(md['n_clusters']):
        if md['sizes'][c] < int(min_size):
            continue
        m = out['dbscanClumpID'] == c + 1
        centre = 0.5 * (md['bbox'][c, :3] + md['bbox'][c, 3:])
        truth = truths[int(np.argmin([np.abs(centre - t.mean(0)).sum() for t in truths]))]
        print('object %d: %d localizations, box %s .. %s: %s' % (n_objects, int(m.sum()), np.round(md['bbox'][c, :3]).tolist(), np.round(md['bbox'][c, 3:]).tolist(),
                                                                describe(fit({k: v[m] for k, v in table.items()}), truth)))
        n_objects += 1
    print('%d objects' % n_objects)
    try:
        print('the raw table as one object: %s' % describe(fit(table), np.concatenate(truths)))
    except Exception as e:
        print('the raw table as one object: no fit (%s: %s)' % (type(e).__name__, e))
    return n_objects


if __name__ == '__main__':
    a = sys.argv[1:]
    main(float(a[0]) if len(a) > 0 else 25.0, int(a[1]) if len(a) > 1 else 10, int(a[2]) if len(a) > 2 else 100)
