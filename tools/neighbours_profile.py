"""Wall time of the k-th-neighbour queries through kept contexts (profiles/neighbours.txt): local_density on the clouds of configs C3 and
C4, and node_field on C4's 8 nm grid (the grid of profiles/isosurface_c4.txt) at k = 20 for two threshold densities of upstream's sweep,
each against scipy's cKDTree on the same host and against nwi_density on the same grid.
usage: python tools/neighbours_profile.py [scale] [nohost]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/neighbours_profile.py 1.0 nohost   (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, build, neighbours as N, isosurface as I

scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
host = not (len(sys.argv) > 2 and sys.argv[2] == 'nohost')
workers = int(os.environ.get('OMP_NUM_THREADS', '16'))
K = 20
ms = lambda a: ' '.join('%.1f' % (1e3 * x) for x in a)


def timed(fn, n=3):
    out, t = None, []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return out, t


if os.path.exists(build.OBJ_NEIGHBOURS):                       # (the object is there after a build in this tree)
    for k, r in sorted(build.kernel_resources(build.OBJ_NEIGHBOURS).items()):
        print('%-14s %d VGPRs, %d SGPRs, %d bytes of LDS, scratch %d, spills %d / %d' % (k, r['vgpr'], r['sgpr'], r['lds'], r['scratch'], r['vgpr_spill'], r['sgpr_spill']))

ctx = N.NeighbourContext()
clouds = {}
for name in ('c3', 'c4'):
    pts = np.ascontiguousarray(synth.make_config(name, scale=scale, seed=0)['points'], np.float32)
    clouds[name] = pts
    t0 = time.perf_counter()
    ctx.set_cloud(pts)
    first = time.perf_counter() - t0
    _, sets = timed(lambda: ctx.set_cloud(pts))
    r, qs = timed(lambda: ctx.kth_distance(pts, K + 1))
    dens, whole = timed(lambda: N.local_density(pts, K, context=ctx))
    print('%s x%g: %d localizations; set_cloud first %.1f ms, then %s ms; kth_distance(k = %d) at the cloud %s ms (min %.1f, %.1f ns a point); '
          'local_density %s ms; median density %.3e nm^-3, r_%d quantiles 5/50/95 %%: %s nm'
          % (name, scale, pts.shape[0], 1e3 * first, ms(sets), K + 1, ms(qs), 1e3 * min(qs), 1e9 * min(qs) / pts.shape[0], ms(whole),
             float(np.median(dens)), K, np.round(np.percentile(r, [5, 50, 95]), 2)))
    if host:
        from scipy.spatial import cKDTree
        p64 = pts.astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(p64)
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        d = tree.query(p64, k=K + 1, workers=workers)[0][:, -1]
        t_query = time.perf_counter() - t0
        nz = d > 0
        print('%s: cKDTree build %.2f s, query(k = %d, %d workers) %.2f s; largest relative difference from the device %.2e'
              % (name, t_build, K + 1, workers, t_query, float((np.abs(r[nz] - d[nz]) / d[nz]).max())))
        if name == 'c4':
            clouds['tree'] = tree

pts = clouds['c4']
h = 8.0
lo, dims = I.grid_for(pts, h, 5)                                  # the grid of profiles/isosurface_c4.txt: passes + 3 voxels of margin
print('c4 grid at %.0f nm: %d x %d x %d = %d nodes' % (h, dims[0], dims[1], dims[2], int(np.prod(dims.astype(np.int64)))))
ctx.set_cloud(pts)
ictx = I.IsosurfaceContext()
_, dens_t = timed(lambda: ictx.density(pts, lo, h, dims, 2))
print('nwi_density (2 passes) on the same grid, host cloud: %s ms' % ms(dens_t))
for td in (2e-3, 2e-5):
    R_thr, r_cap, pad, thr = I.knn_threshold(h, K, td)
    field, t = timed(lambda: ctx.node_field(lo, h, dims, K, r_cap, return_field=True))
    _, t_dev = timed(lambda: ctx.node_field(lo, h, dims, K, r_cap))
    t0 = time.perf_counter()
    ictx.set_field(ctx.field_pointer(), lo, h, dims)
    try:
        v, f = ictx.extract(thr)
        mesh = '%d vertices / %d faces' % (v.shape[0], f.shape[0])
    except RuntimeError as e:                                     # (this grid's margin is the density chain's, not ceil(R_thr / h) + 2)
        mesh = str(e)
    t_ext = time.perf_counter() - t0
    print('threshold %.0e nm^-3: R_thr %.1f nm, r_cap %.1f nm; node_field with the copy to the host %s ms, without %s ms (min %.1f, %.1f ns a node); '
          '%.1f %% of the nodes below the cap; set_field + extract %.1f ms: %s'
          % (td, R_thr, r_cap, ms(t), ms(t_dev), 1e3 * min(t_dev), 1e9 * min(t_dev) / field.size, 100.0 * float((field > 0).mean()), 1e3 * t_ext, mesh))
    if host:
        ax = [float(lo[a]) + (np.arange(int(dims[a]), dtype=np.float64) + 0.5) * float(np.float32(h)) for a in range(3)]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing='ij')
        nodes = np.stack([x.ravel(), y.ravel(), z.ravel()], 1)
        t0 = time.perf_counter()
        d = clouds['tree'].query(nodes, k=K, distance_upper_bound=r_cap, workers=workers)[0][:, -1]
        t_query = time.perf_counter() - t0
        ref = np.floor((r_cap - np.minimum(d, r_cap)) * 1048576.0).astype(np.uint64).reshape(field.shape)
        diff = np.abs(field.astype(np.int64) - ref.astype(np.int64))
        print('    cKDTree query(k = %d, distance_upper_bound, %d workers) at the nodes %.2f s; field values that differ %d of %d, by at most %d (2^-20 nm)'
              % (K, workers, t_query, int((diff > 0).sum()), field.size, int(diff.max())))
ictx.close()
ctx.close()
