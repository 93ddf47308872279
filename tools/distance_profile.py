"""Wall time of the distance from localizations to a fitted mesh through a kept context, and where the queries' walks end
(profiles/distance_c3.txt): config C3's mesh after a short fit against its 10^6 localizations.
usage: python tools/distance_profile.py [config] [scale] [iterations]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/distance_profile.py     (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, distance as D
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane

name = sys.argv[1] if len(sys.argv) > 1 else 'c3'
scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
cfg = synth.make_config(name, scale=scale, seed=0)
pts = np.ascontiguousarray(cfg['points'], np.float64)
table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
surf = type('Surf', (), {'vertices': cfg['vertices'], 'faces': cfg['faces']})
mesh = ShrinkwrapMembrane(max_iters=iters, remesher=None).execute({'surf': surf, 'filtered_localizations': table})
pos, faces, twin = D._mesh_arrays(mesh, True)
print('%s x%g after %d iterations: %d vertices, %d faces, %d localizations' % (name, scale, iters, pos.shape[0], faces.shape[0], pts.shape[0]))

t0 = time.perf_counter()
ctx = D.DistanceContext()
ctx.set_mesh(pos, faces, twin)
first_set = time.perf_counter() - t0
t0 = time.perf_counter()
dist = ctx.query(pts)
first_query = time.perf_counter() - t0
sets, queries, unsigned = [], [], []
for _ in range(5):
    t0 = time.perf_counter()
    ctx.set_mesh(pos, faces, twin)
    sets.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    again = ctx.query(pts)
    queries.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ctx.query(pts, signed=False)
    unsigned.append(time.perf_counter() - t0)
    assert again.tobytes() == dist.tobytes()
_, feature = ctx.query(pts, return_feature=True, rings=True)
ctx.close()
ms = lambda a: ' '.join('%.1f' % (1e3 * x) for x in a)
print('wall: first set_mesh (context, allocations, upload) %.1f ms, first query %.1f ms' % (1e3 * first_set, 1e3 * first_query))
print('wall: set_mesh %s ms (min %.1f); signed query of %d points %s ms (min %.1f, %.1f ns a point); unsigned %s ms (min %.1f)'
      % (ms(sets), 1e3 * min(sets), pts.shape[0], ms(queries), 1e3 * min(queries), 1e9 * min(queries) / pts.shape[0], ms(unsigned), 1e3 * min(unsigned)))
ring = feature >> 8
code = feature & D.FEATURE_MASK
print('walks end in ring 0: %.2f %%, ring 1: %.2f %%, ring 2: %.2f %%, beyond: %.2f %% (max %d)'
      % (tuple(100.0 * np.mean(c) for c in (ring == 0, ring == 1, ring == 2, ring > 2)) + (int(ring.max()),)))
print('closest feature: interior %.1f %%, edge %.1f %%, vertex %.1f %%; fan walks cut short: %d'
      % (100.0 * np.mean(code == 0), 100.0 * np.mean((code >= 1) & (code <= 3)), 100.0 * np.mean(code >= 4), int(((feature & D.FEATURE_CAPPED) != 0).sum())))
print('signed distance quantiles 1/5/25/50/75/95/99 %%: %s nm; %.1f %% inside' % (np.round(np.percentile(dist, [1, 5, 25, 50, 75, 95, 99]), 2), 100.0 * (dist < 0).mean()))
