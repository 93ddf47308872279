"""Wall time of the self-intersection check through a kept context, and the share of candidate pairs that reach the predicate
(profiles/intersections.txt): config C3's mesh after a short fit.
usage: python tools/intersections_profile.py [config] [scale] [iterations]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/intersections_profile.py     (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, intersections as X
from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane

name = sys.argv[1] if len(sys.argv) > 1 else 'c3'
scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
cfg = synth.make_config(name, scale=scale, seed=0)
pts = np.ascontiguousarray(cfg['points'], np.float64)
table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
surf = type('Surf', (), {'vertices': cfg['vertices'], 'faces': cfg['faces']})
mesh = ShrinkwrapMembrane(max_iters=iters, remesher=None).execute({'surf': surf, 'filtered_localizations': table})
pos, faces = X._mesh_arrays(mesh)
print('%s x%g after %d iterations: %d vertices, %d faces' % (name, scale, iters, pos.shape[0], faces.shape[0]))

t0 = time.perf_counter()
ctx = X.IntersectionContext()
ctx.set_mesh(pos, faces)
first_set = time.perf_counter() - t0
t0 = time.perf_counter()
first = ctx.find()
first_find = time.perf_counter() - t0
sets, finds, counts_only = [], [], []
for _ in range(5):
    t0 = time.perf_counter()
    ctx.set_mesh(pos, faces)
    sets.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    again = ctx.find()
    finds.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ctx.find(return_pairs=False)
    counts_only.append(time.perf_counter() - t0)
    assert again['count'].tobytes() == first['count'].tobytes() and again['pairs'].tobytes() == first['pairs'].tobytes()
st = ctx.find(stats=True)
ctx.close()
ms = lambda a: ' '.join('%.1f' % (1e3 * x) for x in a)
nf = faces.shape[0]
print('wall: first set_mesh (context, allocations, upload) %.1f ms, first find %.1f ms' % (1e3 * first_set, 1e3 * first_find))
print('wall: set_mesh %s ms (min %.1f); find with the pair list %s ms (min %.1f, %.1f ns a face); counts only %s ms (min %.1f)'
      % (ms(sets), 1e3 * min(sets), ms(finds), 1e3 * min(finds), 1e9 * min(finds) / nf, ms(counts_only), 1e3 * min(counts_only)))
print('crossing pairs: %d, faces in one: %d' % (first['n_pairs'], first['n_faces']))
print('candidates read: %d (%.1f a face); reached the predicate: %d (%.1f a face, %.2f %% of the candidates)'
      % (st['candidates'], st['candidates'] / nf, st['tested'], st['tested'] / nf, 100.0 * st['tested'] / max(st['candidates'], 1)))
