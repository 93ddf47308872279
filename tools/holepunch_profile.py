"""Hole punching at C3 size on the GPU, eps 50 nm, two scenes:
  sphere  10^6 localizations, a 397 620-face geodesic sphere 40 nm outside them (a bare cap): many candidates, no opposite pairs;
  torus   10^6 localizations on a torus (R 1500, r 300 nm), a 327 680-face flattened sphere around it spanning the hole: ~10^5 candidates
          facing each other across the hole, so steps 2 and 3 do their full work.
Prints the wall time of the grid build, of each of steps 1-3 and of a whole punch_holes call (sphere scene), and the cKDTree time of
step 1 on the same data.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/holepunch_profile.py` for the device times (profiles/holepunch_*)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ch_shrinkwrap_amd import holepunch as H                                  # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import MembraneMesh                      # noqa: E402
from ch_shrinkwrap_amd.trimesh import geodesic_sphere                         # noqa: E402
from ch_shrinkwrap_amd.synth import sphere_cloud                              # noqa: E402

eps = 50.0
pts = sphere_cloud(1000000, 1000.0, 10.0, seed=5).astype(np.float32)
pts = pts[pts[:, 2] < 800.0]
v, f = geodesic_sphere(141, 1040.0)
v = v.astype(np.float32)
m = MembraneMesh(v, f)
nrm = m.face_normals.copy()
ctx = H.HolePunchContext(0)
ms = lambda t0: 1e3 * (time.perf_counter() - t0)
for rep in range(3):
    t0 = time.perf_counter(); ctx.set_points(pts); t_grid = ms(t0)
    t0 = time.perf_counter(); far = ctx.empty_faces(v, f, eps); t1 = ms(t0)
    hc = np.flatnonzero(far).astype('i4')
    t0 = time.perf_counter(); pairs = ctx.pair_faces(v, f, nrm, hc); t2 = ms(t0)
    cands, cp = H.pair_postprocess(hc, pairs)
    t0 = time.perf_counter(); empty = ctx.prism_empty(v, f, nrm, cands, cp, eps); t3 = ms(t0)
    print('sphere rep %d: %d localizations, %d faces, C = %d candidates, %d pairs, %d empty; wall ms: grid %.1f  step1 %.1f  step2 %.1f  step3 %.1f'
          % (rep, len(pts), len(f), len(hc), len(cands), int(empty.sum()), t_grid, t1, t2, t3))
# the torus scene: steps 1-3 with real pairs
rng = np.random.default_rng(3)
u, w = rng.uniform(0, 2 * np.pi, 3000000), rng.uniform(0, 2 * np.pi, 3000000)
keep = rng.uniform(0, 1, u.size) < (1500 + 300 * np.cos(w)) / 1800
u, w = u[keep][:1000000], w[keep][:1000000]
tp = np.stack([(1500 + 300 * np.cos(w)) * np.cos(u), (1500 + 300 * np.cos(w)) * np.sin(u), 300 * np.sin(w)], 1)
tp = (tp + rng.normal(0, 10, tp.shape)).astype(np.float32)
from ch_shrinkwrap_amd.trimesh import icosphere                               # noqa: E402
tv, tf = icosphere(7, 1.0)
tv = (tv.astype('f8') * np.array([2000.0, 2000.0, 420.0])).astype(np.float32)
tn = MembraneMesh(tv, tf).face_normals.copy()
for rep in range(3):
    t0 = time.perf_counter(); ctx.set_points(tp); t_grid = ms(t0)
    t0 = time.perf_counter(); far = ctx.empty_faces(tv, tf, eps); t1 = ms(t0)
    hc = np.flatnonzero(far).astype('i4')
    t0 = time.perf_counter(); pairs = ctx.pair_faces(tv, tf, tn, hc); t2 = ms(t0)
    cands, cp = H.pair_postprocess(hc, pairs)
    t0 = time.perf_counter(); empty = ctx.prism_empty(tv, tf, tn, cands, cp, eps); t3 = ms(t0)
    print('torus rep %d: %d localizations, %d faces, C = %d candidates, %d pairs, %d empty; wall ms: grid %.1f  step1 %.1f  step2 %.1f  step3 %.1f'
          % (rep, len(tp), len(tf), len(hc), len(cands), int(empty.sum()), t_grid, t1, t2, t3))
for rep in range(2):
    mm = MembraneMesh(v, f)
    t0 = time.perf_counter(); mm.punch_holes(pts, eps); t = ms(t0)
    print('punch_holes (grid included): %.1f ms; log %s' % (t, {k: mm.punch_log[-1][k] for k in ('candidates', 'pairs', 'kept_pairs', 'components', 'holes')}))
if os.environ.get('HP_KDTREE', '1') == '1':
    from scipy.spatial import cKDTree
    t0 = time.perf_counter(); tree = cKDTree(pts); tb = ms(t0)
    t0 = time.perf_counter(); tree.query(v[f].mean(1), workers=1); tq = ms(t0)
    print('cKDTree step 1 on the same data: build %.0f ms, query %.0f ms (one thread)' % (tb, tq))
