"""Neck removal / short-edge cleanup on the GPU, two parts:
  queries  the four entry points of include/nw_surgery.h at C3 size: a 397 620-face geodesic sphere (radius 1000 nm) plus a 5 120-face
           sphere inside it; labelling of all faces and of a random 30 % of them, component statistics, winding numbers of 512 queries,
           the short-edge selection -- wall times of 3 calls each (the device times come from rocprofv3);
  fit      examples/fit_network.py 0.2 (the ERSim2 network, 10^6 localizations) with neck_remover='device' and edge_cleaner='device':
           candidates, regions and cuts of every neck boundary and the wall time of every remove_necks / remove_extra_short_edges call
           and of the selection inside it; then, on the fitted mesh, one remove_necks with the guard (no cut) and one without (every
           candidate cut), and the same fit without the hooks.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/surgery_profile.py` for the device times (profiles/surgery_c3.txt)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ch_shrinkwrap_amd import surgery as S                                    # noqa: E402
from ch_shrinkwrap_amd import synth                                           # noqa: E402
from ch_shrinkwrap_amd.membrane_mesh import MembraneMesh, ShrinkwrapMembrane  # noqa: E402
from ch_shrinkwrap_amd.trimesh import geodesic_sphere, icosphere              # noqa: E402

ms = lambda t0: 1e3 * (time.perf_counter() - t0)

# ---- the four queries at C3 size --------------------------------------------------------------------------------------------------
v0, f0 = geodesic_sphere(141, 1000.0)
v1, f1 = icosphere(5, 300.0)
v = np.vstack([v0, v1]).astype(np.float32)
f = np.vstack([f0, f1 + v0.shape[0]]).astype(np.int32)
tw = S.twins(f, v.shape[0])
ctx = S.SurgeryContext(0)
mask = (np.random.default_rng(0).random(f.shape[0]) < 0.3).astype(np.uint8)
rng = np.random.default_rng(1)
q = (rng.normal(size=(512, 3)) * 200.0).astype(np.float32)
print('C3-size mesh: %d vertices, %d faces' % (v.shape[0], f.shape[0]))
for rep in range(3):
    t0 = time.perf_counter(); lab, n = ctx.label_faces(f, tw); t1 = ms(t0)
    t0 = time.perf_counter(); labm, nm = ctx.label_faces(f, tw, mask); t2 = ms(t0)
    t0 = time.perf_counter(); st = ctx.component_stats(v, f, tw, lab, n); t3 = ms(t0)
    t0 = time.perf_counter(); w = ctx.winding(v, f, lab, n, q); t4 = ms(t0)
    t0 = time.perf_counter(); flags, med = ctx.short_edge_vertices(v, f, 0.05); t5 = ms(t0)
    print('rep %d wall ms: label %.2f (%d components)  label 30%% mask %.2f (%d)  stats %.2f  winding 512 %.2f  short edges %.2f (median %.3f, %d flagged)'
          % (rep, t1, n, t2, nm, t3, t4, t5, med, flags.sum()))

# ---- one fit: examples/fit_network.py 0.2 with the hooks on --------------------------------------------------------------------------
scale = 0.2
cfg = synth.make_config('c4', scale=scale, seed=0)
pts = cfg['points']
timings = []
orig_necks, orig_edges, orig_select = MembraneMesh.remove_necks, MembraneMesh.remove_extra_short_edges, MembraneMesh.neck_vertices


def timed(name, fn):
    def run(self, *a, **k):
        t0 = time.perf_counter()
        out = fn(self, *a, **k)
        timings.append((name, getattr(self, '_neck_iteration', None) or getattr(self, '_edge_iteration', None), ms(t0), int(self.faces.shape[0])))
        return out
    return run


def fit(**hooks):
    class Surf(object):
        vertices, faces = cfg['vertices'], cfg['faces']
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2],
             'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    mod = ShrinkwrapMembrane(max_iters=39, remesh_frequency=5, curvature_weight=20.0, minimum_edge_length=max(5.0, 2.5 / np.sqrt(scale)),
                             neck_first_iter=9, remesher='device', **hooks)
    t0 = time.perf_counter()
    mesh = mod.execute({'surf': Surf, 'filtered_localizations': table})
    return mesh, ms(t0)


MembraneMesh.remove_necks = timed('remove_necks', orig_necks)
MembraneMesh.remove_extra_short_edges = timed('remove_extra_short_edges', orig_edges)
MembraneMesh.neck_vertices = timed('  selection (neck_vertices)', orig_select)
mesh, t_fit = fit(neck_remover='device', edge_cleaner='device')
print('fit_network %g with neck_remover / edge_cleaner = device: %d localizations, fitted mesh %d vertices / %d faces, %.0f ms'
      % (scale, pts.shape[0], mesh.vertices.shape[0], mesh.faces.shape[0], t_fit))
for r in mesh.neck_log:
    print('  neck iteration %s: %d candidates, %d regions, %d disks, %d examined, %d cut, skips %s' %
          (r['iteration'], r['candidates'], r['regions'], r['disks'], r['examined'], r['cut'], [s[1] for s in r['skips']][:3]))
for r in mesh.edge_log:
    print('  short edges iteration %s: median %.3f nm, %d vertices flagged' % (r['iteration'], r['median'], r['vertices']))
for name, it, t, nf in timings:
    print('  %-28s iteration %s: %.1f ms (%d faces after)' % (name, it, t, nf))
timings.clear()
MembraneMesh.remove_necks, MembraneMesh.remove_extra_short_edges, MembraneMesh.neck_vertices = orig_necks, orig_edges, orig_select

# ---- the fitted mesh, one boundary each way --------------------------------------------------------------------------------------------
vv, ff = np.array(mesh.vertices), np.array(mesh.faces)
for guard in (True, False):
    m = MembraneMesh(vv, ff, neck_remover='device', neck_guard=guard, remesher='device')
    m.neck_vertices(-1e-3, 1e-2)                       # (the curvature kernel's context warmed up)
    t0 = time.perf_counter(); m.neck_vertices(-1e-3, 1e-2); t_sel = ms(t0)
    m = MembraneMesh(vv, ff, neck_remover='device', neck_guard=guard, remesher='device')
    m.neck_vertices(-1e-3, 1e-2)
    t0 = time.perf_counter(); m.remove_necks(-1e-3, 1e-2); t = ms(t0)
    r = m.neck_log[-1]
    print('fitted mesh, remove_necks guard=%s: %.1f ms (selection alone %.1f ms); %d candidates, %d regions, %d cut, components %s -> %s, %d faces after'
          % (guard, t, t_sel, r['candidates'], r['regions'], r['cut'], r['components_before'], r['components_after'], m.faces.shape[0]))
m = MembraneMesh(vv, ff, remesher='device')
for rep in range(2):
    t0 = time.perf_counter(); m.remove_extra_short_edges(); t = ms(t0)
    print('fitted mesh, remove_extra_short_edges: %.1f ms, %s' % (t, m.edge_log[-1]))
plain, t_plain = fit()
print('the same fit without the hooks: %.0f ms, %d vertices' % (t_plain, plain.vertices.shape[0]))
