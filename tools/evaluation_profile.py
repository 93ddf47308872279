"""Wall time of evaluation.fit_quality on the host and on the device, on one input: the C3 start mesh against synth.truth_cloud, dx 5
(profiles/evaluation_c3.txt).
usage: python tools/evaluation_profile.py [both | device] [config] [scale]
       rocprofv3 --kernel-trace --stats -d DIR -- python tools/evaluation_profile.py device     (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, evaluation as E

what = sys.argv[1] if len(sys.argv) > 1 else 'both'
name = sys.argv[2] if len(sys.argv) > 2 else 'c3'
scale = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
cfg = synth.make_config(name, scale=scale, seed=0)
truth = synth.truth_cloud(cfg)
mesh = type('M', (), {'_vertices': {'position': np.ascontiguousarray(cfg['vertices'], np.float32)}, 'faces': cfg['faces']})()
print('%s x%g: %d vertices, %d faces, %d truth points, dx 5' % (name, scale, cfg['vertices'].shape[0], cfg['faces'].shape[0], truth.shape[0]))

t0 = time.perf_counter()
ctx = E.EvaluationContext()
q = E.fit_quality(mesh, truth, backend='device', context=ctx)
first = time.perf_counter() - t0
calls = []
for _ in range(5):
    t0 = time.perf_counter()
    q = E.fit_quality(mesh, truth, backend='device', context=ctx)
    calls.append(time.perf_counter() - t0)
t0 = time.perf_counter()
n = ctx.sample_mesh(mesh._vertices['position'], mesh.faces, 5.0)
t_sample = time.perf_counter() - t0
t0 = time.perf_counter()
ctx.average_squared_distance(E.SAMPLES, np.asarray(truth, np.float64))
t_asd = time.perf_counter() - t0
ctx.close()
print('device: %s' % q)
print('device wall: first call (context, allocations) %.1f ms; then %s ms (min %.1f); sample_mesh alone %.1f ms, average_squared_distance alone %.1f ms'
      % (1e3 * first, ' '.join('%.1f' % (1e3 * c) for c in calls), 1e3 * min(calls), 1e3 * t_sample, 1e3 * t_asd))
if what == 'both':
    t0 = time.perf_counter()
    m = E.points_from_mesh(mesh, dx_min=5.0)
    t_pts = time.perf_counter() - t0
    t0 = time.perf_counter()
    E.average_squared_distance(m, np.asarray(truth, m.dtype))
    t_nn = time.perf_counter() - t0
    t0 = time.perf_counter()
    h = E.fit_quality(mesh, truth)
    t_host = time.perf_counter() - t0
    print('host:   %s' % h)
    print('host wall: fit_quality %.1f ms (points_from_mesh %.1f ms, average_squared_distance %.1f ms)' % (1e3 * t_host, 1e3 * t_pts, 1e3 * t_nn))
    print('ratio host / device: %.1f' % (t_host / min(calls)))
    for k in ('mse01', 'mse10', 'mse_rms'):
        assert np.isclose(q[k], h[k], rtol=1e-9, atol=0), (k, q[k], h[k])
    assert q['n_mesh_points'] == h['n_mesh_points']
