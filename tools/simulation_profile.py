"""Times of the SMLM cloud simulator on one GPU (profiles/simulation.txt): generate_smlm_pointcloud_from_shape through a kept
SimulationContext against the NumPy restatement (tests/simulation_ref.py) on the same inputs and against synth.sample_surface for an
equal count -- TwoToruses at the recipe's defaults, ERSim2 at about 10^6 localizations.

    python tools/simulation_profile.py [all | device] [output.json]
        (device: the device path only, for a `rocprofv3 --kernel-trace --stats -- python tools/simulation_profile.py device` run)
"""
import sys, time, json, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import simulation_ref as R
from ch_shrinkwrap_amd import simulation as S, synth

MODE = sys.argv[1] if len(sys.argv) > 1 else 'all'
out = {}
ctx = S.SimulationContext(0)
KW = dict(psf_width=(280.0, 280.0, 840.0), mean_photon_count=600, bg_photon_count=20, noise_fraction=0.1)

def timed(fn, reps, warm=2):
    for _ in range(warm): fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); r = fn(); ts.append(time.perf_counter() - t)
    return r, float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

def ref_pipeline(prog, dx, p, seed):
    t = {}
    t0 = time.perf_counter(); L = R.lattice(prog.ops, prog.centre, prog.r_max + dx, dx, p, seed); t['lattice+project'] = time.perf_counter() - t0
    pts = L['points']; n = pts.shape[0]
    t0 = time.perf_counter(); s0, _ = R.loc_error(n, seed, S.STREAM_PHOTONS, KW['psf_width'], 600, 20); pts = R.displace(pts, s0, seed, S.STREAM_DISPLACE); t['loc_error+displace'] = time.perf_counter() - t0
    t0 = time.perf_counter(); P, sg, cp = R.smlmify(pts, s0, seed, (3, 4, 5), KW['psf_width'], 600, 20); t['smlmify'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ln = int(0.1 * len(P) / 0.9)
    bg = R.background(1.2 * P.min(0), 1.2 * P.max(0), ln, seed, 6); bs, _ = R.loc_error(ln, seed, 7, KW['psf_width'], 600, 20)
    bp, bsg, _ = R.smlmify(bg, bs, seed, (8, 9, 10), KW['psf_width'], 600, 20); P = np.vstack([P, bp]); t['background'] = time.perf_counter() - t0
    t0 = time.perf_counter(); nr = R.normals(prog.ops, P); t['normals'] = time.perf_counter() - t0
    return P, t

# TwoToruses at the recipe's defaults
prog = S.compile_shape('TwoToruses', dict(r=30, R=100))
f = lambda: S.generate_smlm_pointcloud_from_shape(prog, density=1.0, p=0.01, seed=0, context=ctx, **KW)
r, med, lo, hi = timed(f, 20)
out['two_toruses_device'] = dict(n=int(r[0].shape[0]), median_s=med, min_s=lo, max_s=hi)
t0 = time.perf_counter(); P, tt = ref_pipeline(prog, 1.0, 0.01, 0); out['two_toruses_restatement'] = dict(n=int(P.shape[0]), total_s=time.perf_counter() - t0, stages=tt)
assert np.abs(P - r[0]).max() < 1e-9
print(json.dumps(out), flush=True)

# ERSim2 at about 1e6 localizations
prog = S.compile_shape('ERSim2')
ctx.set_program(prog)
n_all = ctx.sample_surface(prog.centre, prog.r_max + 1.0, 1.0, 1.0, project=0).shape[0]
p = min(1.0, 0.9e6 / n_all)
out['er_sim2_fluorophores'] = int(n_all); out['er_sim2_p'] = p
f = lambda: S.generate_smlm_pointcloud_from_shape(prog, density=1.0, p=p, seed=0, context=ctx, **KW)
r, med, lo, hi = timed(f, 7, warm=1)
out['er_sim2_device'] = dict(n=int(r[0].shape[0]), median_s=med, min_s=lo, max_s=hi)
# where the device path's wall time goes: the calls one by one
ctx.set_program(prog)
st = {}
t0 = time.perf_counter(); pts = ctx.sample_surface(prog.centre, prog.r_max + 1.0, 1.0, p, seed=0); st['sample_surface'] = time.perf_counter() - t0
t0 = time.perf_counter(); s0 = ctx.loc_error(pts.shape[0], seed=0, **{k: KW[k] for k in ('psf_width', 'mean_photon_count', 'bg_photon_count')}); st['loc_error'] = time.perf_counter() - t0
t0 = time.perf_counter(); pj = ctx.displace(pts, s0, seed=0); st['displace'] = time.perf_counter() - t0
t0 = time.perf_counter(); P2, sg, cp = ctx.smlmify(pj, s0, seed=0, **{k: KW[k] for k in ('psf_width', 'mean_photon_count', 'bg_photon_count')}); st['smlmify'] = time.perf_counter() - t0
t0 = time.perf_counter(); nr = ctx.normals(P2); st['normals'] = time.perf_counter() - t0
out['er_sim2_device_calls'] = st
print(json.dumps(out), flush=True)
if MODE == 'all':
    t0 = time.perf_counter(); P, tt = ref_pipeline(prog, 1.0, p, 0); out['er_sim2_restatement'] = dict(n=int(P.shape[0]), total_s=time.perf_counter() - t0, stages=tt)
    print('max |device - restatement| = %.3e' % np.abs(P - r[0]).max(), flush=True)
    print(json.dumps(out), flush=True)
    sdf = synth.sdf_er_sim2
    t0 = time.perf_counter(); v, fc = synth.isosurface_mesh(sdf, (-750, -750, -210), (700, 450, 210), 6.0, slack=30.0); t_mesh = time.perf_counter() - t0
    t0 = time.perf_counter(); sp = synth.sample_surface(sdf, v, fc, int(r[0].shape[0]), 10.0, 0, iters=4); t_s = time.perf_counter() - t0
    out['synth_sample_surface'] = dict(n=int(sp.shape[0]), mesh_s=t_mesh, sample_s=t_s)
ctx.close()
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], 'w'), indent=1)
