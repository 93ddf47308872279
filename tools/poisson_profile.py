"""Wall time of the screened Poisson grid solver on a simulated cloud with the generator's normals, through a kept context -- set_samples,
plan, every level's level_begin (splat, system, prolongation) and relax, field, and the surface nets on the field -- the relaxation's bytes
per second next to a device-to-device copy measured in the same process, and the NumPy restatement's time on the same host
(profiles/poisson.txt).
usage: python tools/poisson_profile.py [c3 | c4] [depth] [scale] [host: 0 | 1]
       the scene: the config's localizations (c3: 10^6, c4: 5 10^6 at scale 1) with the normalised gradient of the config's signed distance
       as normals; fulldepth = depth, so that the solve ends at the depth asked; defaults c3 8 1.0 0
       host 1: tests/screened_poisson_ref.py on the same samples at depth 5, 6, ... until one solve takes more than a minute
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/poisson_profile.py c3 8
                                                                       (device time per kernel, a run of its own)
The relaxation's traffic is counted by whole lines: a colour of a sweep reads chi, rhs and diag of every node (the other colour's half of
a line comes with it) and writes half of chi: 3.5 arrays of 8 bytes a node, 56 bytes a node and sweep."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ch_shrinkwrap_amd import synth, poisson as C, isosurface

ms = lambda a: ' '.join('%.2f' % (1e3 * x) for x in a)
SWEEP_BYTES = 56


def say(*a):
    print(*a)
    sys.stdout.flush()


def timed(fn, repeats=3):
    out, ts = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def sdf_normals(sdf, P, eps=0.05):
    """the normalised central-difference gradient of the generator's signed distance, in float64 on the host"""
    P = P.astype(np.float64)
    g = np.empty_like(P)
    for d in range(3):
        e = np.zeros(3)
        e[d] = eps
        g[:, d] = np.asarray(sdf(P + e), np.float64) - np.asarray(sdf(P - e), np.float64)
    return (g / np.maximum(np.linalg.norm(g, axis=1), 1e-300)[:, None]).astype(np.float32)


def copy_ceiling(n_bytes=1 << 30):
    import torch
    a = torch.empty(n_bytes // 8, dtype=torch.float64, device='cuda')
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * n_bytes / min(ts)


def main(name='c3', depth=8, scale=1.0, with_host=0):
    cfg = synth.make_config(name, scale=scale, seed=0)
    P = np.ascontiguousarray(cfg['points'], np.float32)
    t0 = time.perf_counter()
    N = sdf_normals(cfg['sdf'], P)
    say('%s x%g: %d localizations, normals from the generator\'s signed distance in %.1f s; depth %d, fulldepth %d, pointweight 4, iters 8'
        % (name, scale, len(P), time.perf_counter() - t0, depth, depth))
    try:
        from ch_shrinkwrap_amd import build
        for k, res in sorted(build.kernel_resources(build.OBJ_POISSON).items()):
            say('  %-16s %3d VGPRs %5d B LDS scratch %d' % (k, res['vgpr'], res['lds'], res['scratch']))
    except Exception:
        say('  (no object file here: the kernels\' registers are read where the library is built)')
    lo, h = C.cube_for(P, depth)
    t0 = time.perf_counter()
    ctx = C.PoissonContext()
    ctx.set_samples(P, N)
    say('wall: first set_samples (context, allocations, upload, normals) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, ts = timed(lambda: ctx.set_samples(P, N))
    say('wall: set_samples %s ms' % ms(ts))
    (used, occ), ts = timed(lambda: ctx.plan(lo, h, depth, depth, 1.5))
    say('wall: plan (the occupancy of levels 2..%d) %s ms; occ %s' % (depth, ms(ts), occ))
    alpha = ctx.alpha(4.0)
    ctx.solve(4.0, 8, 64)                                             # allocations
    ceiling = copy_ceiling()
    say('device-to-device copy of 1 GiB (torch, read + write): %.0f GB/s' % (ceiling / 1e9))
    for l in range(2, used + 1):
        t0 = time.perf_counter()
        ctx.level_begin(l, alpha)
        t1 = time.perf_counter()
        before, _ = ctx.relax(0)
        t2 = time.perf_counter()
        sweeps = 64 if l == 2 else 8
        _, after = ctx.relax(sweeps)
        t3 = time.perf_counter()
        dt = max((t3 - t2) - (t2 - t1), 1e-9)
        nodes = 8 ** l
        say('  level %d (%4d^3): level_begin %8.2f ms, two residuals %7.2f ms, %2d sweeps %8.2f ms = %6.1f GB/s by whole lines (%.0f %% of the copy), residual %.3g -> %.3g'
            % (l, 1 << l, 1e3 * (t1 - t0), 1e3 * (t2 - t1), sweeps, 1e3 * dt, SWEEP_BYTES * nodes * sweeps / dt / 1e9,
               100.0 * SWEEP_BYTES * nodes * sweeps / dt / ceiling, before, after))
    fld, ts = timed(lambda: ctx.field())
    say('wall: field (largest |chi|, F, the level) %s ms; thr %d, E %g' % (ms(ts), fld['thr'], fld['E']))
    (_, res), ts = timed(lambda: ctx.solve(4.0, 8, 64))
    say('wall: solve, all levels %s ms (min %.1f)' % (ms(ts), 1e3 * min(ts)))
    ctx.field()
    ictx = isosurface.IsosurfaceContext()
    n = 1 << used
    t0 = time.perf_counter()
    ictx.set_field(ctx.field_pointer(), lo, ctx.h_used, (n, n, n))
    try:
        v, f = ictx.extract(fld['thr'])
        say('wall: surface nets on the field %.1f ms: %d vertices, %d faces' % (1e3 * (time.perf_counter() - t0), len(v), len(f)))
    except RuntimeError as e:
        say('surface nets: %s' % e)
    ictx.close()
    ctx.close()
    t0 = time.perf_counter()
    try:
        v, f, info = C.screened_poisson(P, N, depth=depth, return_info=True)
        say('wall: screened_poisson(depth=%d) with upstream\'s defaults, one call: %.1f ms; depth used %d, h %.2f nm, %d faces'
            % (depth, 1e3 * (time.perf_counter() - t0), info['depth_used'], info['h'], len(f)))
    except RuntimeError as e:
        say('screened_poisson: %s' % e)
    if with_host:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import screened_poisson_ref as R
        for d in range(5, depth + 1):
            lo_d, h_d = R.cube_for(P, d)
            t0 = time.perf_counter()
            R.solve(P, N, lo_d, h_d, d, fulldepth=d, keep_levels=False)
            dt = time.perf_counter() - t0
            say('restatement (NumPy, this host): depth %d in %.1f s' % (d, dt))
            if dt > 60.0:
                break


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if len(a) > 0 else 'c3', int(a[1]) if len(a) > 1 else 8, float(a[2]) if len(a) > 2 else 1.0, int(a[3]) if len(a) > 3 else 0)
