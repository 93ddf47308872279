"""Wall time of DBSCAN on a simulated cloud with background through a kept context, the counters of the walk with and without the two
shortcuts, and scikit-learn's DBSCAN on the same host and the same input as the baseline (profiles/clustering.txt).
usage: python tools/clustering_profile.py [c3 | c4] [scale] [eps] [min_points] [sklearn: 0 | 1]
       the scene: the config's localizations (c3: 10^6, c4: 5 10^6 at scale 1) plus 10 % uniform background from SimulationContext.background
       in the cloud's box scaled by 1.2; defaults c3 1.0 15 10 0
       sklearn 1: sklearn.cluster.DBSCAN(n_jobs=16) on the float64 copy, its core mask and core partition checked for equality (it keeps
       every neighbour list in memory: pick a scale it can hold)
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/clustering_profile.py c3 1.0
                                                                       (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, clustering as C

ms = lambda a: ' '.join('%.1f' % (1e3 * x) for x in a)


def say(*a):
    print(*a)
    sys.stdout.flush()


def timed(fn, repeats=5):
    out, ts = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts


def scene(name, scale):
    from ch_shrinkwrap_amd.simulation import SimulationContext
    pts = np.ascontiguousarray(synth.make_config(name, scale=scale, seed=0)['points'], np.float64)
    lo, hi = pts.min(0), pts.max(0)
    c, half = 0.5 * (lo + hi), 0.6 * (hi - lo)
    sim = SimulationContext()
    bg = sim.background(c - half, c + half, len(pts) // 10, seed=1)
    sim.close()
    return np.ascontiguousarray(np.concatenate([pts, bg]), np.float32), len(pts)


def same_partition(a, b, mask):
    """whether two labellings split the points of `mask` into the same sets"""
    a, b = np.asarray(a)[mask], np.asarray(b)[mask]
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


def main(name='c3', scale=1.0, eps=15.0, min_points=10, with_sklearn=0):
    P, n_structure = scene(name, scale)
    n = len(P)
    say('%s x%g: %d localizations and %d background points; eps %g nm, min_points %d' % (name, scale, n_structure, n - n_structure, eps, min_points))
    try:
        from ch_shrinkwrap_amd import build
        for k, r in sorted(build.kernel_resources(build.OBJ_CLUSTERING).items()):
            say('  %-16s %3d VGPRs %4d B LDS scratch %d' % (k, r['vgpr'], r['lds'], r['scratch']))
    except Exception:
        say('  (no object file here: the kernels\' registers are read where the library is built)')
    t0 = time.perf_counter()
    ctx = C.ClusterContext()
    ctx.set_cloud(P)
    say('wall: first set_cloud (context, allocations, upload, bounding box) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, ts = timed(lambda: ctx.set_cloud(P))
    say('wall: set_cloud %s ms (min %.1f)' % (ms(ts), 1e3 * min(ts)))
    t0 = time.perf_counter()
    ctx.dbscan(eps, min_points)
    say('wall: first dbscan (binning at this eps, allocations) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    results = {}
    for label, cap in (('count_cap = min_points', None), ('full counts', n)):
        for on in (True, False):
            ctx.set_shortcuts(on)
            r, ts = timed(lambda: ctx.dbscan(eps, min_points, cap))
            i = r['info']
            results[(label, on)] = r
            say('wall: dbscan, %s, shortcuts %s: %s ms (min %.1f, %.1f ns a point)' % (label, 'on' if on else 'off', ms(ts), 1e3 * min(ts), 1e9 * min(ts) / n))
            say('  distance tests a point: %.1f (count %.1f, unions %.1f, border %.1f); settled by (a): %.2f %% of the points; joined by (b): %d; guard %d'
                % (i['tests'] / n, i['tests_count'] / n, i['tests_hook'] / n, (i['tests'] - i['tests_count'] - i['tests_hook']) / n, 100.0 * i['shortcut_a'] / n,
                   i['shortcut_b'], i['guard']))
    ctx.set_shortcuts(True)
    r = results[('count_cap = min_points', True)]
    i = r['info']
    say('cell %.3f nm, %d cells; %d core, %d border, %d noise, %d clusters; the five largest: %s'
        % (i['cell_size'], i['cells'], i['n_core'], i['n_border'], i['n_noise'], i['n_clusters'], np.sort(ctx.stats()['sizes'])[::-1][:5].tolist()))
    bg_kept = int((r['labels'][n_structure:] >= 0).sum())
    say('  structure lost to noise: %d of %d; background kept: %d of %d' % (int((r['labels'][:n_structure] < 0).sum()), n_structure, bg_kept, n - n_structure))
    for k in ('labels', 'anchor', 'core'):
        assert np.array_equal(r[k], results[('count_cap = min_points', False)][k]) and np.array_equal(r[k], results[('full counts', True)][k]), k
    ctx.close()
    if with_sklearn:
        from sklearn.cluster import DBSCAN
        P64 = P.astype(np.float64)
        sk, ts = timed(lambda: DBSCAN(eps=eps, min_samples=min_points, n_jobs=16).fit(P64), repeats=2)
        core = np.zeros(n, bool)
        core[sk.core_sample_indices_] = True
        say('host baseline: sklearn.cluster.DBSCAN(n_jobs=16) %s ms' % ms(ts))
        say('  core mask equal: %s (%d against %d); core partition equal: %s; noise set equal: %s'
            % (np.array_equal(core, r['core']), core.sum(), r['core'].sum(), same_partition(sk.labels_, r['labels'], core & r['core']),
               np.array_equal(sk.labels_ < 0, r['labels'] < 0)))


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if len(a) > 0 else 'c3', float(a[1]) if len(a) > 1 else 1.0, float(a[2]) if len(a) > 2 else 15.0, int(a[3]) if len(a) > 3 else 10,
         int(a[4]) if len(a) > 4 else 0)
