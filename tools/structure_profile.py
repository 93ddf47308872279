"""Wall time of the local shape on a simulated cloud through a kept context -- set_cloud, and query with and without the moments brought
back --, the neighbours, distance tests and cells read per query, and the host route on the same machine and the same input as the
baseline: scipy's cKDTree.query_ball_point, float64 moments and np.linalg.eigh (profiles/structure.txt).
usage: python tools/structure_profile.py [c3 | c4] [scale] [r] [host: 0 | 1] [host_queries]
       the scene: the config's localizations (c3: 10^6, c4: 5 10^6 at scale 1), auto mode; defaults c3 1.0 30 0 20000
       host 1: the host route on the first `host_queries` points as queries against the whole cloud (a subsample: the whole of it takes
       minutes), neighbour counts checked for equality with the device's (a mismatch is printed, not raised) and the time scaled to the
       whole cloud
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/structure_profile.py c3 1.0
                                                                       (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, structure as C

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


def main(name='c3', scale=1.0, r=30.0, with_host=0, host_queries=20000):
    P = np.ascontiguousarray(synth.make_config(name, scale=scale, seed=0)['points'], np.float32)
    n = len(P)
    say('%s x%g: %d localizations; r %g nm, auto mode' % (name, scale, n, r))
    try:
        from ch_shrinkwrap_amd import build
        for k, res in sorted(build.kernel_resources(build.OBJ_STRUCTURE).items()):
            say('  %-18s %3d VGPRs %5d B LDS scratch %d' % (k, res['vgpr'], res['lds'], res['scratch']))
    except Exception:
        say('  (no object file here: the kernels\' registers are read where the library is built)')
    t0 = time.perf_counter()
    ctx = C.StructureContext()
    ctx.set_cloud(P)
    say('wall: first set_cloud (context, allocations, upload, bounding box) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, ts = timed(lambda: ctx.set_cloud(P))
    say('wall: set_cloud %s ms (min %.1f)' % (ms(ts), 1e3 * min(ts)))
    t0 = time.perf_counter()
    ctx.query(r, moments=False, shape=False)
    say('wall: first query (the grid is built in it) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    for label, kw in (('nothing brought back (info alone)', dict(moments=False, shape=False)), ('eigenvalues, vectors, flags', dict(moments=False)),
                      ('moments as well', dict())):
        out, ts = timed(lambda: ctx.query(r, **kw))
        say('wall: query, %s: %s ms (min %.1f, %.1f ns a point)' % (label, ms(ts), 1e3 * min(ts), 1e9 * min(ts) / n))
    i = out['info']
    say('  neighbours a query: %.1f; distance tests a query: %.1f; cells read a query: %.1f; cell %.3f nm, %d cells; queries with n < 3: %d'
        % (i['neighbours'] / n, i['tests'] / n, i['cells_read'] / n, i['cell_size'], i['cells'], i['few']))
    F = C.shape_features(out['moments'], out['eigenvalues'], out['flags'], r)
    cls = np.where(F['valid'], np.argmax(np.nan_to_num(np.stack([F['linearity'], F['planarity'], F['scattering']], 1)), 1), -1)
    say('  classes: line %.3f, plane %.3f, blob %.3f, not valid %.3f' % tuple(float((cls == c).mean()) for c in (0, 1, 2, -1)))
    ctx.close()
    if with_host:
        from scipy.spatial import cKDTree
        P64 = P.astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(P64)
        say('host baseline: cKDTree build %.1f ms' % (1e3 * (time.perf_counter() - t0)))
        nq = min(int(host_queries), n)
        t0 = time.perf_counter()
        nb = tree.query_ball_point(P64[:nq], r)
        t1 = time.perf_counter()
        cnt = np.array([len(b) for b in nb], np.int64)
        row = np.repeat(np.arange(nq), cnt)
        e = P64[np.concatenate(nb)] - P64[row]
        S1 = np.zeros((nq, 3))
        S2 = np.zeros((nq, 3, 3))
        np.add.at(S1, row, e)
        np.add.at(S2, row, e[:, :, None] * e[:, None, :])
        m = S1 / cnt[:, None]
        cov = S2 / cnt[:, None, None] - m[:, :, None] * m[:, None, :]
        t2 = time.perf_counter()
        w, v = np.linalg.eigh(cov)
        t3 = time.perf_counter()
        say('host baseline, the first %d points as queries (a subsample): query_ball_point %.1f ms, moments (np.add.at) %.1f ms, np.linalg.eigh %.1f ms; '
            'scaled to %d queries: %.1f s' % (nq, 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), n, (t3 - t0) * n / nq))
        mine = out['moments'][:nq, 0]
        say('  neighbour counts equal on %d of %d queries (the host roots no distance but compares float64 |e| with r: a pair within an ulp of r '
            'may differ); largest eigenvalue: max relative difference %.2e'
            % (int((mine == cnt).sum()), nq, float(np.nanmax(np.abs(w[:, 2] - out['eigenvalues'][:nq, 0]) / out['eigenvalues'][:nq, 0]))))


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if len(a) > 0 else 'c3', float(a[1]) if len(a) > 1 else 1.0, float(a[2]) if len(a) > 2 else 30.0, int(a[3]) if len(a) > 3 else 0,
         int(a[4]) if len(a) > 4 else 20000)
