"""Wall time of the pair counts on a simulated cloud through a kept context -- 16 and 64 bins, with and without the per-point counts --,
the distance tests and cells read per query, a sweep of the starting cell size (NWQ_CELL_OF_RMAX), and scipy's
cKDTree.count_neighbors on the same host and the same input as the baseline (profiles/pairs.txt).
usage: python tools/pairs_profile.py [c3 | c4] [scale] [r_max] [ckdtree: 0 | 1] [sweep: 0 | 1]
       the scene: the config's localizations (c3: 10^6, c4: 5 10^6 at scale 1); defaults c3 1.0 30 0 1
       ckdtree 1: cKDTree(points).count_neighbors(itself, radii) on the float64 copy, cumulative counts checked for equality where no pair
       sits within 1e-9 of an edge (it is not checked here: a mismatch is printed, not raised)
       sweep 1: a fresh context per starting cell size, through the developer knob NW_PAIRS_CELL_OF_RMAX (no output depends on it)
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pairs_profile.py c3 1.0
                                                                       (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, pairs as C

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


def measure(ctx, n, m, r_max, label=''):
    ctx.set_edges(np.linspace(r_max / m, r_max, m))
    t0 = time.perf_counter()
    ctx.count()
    first = time.perf_counter() - t0
    out = {}
    for local in (False, True):
        r, ts = timed(lambda: ctx.count(local=local))
        out[local] = r
        i = r['info']
        say('wall: %s%d bins (%s), local %s: %s ms (min %.1f, %.1f ns a point; first call %.1f)'
            % (label, m, i['variant'], 'on ' if local else 'off', ms(ts), 1e3 * min(ts), 1e9 * min(ts) / n, 1e3 * first))
    i = out[True]['info']
    say('  distance tests a query: %.1f, of which counted: %.1f; cells read a query: %.1f; cell %.3f nm, %d cells'
        % (i['tests'] / n, float(out[True]['hist'].sum()) / n, i['cells_read'] / n, i['cell_size'], i['cells']))
    assert np.array_equal(out[True]['hist'], out[False]['hist']) and np.array_equal(out[True]['local'].sum(0, dtype=np.uint64), out[True]['hist'])
    return out[True]


def main(name='c3', scale=1.0, r_max=30.0, with_ckdtree=0, sweep=1):
    P = np.ascontiguousarray(synth.make_config(name, scale=scale, seed=0)['points'], np.float32)
    n = len(P)
    say('%s x%g: %d localizations; r_max %g nm' % (name, scale, n, r_max))
    try:
        from ch_shrinkwrap_amd import build
        for k, r in sorted(build.kernel_resources(build.OBJ_PAIRS).items()):
            say('  %-18s %3d VGPRs %5d B LDS scratch %d' % (k, r['vgpr'], r['lds'], r['scratch']))
    except Exception:
        say('  (no object file here: the kernels\' registers are read where the library is built)')
    t0 = time.perf_counter()
    ctx = C.PairContext()
    ctx.set_cloud(P)
    say('wall: first set_cloud (context, allocations, upload, bounding box) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, ts = timed(lambda: ctx.set_cloud(P))
    say('wall: set_cloud %s ms (min %.1f)' % (ms(ts), 1e3 * min(ts)))
    res = {m: measure(ctx, n, m, r_max) for m in (16, 64)}
    q = P[::10]
    ctx.set_edges(np.linspace(r_max / 16, r_max, 16))
    r, ts = timed(lambda: ctx.count(q, local=True))
    say('wall: cross mode, every tenth point as a query (%d), 16 bins, local on: %s ms (min %.1f)' % (len(q), ms(ts), 1e3 * min(ts)))
    ctx.close()
    if sweep:
        for share in (0.25, 0.35, 0.5, 0.7, 1.0, 1.5):
            os.environ['NW_PAIRS_CELL_OF_RMAX'] = repr(share)
            c = C.PairContext()
            c.set_cloud(P)
            for m in (16, 64):
                got = measure(c, n, m, r_max, 'cell = %.2f r_max: ' % share)
                assert np.array_equal(got['hist'], res[m]['hist']) and np.array_equal(got['local'], res[m]['local'])
            c.close()
        del os.environ['NW_PAIRS_CELL_OF_RMAX']
    if with_ckdtree:
        from scipy.spatial import cKDTree
        P64 = P.astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(P64)
        say('host baseline: cKDTree build %.1f ms' % (1e3 * (time.perf_counter() - t0)))
        for m in (16, 64):
            radii = np.linspace(r_max / m, r_max, m)
            cum, ts = timed(lambda: tree.count_neighbors(tree, radii), repeats=1)     # (a minute or more at 10^6 points)
            say('host baseline: cKDTree.count_neighbors, %d radii: %s ms; cumulative equal: %s'
                % (m, ms(ts), np.array_equal(np.asarray(cum, np.int64) - n, res[m]['cumulative'].astype(np.int64))))


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if len(a) > 0 else 'c3', float(a[1]) if len(a) > 1 else 1.0, float(a[2]) if len(a) > 2 else 30.0, int(a[3]) if len(a) > 3 else 0,
         int(a[4]) if len(a) > 4 else 1)
