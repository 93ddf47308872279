"""Wall time, rounds and launches of the geodesic graph distance on the C3 mesh after ten iterations (397 620 faces at scale 1) through a
kept context -- set_mesh, then distances from 1 source, from 1 000 random sources and from 1 000 sources capped at 200 nm, each with
and without labels --, the share of half-edges the stamp skip removes, and scipy.sparse.csgraph.dijkstra on the same host and the same
arcs as the baseline, the values compared to 1e-12 (profiles/geodesic.txt).
usage: python tools/geodesic_profile.py [scale] [iters] [scipy: 0 | 1] [mesh cache .npz]
       defaults 1.0 10 1 none
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/geodesic_profile.py 1.0 10 0 CACHE
                                                                       (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, distance, geodesic as G

ms = lambda a: ' '.join('%.1f' % (1e3 * x) for x in a)


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


def scene(scale, iters, cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z['pos'], z['faces']
    cfg = synth.make_config('c3', scale=scale, seed=0)
    pts, sigma = np.ascontiguousarray(cfg['points'], np.float64), np.asarray(cfg['sigma'], np.float64)
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': sigma[:, 0], 'error_y': sigma[:, 1], 'error_z': sigma[:, 2]}
    surf = type('Surf', (), {'vertices': cfg['vertices'], 'faces': cfg['faces']})
    mesh = ShrinkwrapMembrane(max_iters=iters, remesher=None).execute({'surf': surf, 'filtered_localizations': table})
    pos, faces, _ = distance._mesh_arrays(mesh, False)
    if cache:
        np.savez(cache, pos=pos, faces=faces)
    return pos, faces


def host_arcs(pos, faces, twin):
    """the arcs of the definition in NumPy (as tests/mesh_geodesic_ref.py states them), as a CSR matrix for scipy"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import mesh_geodesic_ref as R
    from scipy.sparse import coo_matrix
    tail, head, w = R.arcs(pos, faces, True, twin)
    _, first = np.unique(tail * len(pos) + head, return_index=True)
    return coo_matrix((w[first], (tail[first], head[first])), shape=(len(pos),) * 2).tocsr()


def main(scale=1.0, iters=10, with_scipy=1, cache=None):
    pos, faces = scene(scale, iters, cache)
    V, F = len(pos), len(faces)
    say('c3 x%g after %d iterations: %d vertices, %d faces, %d half-edges; batch %d rounds, up to %d sweeps a round' % (scale, iters, V, F, 3 * F, G.BATCH, G.SWEEPS))
    try:
        from ch_shrinkwrap_amd import build
        for k, r in sorted(build.kernel_resources(build.OBJ_GEODESIC).items()):
            say('  %-14s %3d VGPRs %4d B LDS scratch %d' % (k, r['vgpr'], r['lds'], r['scratch']))
    except Exception:
        say('  (no object file here: the kernels\' registers are read where the library is built)')
    twin = distance.mesh_twins(faces, V)
    t0 = time.perf_counter()
    ctx = G.GeodesicContext()
    ctx.set_mesh(pos, faces, twin)
    say('wall: first set_mesh (context, allocations, upload, weights) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, ts = timed(lambda: ctx.set_mesh(pos, faces, twin))
    say('wall: set_mesh %s ms (min %.1f)' % (ms(ts), 1e3 * min(ts)))
    rng = np.random.default_rng(0)
    many = rng.choice(V, 1000, replace=False).astype(np.int32)
    cases = [('1 source', np.array([0], np.int32), np.inf), ('1 000 sources', many, np.inf), ('1 000 sources, cap 200 nm', many, 200.0)]
    kept = {}
    for name, ids, cap in cases:
        for labels in (False, True):
            r, ts = timed(lambda: ctx.distances(ids, max_distance=cap, labels=labels))
            i = r['info']
            rounds = i['rounds'] + i['label_rounds']
            say('wall: %s, labels %s: %s ms (min %.1f); rounds %d + %d, launches %d: %.0f rounds a second; atomics that lowered a value %d; '
                'arcs looked at %d = %.1f %% of rounds x half-edges (the stamp skip and the idle diagonal lanes remove the rest); reached %d, in band %d, diagonals %d'
                % (name, 'on ' if labels else 'off', ms(ts), 1e3 * min(ts), i['rounds'], i['label_rounds'], i['launches'], rounds / min(ts), i['lowered'],
                   i['relaxed'], 100.0 * i['relaxed'] / max(1, rounds * i['halfedges']), i['reached'], i['in_band'], i['diagonals']))
        kept[name] = r
    ctx.close()
    if with_scipy:
        from scipy.sparse.csgraph import dijkstra
        t0 = time.perf_counter()
        A = host_arcs(pos, faces, twin)
        say('host baseline: the arcs in NumPy and a CSR matrix %.1f ms' % (1e3 * (time.perf_counter() - t0)))
        for name, ids, cap in cases:
            t0 = time.perf_counter()
            want = dijkstra(A, directed=True, indices=ids, limit=cap, min_only=True)
            dt = time.perf_counter() - t0
            got = kept[name]['distance']
            both = np.isfinite(got) & np.isfinite(want)
            agree = bool((np.isfinite(got) == np.isfinite(want)).all() and np.allclose(got[both], want[both], rtol=1e-12, atol=0))
            say('host baseline: scipy.sparse.csgraph.dijkstra, %s: %.1f ms; values agree to 1e-12: %s' % (name, 1e3 * dt, agree))


if __name__ == '__main__':
    a = sys.argv[1:]
    main(float(a[0]) if len(a) > 0 else 1.0, int(a[1]) if len(a) > 1 else 10, int(a[2]) if len(a) > 2 else 1, a[3] if len(a) > 3 else None)
