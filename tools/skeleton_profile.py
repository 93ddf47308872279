"""Wall time of the level-set skeleton on the C3 mesh after ten iterations (397 620 faces at scale 1) through a kept context: set_mesh, then
level_sets at band widths of 1, 2 and 4 mean edge lengths on the geodesic graph distance from vertex 0 -- the whole call, and with
NWA_FLAG_TIMING the time per kernel, of the arc keys' download and of their de-duplication on the host, with the piece, node and arc
counts --, and for comparison the restatement's component step alone (scipy.sparse.csgraph.connected_components on the same piece graph,
same host) (profiles/skeleton.txt).
usage: python tools/skeleton_profile.py [scale] [iters] [scipy: 0 | 1] [mesh cache .npz]
       defaults 1.0 10 1 none"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from ch_shrinkwrap_amd import distance, geodesic as G, skeleton as S
from ch_shrinkwrap_amd.isosurface import mean_edge_length
from geodesic_profile import scene, timed, say, ms

STAGES = ('upload_us', 'bands_us', 'scan_us', 'init_us', 'hook_us', 'compress_us', 'sums_us', 'arcs_us', 'vertex_us', 'keys_download_us', 'dedup_us')


def host_components(faces, twin, D, w):
    """the piece graph as tests/mesh_skeleton_ref.py builds it, and scipy's components on it: (seconds to build, seconds for the components, nodes)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    b = np.floor(D / w).astype(np.int64)
    fb = b[faces]
    lo, span = fb.min(1), fb.max(1) - fb.min(1) + 1
    start = np.concatenate([[0], np.cumsum(span)])
    h = np.arange(3 * faces.shape[0])
    t = twin.astype(np.int64)
    own = t > h
    h, t = h[own], t[own]
    bu, bv = b[faces.reshape(-1)[h]], b[faces[h // 3, (h % 3 + 1) % 3]]
    k0, n = np.minimum(bu, bv), np.abs(bu - bv) + 1
    e = np.repeat(np.arange(h.size), n)
    k = k0[e] + (np.arange(e.size) - np.repeat(np.cumsum(n) - n, n))
    f, g = h[e] // 3, t[e] // 3
    A = coo_matrix((np.ones(e.size), (start[f] + k - lo[f], start[g] + k - lo[g])), shape=(int(start[-1]),) * 2).tocsr()
    t1 = time.perf_counter()
    nn, _ = connected_components(A, directed=False)
    return t1 - t0, time.perf_counter() - t1, int(nn)


def main(scale=1.0, iters=10, with_scipy=1, cache=None):
    pos, faces = scene(scale, iters, cache)
    V, F = len(pos), len(faces)
    edge = mean_edge_length(pos, faces)
    say('c3 x%g after %d iterations: %d vertices, %d faces, mean edge %.2f nm' % (scale, iters, V, F, edge))
    twin = distance.mesh_twins(faces, V)
    g = G.GeodesicContext()
    D = g.set_mesh(pos, faces, twin).distances([0])['distance']
    g.close()
    t0 = time.perf_counter()
    ctx = S.SkeletonContext()
    ctx.set_mesh(pos, faces, twin)
    say('wall: first set_mesh (context, allocations, upload, bounding box) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, ts = timed(lambda: ctx.set_mesh(pos, faces, twin))
    say('wall: set_mesh %s ms (min %.1f)' % (ms(ts), 1e3 * min(ts)))
    for m in (1.0, 2.0, 4.0):
        w = m * edge
        ctx.level_sets(D, w)                                      # (allocations)
        r, ts = timed(lambda: ctx.level_sets(D, w))
        i = r['info']
        say('wall: level_sets at %g mean edges (%.1f nm): %s ms (min %.1f), fetch included; pieces %d, nodes %d, arcs %d (from %d keys), segments %d, '
            'compare-and-swaps %d of which %d lost' % (m, w, ms(ts), 1e3 * min(ts), i['pieces'], i['nodes'], i['arcs'], i['arc_keys'], i['segments'], i['atomics'],
                                                      i['hook_retries']))
        best = None
        for _ in range(3):
            t = ctx.level_sets(D, w, timing=True)['info']
            best = t if best is None else dict((k, min(best[k], t[k])) if k in STAGES else (k, best[k]) for k in best)
        say('  per stage, the stream waited for after each (us, best of 3): ' + ', '.join('%s %d' % (k[:-3], best[k]) for k in STAGES))
        t0 = time.perf_counter()
        L = ctx.L
        out = [np.zeros(F + 1, np.int32), np.zeros(i['pieces'], np.int32), np.zeros(V, np.int32), np.zeros(i['nodes'], np.int32),
               np.zeros((i['nodes'], 12), np.uint64), np.zeros((i['arcs'], 2), np.int32)]
        ctx.check(L.nwa_fetch(ctx.h, *[a.ctypes.data_as(S.ctypes.c_void_p) for a in out]), 'nwa_fetch')
        say('  the download of the tables (nwa_fetch): %.2f ms for %.1f MB' % (1e3 * (time.perf_counter() - t0), sum(a.nbytes for a in out) / 1e6))
        if with_scipy and np.isfinite(D).all():
            tb, tc, nn = host_components(faces, twin, D, w)
            say('  host baseline: the piece graph in NumPy %.1f ms, scipy.sparse.csgraph.connected_components on it %.1f ms; %d nodes (%s)'
                % (1e3 * tb, 1e3 * tc, nn, 'the same' if nn == i['nodes'] else 'DIFFERENT'))
    ctx.close()


if __name__ == '__main__':
    a = sys.argv[1:]
    main(float(a[0]) if len(a) > 0 else 1.0, int(a[1]) if len(a) > 1 else 10, int(a[2]) if len(a) > 2 else 1, a[3] if len(a) > 3 else None)
