"""Wall time of the mesh-to-mesh distance through a kept context, the walk's counters, and the only route there was before it:
distance_to_mesh of A's vertices against B, with how often that route is wrong (profiles/proximity.txt).
usage: python tools/proximity_profile.py [scale] [iterations] [mesh.npz | -] [sweep]
       the scene: config C3's mesh after a short fit (A) against a copy of itself shifted by SHIFT so that the two overlap in part (B);
       bands 30 nm and inf.  mesh.npz: where the fitted mesh is kept between runs (made if it is not there; - for none)
       sweep: after the report, the query's time and counters at explicit cell sizes (SWEEP), the measurement the unit's own choice
       of cell size (nwm_band_cell in csrc/nw_proximity_core.h) rests on
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/proximity_profile.py 1.0 10 mesh.npz
                                                                       (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, distance, proximity as C

SHIFT = (0.0, 520.0, 35.0)
# band -> the cell sizes of the sweep in nm; 0 = the unit's own choice
SWEEP = {30.0: (0.0, 5.0, 8.0, 12.0, 16.0, 22.0, 32.0), np.inf: (0.0, 5.0, 10.0, 20.0, 40.0, 80.0)}
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


def fitted_mesh(scale, iters, cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z['pos'], z['faces']
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    cfg = synth.make_config('c3', scale=scale, seed=0)
    pts = np.ascontiguousarray(cfg['points'], np.float64)
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    surf = type('Surf', (), {'vertices': cfg['vertices'], 'faces': cfg['faces']})
    mesh = ShrinkwrapMembrane(max_iters=iters, remesher=None).execute({'surf': surf, 'filtered_localizations': table})
    pos, faces, _ = distance._mesh_arrays(mesh, False)
    if cache:
        np.savez(cache, pos=pos, faces=faces)
    return pos, faces


def sweep(pa, fa, pb, fb):
    ctx = C.ProximityContext()
    n = fa.shape[0]
    for band, cells in SWEEP.items():
        for cell in cells:
            ctx.set_mesh(pb, fb, cell_size=cell)
            ctx.query(pa, fa, band=band)                                  # (binning, allocations)
            r, ts = timed(lambda: ctx.query(pa, fa, band=band))
            i = r['info']
            say('sweep: band %g, cell %s -> %.2f nm (%d cells): query %s ms (min %.1f); a face: %.2f rings, %.1f centroids read, %.2f exact tests'
                % (band, 'of the unit\'s choice' if cell == 0.0 else 'asked %g' % cell, i['cell_size'], i['cells'], ms(ts), 1e3 * min(ts), i['rings'] / n,
                   i['centroids'] / n, i['tests'] / n))
    ctx.close()


def main(scale=1.0, iters=10, cache=None, with_sweep=False):
    pa, fa = fitted_mesh(scale, iters, cache)
    pb, fb = (pa.astype(np.float64) + np.asarray(SHIFT)).astype(np.float32), fa
    c = pa.astype(np.float64)[fa]
    rho = np.sqrt(((c - c.mean(1, keepdims=True)) ** 2).sum(2)).max(1)
    say('c3 x%g after %d iterations: %d vertices, %d faces, against itself shifted by %s; mean rho %.2f, rho_max %.2f nm'
        % (scale, iters, pa.shape[0], fa.shape[0], SHIFT, rho.mean(), rho.max()))
    try:
        from ch_shrinkwrap_amd import build
        for k, r in sorted(build.kernel_resources(build.OBJ_PROXIMITY).items()):
            say('  %-16s %3d VGPRs %4d B LDS scratch %d' % (k, r['vgpr'], r['lds'], r['scratch']))
    except Exception:
        say('  (no object file here: the kernels\' registers are read where the library is built)')
    t0 = time.perf_counter()
    ctx = C.ProximityContext()
    ctx.set_mesh(pb, fb)
    say('wall: first set_mesh (context, allocations, upload) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, sets = timed(lambda: ctx.set_mesh(pb, fb))
    say('wall: set_mesh %s ms (min %.1f)' % (ms(sets), 1e3 * min(sets)))
    results = {}
    for band in (30.0, np.inf):
        t0 = time.perf_counter()
        ctx.query(pa, fa, band=band)
        first = time.perf_counter() - t0
        r, ts = timed(lambda: ctx.query(pa, fa, band=band, return_closest=True))
        i, n = r['info'], fa.shape[0]
        say('band %g: first query (binning at this band\'s cell size, allocations) %.1f ms; query %s ms (min %.1f, %.1f ns a face)'
            % (band, 1e3 * first, ms(ts), 1e3 * min(ts), 1e9 * min(ts) / n))
        say('  cell %.2f nm, %d cells; in band %d of %d faces (%.2f %%), at 0: %d; a face: %.2f rings, %.1f centroids read, %.2f exact tests'
            % (i['cell_size'], i['cells'], i['in_band'], n, 100.0 * i['in_band'] / n, i['at_zero'], i['rings'] / n, i['centroids'] / n, i['tests'] / n))
        results[band] = r
    ctx.close()
    # the route there was: the distance of A's vertices from B; a face's value is the smallest of its corners'
    dctx = distance.DistanceContext()
    t0 = time.perf_counter()
    dctx.set_mesh(pb, fb)
    t_set = time.perf_counter() - t0
    dv, tq = timed(lambda: dctx.query(pa.astype(np.float64), signed=False))
    dctx.close()
    by_vertex = dv[fa].min(1)
    r = results[np.inf]
    near = r['distance'] <= 30.0
    crossing = r['kind'] == 0
    say('baseline: distance_to_mesh of A\'s %d vertices against B: set_mesh %.1f ms, query %s ms (min %.1f)' % (pa.shape[0], 1e3 * t_set, ms(tq), 1e3 * min(tq)))
    say('  of the %d faces within 30 nm, the smallest corner value exceeds the exact face distance by more than 1 nm on %d (largest excess %.2f nm); '
        'of the %d crossing faces (kind 0), it is positive on %d (largest %.2f nm); it is never below the exact distance: %s'
        % (near.sum(), (near & (by_vertex - r['distance'] > 1.0)).sum(), (by_vertex - r['distance'])[near].max() if near.any() else 0.0,
           crossing.sum(), (crossing & (by_vertex > 0)).sum(), by_vertex[crossing].max() if crossing.any() else 0.0,
           bool((by_vertex >= r['distance']).all())))
    say('  contact area of A within 30 nm: %.0f nm^2 by exact face distance, %.0f nm^2 by the corners\' route'
        % (face_area(pa, fa)[near].sum(), face_area(pa, fa)[by_vertex <= 30.0].sum()))
    if with_sweep:
        sweep(pa, fa, pb, fb)


def face_area(pos, faces):
    p = pos.astype(np.float64)[faces]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return 0.5 * np.sqrt((n * n).sum(1))


if __name__ == '__main__':
    main(float(sys.argv[1]) if len(sys.argv) > 1 else 1.0, int(sys.argv[2]) if len(sys.argv) > 2 else 10,
         sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != '-' else None, 'sweep' in sys.argv[4:])
