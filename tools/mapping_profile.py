"""Wall time of mapping a cloud onto a fitted mesh through a kept context, the walk's counters, the walk alone against the walk with its
integer atomics, and the only route there was before it: distance_to_mesh with faces and closest points brought to the host, then
np.add.at (profiles/mapping.txt).
usage: python tools/mapping_profile.py [scale] [iterations] [mesh.npz | -]
       the scene: config C3's mesh after a short fit and C3's own localizations, band 30 nm, two value columns
       mesh.npz: where the fitted mesh is kept between runs (made if it is not there; - for none)
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mapping_profile.py 1.0 10 mesh.npz
                                                                       (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, distance, mapping as C

BAND = 30.0
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
    cfg = synth.make_config('c3', scale=scale, seed=0)
    pts = np.ascontiguousarray(cfg['points'], np.float64)
    sigma = np.asarray(cfg['sigma'], np.float64)
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return pts, sigma, z['pos'], z['faces']
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': sigma[:, 0], 'error_y': sigma[:, 1], 'error_z': sigma[:, 2]}
    surf = type('Surf', (), {'vertices': cfg['vertices'], 'faces': cfg['faces']})
    mesh = ShrinkwrapMembrane(max_iters=iters, remesher=None).execute({'surf': surf, 'filtered_localizations': table})
    pos, faces, _ = distance._mesh_arrays(mesh, False)
    if cache:
        np.savez(cache, pos=pos, faces=faces)
    return pts, sigma, pos, faces


def main(scale=1.0, iters=10, cache=None):
    pts, sigma, pos, faces = scene(scale, iters, cache)
    n, V, F = len(pts), len(pos), len(faces)
    vals = np.ascontiguousarray(np.stack([sigma[:, 0], np.arange(n, dtype=np.float64)], 1))
    scales = [C.column_scale(vals[:, c]) for c in range(vals.shape[1])]
    say('c3 x%g after %d iterations: %d vertices, %d faces, %d localizations, band %g nm, %d value columns' % (scale, iters, V, F, n, BAND, vals.shape[1]))
    try:
        from ch_shrinkwrap_amd import build
        for k, r in sorted(build.kernel_resources(build.OBJ_MAPPING).items()):
            say('  %-16s %3d VGPRs %4d B LDS scratch %d' % (k, r['vgpr'], r['lds'], r['scratch']))
    except Exception:
        say('  (no object file here: the kernels\' registers are read where the library is built)')
    t0 = time.perf_counter()
    ctx = C.MappingContext()
    ctx.set_mesh(pos, faces)
    say('wall: first set_mesh (context, allocations, upload) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, sets = timed(lambda: ctx.set_mesh(pos, faces))
    say('wall: set_mesh %s ms (min %.1f)' % (ms(sets), 1e3 * min(sets)))
    t0 = time.perf_counter()
    ctx.map(pts, band=BAND, values=vals, scales=scales)
    say('wall: first map (binning at this band\'s cell size, allocations) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    full, t_full = timed(lambda: ctx.map(pts, band=BAND, values=vals, scales=scales))
    i = full['info']
    say('wall: map, every output to the host: %s ms (min %.1f, %.1f ns a localization)' % (ms(t_full), 1e3 * min(t_full), 1e9 * min(t_full) / n))
    say('  cell %.2f nm, %d cells; in band %d of %d (%.2f %%); a localization: %.2f rings, %.1f centroids read'
        % (i['cell_size'], i['cells'], i['in_band'], n, 100.0 * i['in_band'] / n, i['rings'] / n, i['centroids'] / n))
    # the launch alone: the cloud and the values on the device, no per-localization output, accumulators left on the device
    import torch
    tp, tv = torch.from_numpy(pts).to('cuda'), torch.from_numpy(vals).to('cuda')
    torch.cuda.synchronize()
    dev_pts, dev_vals = (tp.data_ptr(), n), (tv.data_ptr(), vals.shape[1])
    for label, kw in (('walk and atomics, %d columns' % vals.shape[1], dict(values=dev_vals, scales=scales, accumulators=False)),
                      ('walk and atomics, no column', dict(accumulators=False)),
                      ('walk alone (NWL_WALK_ONLY)', dict(walk_only=True))):
        ctx.map(dev_pts, band=BAND, per_point=False, **kw)
        _, ts = timed(lambda: ctx.map(dev_pts, band=BAND, per_point=False, **kw), repeats=5)
        say('wall: map from device pointers, nothing brought back, %s: %s ms (min %.2f)' % (label, ms(ts), 1e3 * min(ts)))
    ctx.close()
    # the route there was: distance_to_mesh with faces and closest points to the host, then np.add.at of barycentric weights in float64
    dctx = distance.DistanceContext()
    dctx.set_mesh(pos, faces)
    dctx.query(pts, signed=False, return_closest=True, return_face=True)

    def host_route():
        t0 = time.perf_counter()
        dist, closest, face = dctx.query(pts, signed=False, return_closest=True, return_face=True)
        t1 = time.perf_counter()
        near = dist <= BAND
        fa = face[near]
        tri = pos.astype(np.float64)[faces[fa]]
        nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        q = closest[near]
        e = np.stack([np.einsum('ij,ij->i', np.cross(tri[:, (k + 1) % 3] - tri[:, k], q - tri[:, k]), nrm) for k in range(3)], 1).clip(min=0.0)
        w = e[:, [1, 2, 0]] / np.maximum(e.sum(1), 1e-300)[:, None]
        mass, sums = np.zeros(V), np.zeros((V, vals.shape[1]))
        for k in range(3):
            np.add.at(mass, faces[fa, k], w[:, k])
            for c in range(vals.shape[1]):
                np.add.at(sums[:, c], faces[fa, k], w[:, k] * vals[near, c])
        return t1 - t0, time.perf_counter() - t1, mass
    runs = [host_route() for _ in range(2)]
    dctx.close()
    say('host route: distance_to_mesh(return_face, return_closest) %s ms, then weights and np.add.at %s ms'
        % (ms([r[0] for r in runs]), ms([r[1] for r in runs])))
    mine = full['mass'].astype(np.float64) / C.W_ONE
    say('  its float64 masses differ from the integers\' by at most %.3g of a localization (total %.6f against %d)'
        % (np.abs(runs[-1][2] - mine).max(), runs[-1][2].sum(), full['n_in_band']))


if __name__ == '__main__':
    main(float(sys.argv[1]) if len(sys.argv) > 1 else 1.0, int(sys.argv[2]) if len(sys.argv) > 2 else 10,
         sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != '-' else None)
