"""Wall time of the banded signed-distance volume through a kept context, the walk's counters, and the only route to the same numbers
without it: distance_to_mesh on the host-built list of the lattice's nodes (profiles/volume.txt).
usage: python tools/volume_profile.py [c3|c4|all] [scale] [iterations]
       c3: config C3's mesh after a short fit, h = 8 nm, band 3 h; set_mesh, volume, offset_surface(+20), and the baseline
       c4: config C4's start surface on the 8 nm grid of profiles/isosurface_c4.txt (322 x 258 x 49 at scale 1)
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/volume_profile.py c3     (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, distance, isosurface as I, volume as C

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


def face_radii(pos, faces):
    c = pos.astype(np.float64)[faces]
    cen = ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0
    rho = np.sqrt(((c - cen[:, None, :]) ** 2).sum(2)).max(1)
    return float(rho.mean()), float(rho.max())


def report(name, pos, faces, lo, h, dims, d_cap, baseline_rows=0):
    n = int(np.prod(np.asarray(dims, np.int64)))
    rho_mean, rho_max = face_radii(pos, faces)
    cell = max(2.0 * rho_mean, (d_cap + rho_max) / 2.0)
    say('%s: %d vertices, %d faces; lattice %d x %d x %d = %d nodes at h = %g nm, band %g nm; mean rho_f %.2f, rho_max %.2f -> starting cell '
        'max(2 mean rho_f = %.2f, (d_cap + rho_max) / 2 = %.2f) = %.2f nm'
        % (name, pos.shape[0], faces.shape[0], dims[0], dims[1], dims[2], n, h, d_cap, rho_mean, rho_max, 2 * rho_mean, (d_cap + rho_max) / 2, cell))
    t0 = time.perf_counter()
    ctx = C.VolumeContext()
    ctx.set_mesh(pos, faces)
    say('wall: first set_mesh (context, twins on the host, allocations, upload) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, sets = timed(lambda: ctx.set_mesh(pos, faces))
    say('wall: set_mesh %s ms (min %.1f)' % (ms(sets), 1e3 * min(sets)))
    t0 = time.perf_counter()
    ctx.volume(lo, h, dims, d_cap, return_sd=False)
    say('wall: first volume (binning at this band\'s cell size, allocations) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    _, dev = timed(lambda: ctx.volume(lo, h, dims, d_cap, return_sd=False))
    out, host = timed(lambda: ctx.volume(lo, h, dims, d_cap, return_face=True, return_mask=True), 3)
    i = ctx.info
    far = i['nodes'] - i['in_band']
    say('wall: volume, arrays left on the device %s ms (min %.1f, %.1f ns a node); with sd, face and mask copied to the host %s ms'
        % (ms(dev), 1e3 * min(dev), 1e9 * min(dev) / n, ms(host)))
    say('  in band %d of %d nodes (%.2f %%), inside %.2f %%; grid of %d cells' % (i['in_band'], n, 100.0 * i['in_band'] / n, 100.0 * out[2].mean(), i['cells']))
    say('  walk: near node %.2f rings, %.1f centroids read; far node %.2f rings, %.1f centroids read'
        % (i['rings_near'] / max(i['in_band'], 1), i['centroids_near'] / max(i['in_band'], 1), i['rings_far'] / max(far, 1), i['centroids_far'] / max(far, 1)))
    sd = out[0]
    if baseline_rows:
        # the route without this unit: all nodes of the lattice as a host array through distance_to_mesh, copies included
        step = max(1, (int(dims[1]) * int(dims[2])) // baseline_rows)
        rows = np.arange(0, int(dims[1]) * int(dims[2]), step)
        ax = [float(lo[a]) + (np.arange(int(dims[a]), dtype=np.float64) + 0.5) * float(np.float32(h)) for a in range(3)]
        t0 = time.perf_counter()
        j, k = rows % int(dims[1]), rows // int(dims[1])
        nodes = np.stack([np.tile(ax[0], rows.size), np.repeat(ax[1][j], int(dims[0])), np.repeat(ax[2][k], int(dims[0]))], 1)
        t_build = time.perf_counter() - t0
        dctx = distance.DistanceContext()
        dctx.set_mesh(pos, faces, distance.mesh_twins(faces, pos.shape[0]))
        dist, tq = timed(lambda: dctx.query(nodes, signed=True), 2)
        dctx.close()
        mine = sd.reshape(int(dims[2]) * int(dims[1]), int(dims[0]))[rows].ravel()
        near = np.abs(dist) <= d_cap
        same = bool(np.array_equal(mine[near], dist[near]) and np.array_equal(np.signbit(mine), np.signbit(dist)))
        scale = (int(dims[1]) * int(dims[2])) / float(rows.size)
        say('baseline: distance_to_mesh on %d of %d x-rows (every %d-th; %d nodes, 24 B a node up, 8 B down): node list on the host %.1f ms, query %s ms '
            '(min %.1f); extrapolated to the lattice x%.2f: %.1f ms against %.1f ms -> %.1f x; in-band values and all signs equal: %s'
            % (rows.size, int(dims[1]) * int(dims[2]), step, nodes.shape[0], 1e3 * t_build, ms(tq), 1e3 * min(tq), scale,
               1e3 * scale * (min(tq) + t_build), 1e3 * min(host), scale * (min(tq) + t_build) / min(host), same))
    ctx.close()


def c3(name, scale, iters):
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    cfg = synth.make_config(name, scale=scale, seed=0)
    pts = np.ascontiguousarray(cfg['points'], np.float64)
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    surf = type('Surf', (), {'vertices': cfg['vertices'], 'faces': cfg['faces']})
    mesh = ShrinkwrapMembrane(max_iters=iters, remesher=None).execute({'surf': surf, 'filtered_localizations': table})
    pos, faces, _ = distance._mesh_arrays(mesh, False)
    h = 8.0
    lo, dims = I.grid_for(pos, h, 5)
    report('%s x%g after %d iterations' % (name, scale, iters), pos, faces, lo, h, dims, 3 * h, baseline_rows=2048)
    for remesh in (False, True):
        s, t = timed(lambda: C.offset_surface((pos, faces), 20.0, voxel_size=h, remesh=remesh), 3)
        say('offset_surface(+20 nm, h = 8 nm, remesh=%s) end to end %s ms: %d vertices, %d faces; lattice %s, %d in band of %d nodes'
            % (remesh, ms(t), s.vertices.shape[0], s.faces.shape[0], s.info['dims'], s.info['in_band'], s.info['nodes']))


def c4(scale):
    cfg = synth.make_config('c4', scale=scale, seed=0)
    pos, faces = np.ascontiguousarray(cfg['vertices'], np.float32), np.ascontiguousarray(cfg['faces'], np.int32)
    h = 8.0
    lo, dims = I.grid_for(cfg['points'], h, 5)                    # the grid of profiles/isosurface_c4.txt: the cloud's, passes + 3 voxels of margin
    report('c4 x%g start surface on the cloud\'s grid' % scale, pos, faces, lo, h, dims, 3 * h, baseline_rows=512)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'all'
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    if what in ('c3', 'all'):
        c3('c3', scale, int(sys.argv[3]) if len(sys.argv) > 3 else 10)
    if what in ('c4', 'all'):
        c4(scale)
