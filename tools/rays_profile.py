"""Wall time of ray casting through a kept context and the walk's three statistics (profiles/rays.txt): the inward thickness of all
vertices of config C3's mesh after a short fit, with one ray and with a cone of 30 per vertex.
usage: python tools/rays_profile.py [config] [scale] [iterations]
       python tools/rays_profile.py network [scale]      the self-consistency numbers on the fit of examples/fit_network.py
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rays_profile.py     (device time per kernel, a run of its own)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ch_shrinkwrap_amd import synth, rays as C

QS = [1, 5, 25, 50, 75, 95, 99]
ms = lambda a: ' '.join('%.1f' % (1e3 * x) for x in a)


def quantiles(a):
    return '  '.join('q%02d %.2f' % (q, v) for q, v in zip(QS, np.percentile(a, QS)))


def face_radii(mesh):
    """the mean and the largest rho_f of a mesh (NumPy, for the record: the walk's boxes grow with the largest)"""
    pos, faces = C._mesh_arrays(mesh)
    c = pos.astype(np.float64)[faces]
    rho = np.sqrt(((c - c.mean(1, keepdims=True)) ** 2).sum(2)).max(1)
    print('face radii: mean rho_f %.2f (cells of twice that unless the grid\'s cap widens them), rho_max %.2f = %.1f mean rho_f; %d faces above 2 mean rho_f'
          % (rho.mean(), rho.max(), rho.max() / rho.mean(), (rho > 2 * rho.mean()).sum()))


def thickness_report(mesh, ctx, n_rays, repeats):
    ids, origins, dirs = C.thickness_rays(mesh, 'in', n_rays, 120.0)
    o, d, sv = np.repeat(origins, n_rays, axis=0), np.ascontiguousarray(dirs.reshape(-1, 3)), np.repeat(ids, n_rays).astype(np.int32)
    casts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = ctx.cast(o, d, skip_vertex=sv)
        casts.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    th = C.thickness(mesh, n_rays=n_rays, context=ctx)
    whole = time.perf_counter() - t0
    st = ctx.cast(o, d, skip_vertex=sv, stats=True)
    assert st['t'].tobytes() == r['t'].tobytes() and st['face'].tobytes() == r['face'].tobytes()
    n = o.shape[0]
    ok = np.isfinite(th['thickness'][ids])
    print('n_rays %d: %d rays; cast (upload, kernel, four arrays back) %s ms (min %.1f, %.1f ns a ray); thickness() with the rays built '
          'on the host %.1f ms' % (n_rays, n, ms(casts), 1e3 * min(casts), 1e9 * min(casts) / n, 1e3 * whole))
    print('  rays that hit %d (%.2f %%), of them through the back %d; vertices without a valid ray %d'
          % ((r['face'] >= 0).sum(), 100.0 * (r['face'] >= 0).mean(), (r['exits'] & (r['face'] >= 0)).sum(), (~ok).sum()))
    print('  thickness: ' + quantiles(th['thickness'][ids][ok]))
    print('  walk: pieces %d (%.1f a ray), centroids read %d (%.1f a ray), exact tests %d (%.2f a ray)'
          % (st['pieces'], st['pieces'] / n, st['centroids'], st['centroids'] / n, st['tested'], st['tested'] / n))
    return th


def c3(name, scale, iters):
    from ch_shrinkwrap_amd.membrane_mesh import ShrinkwrapMembrane
    cfg = synth.make_config(name, scale=scale, seed=0)
    pts = np.ascontiguousarray(cfg['points'], np.float64)
    table = {'x': pts[:, 0], 'y': pts[:, 1], 'z': pts[:, 2], 'error_x': cfg['sigma'][:, 0], 'error_y': cfg['sigma'][:, 1], 'error_z': cfg['sigma'][:, 2]}
    surf = type('Surf', (), {'vertices': cfg['vertices'], 'faces': cfg['faces']})
    mesh = ShrinkwrapMembrane(max_iters=iters, remesher=None).execute({'surf': surf, 'filtered_localizations': table})
    pos, faces = C._mesh_arrays(mesh)
    print('%s x%g after %d iterations: %d vertices, %d faces' % (name, scale, iters, pos.shape[0], faces.shape[0]))
    t0 = time.perf_counter()
    ctx = C.RayContext()
    ctx.set_mesh(pos, faces)
    print('wall: first set_mesh (context, allocations, upload) %.1f ms' % (1e3 * (time.perf_counter() - t0)))
    sets = []
    for _ in range(5):
        t0 = time.perf_counter()
        ctx.set_mesh(pos, faces)
        sets.append(time.perf_counter() - t0)
    print('wall: set_mesh %s ms (min %.1f)' % (ms(sets), 1e3 * min(sets)))
    face_radii(mesh)
    thickness_report(mesh, ctx, 1, 5)
    thickness_report(mesh, ctx, 30, 3)
    ctx.close()


def network(scale):
    """the fit of examples/fit_network.py: its local thickness, and the side of a sample of localizations three ways"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import fit_network
    from ch_shrinkwrap_amd import distance
    mesh, _ = fit_network.main(scale)
    ctx = C.RayContext()
    ctx.set_mesh(*C._mesh_arrays(mesh))
    face_radii(mesh)
    for n_rays in (1, 30):
        thickness_report(mesh, ctx, n_rays, 1)
    cfg = synth.make_config('c4', scale=scale, seed=0)
    p = np.ascontiguousarray(cfg['points'][:200000], np.float64)
    t0 = time.perf_counter()
    ins = C.inside(p, mesh, context=ctx)
    dt = time.perf_counter() - t0
    d = distance.distance_to_mesh(p, mesh)
    pos = np.asarray(mesh.vertices, np.float64)
    clear = np.abs(d) > 1e-6 * np.linalg.norm(pos.max(0) - pos.min(0))
    print('inside(): %d localizations in %.1f ms; %.2f %% inside; against the sign of distance_to_mesh on the %d points farther than '
          '1e-6 of the diagonal from the surface: %d disagree' % (p.shape[0], 1e3 * dt, 100.0 * ins.mean(), clear.sum(), (ins != (d < 0))[clear].sum()))
    other = C.inside(p, mesh, direction=(-0.7071, 0.1234, 0.6961), context=ctx)
    print('inside() along a second direction: %d of %d points differ' % ((other != ins).sum(), p.shape[0]))
    ctx.close()


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'network':
        network(float(sys.argv[2]) if len(sys.argv) > 2 else 0.2)
    else:
        c3(sys.argv[1] if len(sys.argv) > 1 else 'c3', float(sys.argv[2]) if len(sys.argv) > 2 else 1.0, int(sys.argv[3]) if len(sys.argv) > 3 else 10)
