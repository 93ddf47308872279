"""
GPU tests (run with -m gpu on an MI355X) of the iteration kernels, stage by stage: k_attract and its copy inside k_nn_wave, k_prior_ring /
k_prior_directions, k_subspace_point_sums, k_reduce_scalars, k_solve_update.

Every iteration is run phase by phase (nw_iter_attract / nw_iter_directions / nw_iter_update through parallel.HipExecutor) and the device's
arrays are read between the phases.  Each stage is then checked FROM THE DEVICE'S OWN INPUTS to that stage against tests/fit_stages_ref.py
(pinned to the oracle on the CPU by tests/test_fit_stages_ref.py): nothing drifts, the tolerances are per element and derived there, the
integer scatter is compared for equality, and what the kernels compute in float32 in a fixed order (solve, update, the conversions of the
accumulator) is compared bit for bit.

  (a) per-point rows   face against a brute-force reference, vidx == faces[face], w / dist / res within their bounds
  (b) scatter          the accumulator after the attraction step == the integer restatement; S0 and pi bit-equal to its conversions; both
                       attraction paths (k_attract, and the workgroups appended to the query launch, which take over from a block's second
                       iteration on); all zero again after the update
  (c) prior            fdef within 2u max(|fdef|, |vc|, |alpha|); S1 == -float32(prefs64) away from rounding boundaries; isolated slots
  (d) sums             each of the 28 slots (32 parts added in order) within n 2^-53 sum|terms|; count and largest distance exact
  (e) solve, update    H, G, c of the log bit-equal to the float32 restatement; fnew, S[:,2], mesh positions bit-equal
"""
import ctypes

import numpy as np
import pytest

import fit_stages_ref as R

pytestmark = pytest.mark.gpu

U = R.U32
SL = R.scalar_slots()
LAMS = [10.0]


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def _jittered_icosphere(nsub, radius=100.0, seed=1, jitter=0.4):
    from ch_shrinkwrap_amd.trimesh import icosphere
    v, f = icosphere(nsub, radius)
    rng = np.random.default_rng(seed)
    return (v + rng.normal(scale=jitter, size=v.shape)).astype('f4'), f


def _shell_points(n, radius, seed):
    """n points 2-8 nm off the sphere of that radius, inside or outside"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    off = rng.uniform(2.0, 8.0, n) * rng.choice([-1.0, 1.0], n)
    return (d * (radius + off)[:, None]).astype('f4')


def _sigma_inv(n, seed):
    return (1.0 / np.random.default_rng(seed).uniform(5.0, 15.0, size=(n, 3))).astype('f4')


def _over_faces(v, f, face_ids, seed, spread=0.08):
    """one point over each listed face: near its centroid (barycentric jitter), 2-8 nm off the surface along the centroid's direction"""
    rng = np.random.default_rng(seed)
    n = len(face_ids)
    b = np.full((n, 3), 1.0 / 3.0) + rng.uniform(-spread, spread, size=(n, 3))
    b /= b.sum(1)[:, None]
    p = (v[f[face_ids]].astype('f8') * b[:, :, None]).sum(1)
    r = np.linalg.norm(p, axis=1)
    return (p * ((r + rng.uniform(2.0, 8.0, n) * rng.choice([-1.0, 1.0], n)) / r)[:, None]).astype('f4')


def _plane_patch(nx, ny, step=10.0, seed=3, jitter=1.0):
    """nx x ny vertices of a triangulated plane with its boundary: corner valences 2 and 3, edges 4, interior 6"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step, indexing='ij')
    v = np.stack([x.ravel(), y.ravel(), rng.normal(scale=jitter, size=nx * ny)], 1).astype('f4')
    v[:, :2] += rng.uniform(-0.1 * step, 0.1 * step, size=(nx * ny, 2)).astype('f4')
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing='ij')
    a = (i * ny + j).ravel()
    b, c, d = a + ny, a + ny + 1, a + 1
    f = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype('i4')
    return v, f


def _over_plane(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3))
    p[:, 0] = rng.uniform(lo[0], hi[0], n)
    p[:, 1] = rng.uniform(lo[1], hi[1], n)
    p[:, 2] = rng.uniform(2.0, 8.0, n) * rng.choice([-1.0, 1.0], n)
    return p.astype('f4')


def _disjoint_faces(f, want):
    """greedy pass over the faces in index order: pairwise vertex-disjoint faces"""
    used = np.zeros(int(f.max()) + 1, bool)
    out = []
    for k in range(f.shape[0]):
        if not used[f[k]].any():
            used[f[k]] = True
            out.append(k)
            if len(out) == want:
                break
    return np.array(out)


# ---- the device, phase by phase -------------------------------------------------------------------------------------------------------------
def _get(cg, what, shape, dtype):
    from ch_shrinkwrap_amd import _lib as nw
    a = np.empty(shape, dtype)
    cg._native.check(cg._L.nw_get(cg._h, what, nw.ptr(a), a.nbytes))
    return a


def _nbytes(cg, what):
    p, nb = ctypes.c_void_p(), ctypes.c_int64()
    cg._native.check(cg._L.nw_device_ptr(cg._h, what, ctypes.byref(p), ctypes.byref(nb)))
    return int(nb.value)


def run_stages(cg, n_iters, pts, sigma_inv, weights=None, data=None):
    """One block of n_iters iterations through parallel.HipExecutor with the device's arrays read after every phase (nw_get synchronises).
    Returns dict(q, qw, nbr, nrm, valid, iters=[{'A': after attract, 'B': after directions, 'C': after update}], logs)."""
    from ch_shrinkwrap_amd import _lib as nw
    from ch_shrinkwrap_amd.parallel import HipExecutor
    ex = HipExecutor(cg)
    M, N = cg.M, pts.shape[0]
    cg._upload_points(sigma_inv, weights)
    if data is not None:                      # the residual's target, after the upload that would drop it (begin() finds the points uploaded)
        d32 = np.ascontiguousarray(data, 'f4')
        cg._native.check(cg._L.nw_set_data(cg._h, nw.ptr(d32)))
    ex.begin(pts, LAMS, n_iters, sigma_inv, weights, None, False, True)
    out = dict(q=ex.local_quantum(), qw=2.0 ** -40, iters=[])
    for it in range(n_iters):
        ex.attract()
        A = dict(face=_get(cg, nw.NW_ARR_FACE, (N,), 'i4'), vidx=_get(cg, nw.NW_ARR_VIDX, (N, 3), 'i4'), w=_get(cg, nw.NW_ARR_W, (N, 3), 'f4'),
                 dist=_get(cg, nw.NW_ARR_DIST, (N,), 'f4'), res=_get(cg, nw.NW_ARR_RES, (N, 3), 'f4'), vacc=_get(cg, nw.NW_ARR_VACC, (M, 4), 'i8'),
                 pos=_get(cg, nw.NW_ARR_POS, (M, 3), 'f4'), meshpos=_get(cg, nw.NW_ARR_MESHPOS, (M, 3), 'f4'))
        if it == 0:
            out['nbr'] = _get(cg, nw.NW_ARR_NBR, (M, _nbytes(cg, nw.NW_ARR_NBR) // (4 * M)), 'i4')
            out['nrm'] = _get(cg, nw.NW_ARR_NRM, (M, 3), 'f4')
            out['valid'] = _get(cg, nw.NW_ARR_VALID, (M,), 'u1').astype(bool)
        ex.directions()
        B = dict(S=_get(cg, nw.NW_ARR_S, (M, 3, 3), 'f4'), pi=_get(cg, nw.NW_ARR_PI, (M,), 'f4'), fdef=_get(cg, nw.NW_ARR_FDEF, (M, 3), 'f4'),
                 parts=_get(cg, nw.NW_ARR_SCALARS, (_nbytes(cg, nw.NW_ARR_SCALARS) // 8,), 'f8'), vacc=_get(cg, nw.NW_ARR_VACC, (M, 4), 'i8'))
        ex.update()
        C = dict(pos=_get(cg, nw.NW_ARR_POS, (M, 3), 'f4'), meshpos=_get(cg, nw.NW_ARR_MESHPOS, (M, 3), 'f4'), S=_get(cg, nw.NW_ARR_S, (M, 3, 3), 'f4'),
                 vacc=_get(cg, nw.NW_ARR_VACC, (M, 4), 'i8'))
        out['iters'].append(dict(A=A, B=B, C=C))
    n_before = len(cg.iter_logs)
    ex.end()                                  # raises on any status other than NW_OK
    out['logs'] = cg.iter_logs[n_before:]
    assert cg.loopcount == n_iters and len(out['logs']) == n_iters
    return out


def _work_items(cg):
    """the query's work list (nw_debug, what = 1): (n_items, 2) {first localization in sorted order, count}; one wave per item"""
    cap = 1 << 16
    items = np.zeros(2 * cap, 'i4')
    n = ctypes.c_int(0)
    cg._native.check(cg._L.nw_debug(cg._h, 1, items.ctypes.data_as(ctypes.c_void_p), None, cap, ctypes.byref(n)))
    return items[:2 * min(n.value, cap)].reshape(-1, 2)


def _weights_on_device(sigma_inv, weights, N):
    """k_point_gather: weights / float32(float64 sum / 3N) and the mask bits (weight > 0).  The float64 sum of these few thousand float32
    values is exact whatever its order, so the mean is the device's."""
    src = np.ascontiguousarray(sigma_inv if weights is None else weights, 'f4').reshape(N, 3)
    mean = np.float32(float(src.astype('f8').sum()) / (3.0 * N))
    return (src / mean).astype('f4'), src > 0


# ---- the assertions of one run --------------------------------------------------------------------------------------------------------------
def _nearest_reference(pos, faces, pts):
    """nearest centroid, and whether the float64 margin to the second nearest exceeds 1e-6 relative"""
    from oracle import nanowrap_oracle as O
    cent = R.face_centroids32(pos, faces)
    best = np.empty(pts.shape[0], np.int64)
    clear = np.empty(pts.shape[0], bool)
    c8 = cent.astype('f8')
    for s in range(0, pts.shape[0], 512):
        d = np.sqrt(((pts[s:s + 512, None, :].astype('f8') - c8[None]) ** 2).sum(2))
        two = np.partition(d, 1, axis=1)[:, :2]
        best[s:s + 512] = d.argmin(1)
        clear[s:s + 512] = (two[:, 1] - two[:, 0]) > 1e-6 * two[:, 0]
    _, brute = O.nearest_faces(cent, pts, brute=True)
    assert np.array_equal(brute[clear], best[clear])
    return brute, clear


def check_run(run, faces, pts, sigma_inv, weights=None, data=None, wfunc=False, rows_and_scatter=True, label=''):
    """(a)-(e) on every iteration of one run; returns the figures it printed"""
    N, M = pts.shape[0], run['nbr'].shape[0]
    wnorm, mask = _weights_on_device(sigma_inv, weights, N)
    sinv = np.ascontiguousarray(sigma_inv, 'f4').reshape(N, 3)
    nbr, nrm, valid, q, qw = run['nbr'], run['nrm'], run['valid'], run['q'], run['qw']
    fig = dict(w=0.0, dist=0.0, res=0.0, fdef=0.0, sums=0.0, w_bits=0, res_bits=0, res_bits_oracle=0, excluded=0.0, max_x=0)
    for it, (snap, log) in enumerate(zip(run['iters'], run['logs'])):
        A, B, C = snap['A'], snap['B'], snap['C']
        ns = 2 if it == 0 else 3
        assert int(log['n_search']) == ns
        if rows_and_scatter:
            # ---- (a)
            ref_face, clear = _nearest_reference(A['pos'], faces, pts)
            assert (~clear).mean() <= 0.01, 'too many points without a clear nearest face: %.3f' % (~clear).mean()
            assert np.array_equal(A['face'][clear], ref_face[clear]), 'nearest faces differ from the brute-force reference'
            rows = R.attract_rows(A['pos'], faces, A['face'], pts, data, sinv, wnorm, mask)
            rw, rd, rr = R.check_rows(rows, A['vidx'], A['w'], A['dist'], A['res'], faces, A['face'])
            fig['w'], fig['dist'], fig['res'] = max(fig['w'], rw), max(fig['dist'], rd), max(fig['res'], rr)
            fig['excluded'] = max(fig['excluded'], float((~clear).mean()))
            fig['w_bits'] += int((A['w'].view('u4') != rows['w32'].view('u4')).sum())
            fig['res_bits'] += int((A['res'].view('u4') != rows['res32'].view('u4')).sum())
            fig['res_bits_oracle'] += int((A['res'].view('u4') != rows['res32_d64'].view('u4')).sum())
            # (no bit differed on an MI355X in any scene: asserted from then on.  The restatement's float32 weights ARE the oracle's, bit for
            # bit -- tests/test_fit_stages_ref.py; its residual differs from the oracle's in the last bit where the float32 distance does)
            assert np.array_equal(A['w'].view('u4'), rows['w32'].view('u4')), 'weights differ in bits from the float32 restatement (= the oracle)'
            assert np.array_equal(A['res'].view('u4'), rows['res32'].view('u4')), 'residuals differ in bits from the float32 restatement'
            # ---- (b)
            table, S0, pi = R.check_scatter(A['vacc'], A['vidx'], A['w'], A['res'], q, qw, M)
            fig['max_x'] = max(fig['max_x'], int(np.abs(R.quantise(A['w'], A['res'], q, qw)).max()))
            assert np.array_equal(B['vacc'], A['vacc'])
            assert np.array_equal(B['S'][:, :, 0].view('u4'), S0.view('u4')), 'S0 is not float32(sum * q)'
            assert np.array_equal(B['pi'].view('u4'), pi.view('u4')), 'pi is not sqrtf(3 (sum w)^2) of the accumulator'
            unfed = np.ones(M, bool)
            unfed[A['vidx'].ravel()] = False
            assert (B['pi'][unfed] == 0).all() and (B['S'][unfed][:, :, 0] == 0).all()
        assert not C['vacc'].any(), 'the accumulator is not zero after the update'
        # ---- (c)
        wv = R.vertex_area_weights(A['pos'], nbr) if wfunc else None
        pr = R.prior(A['meshpos'], A['pos'], nrm, nbr, B['pi'], wv)
        bf = 2 * U * np.maximum(np.maximum(np.abs(pr['fdef64']), np.abs(pr['vc'])), np.abs(pr['alpha'])[:, None])
        rf = R.ratio(np.abs(B['fdef'].astype('f8') - pr['fdef64']), bf)
        fig['fdef'] = max(fig['fdef'], rf)
        assert rf <= 1.0, 'fdef: max err/bound %.3f' % rf
        lo, hi = R.s1_candidates(pr, A['pos'], wv)
        s1 = B['S'][:, :, 1]
        assert ((s1 >= lo) & (s1 <= hi)).all(), 'S1 is not -float32(prefs64) at %d entries' % int((~((s1 >= lo) & (s1 <= hi))).sum())
        iso = pr['isolated']
        assert (B['pi'][iso] == 0).all() and np.array_equal(B['fdef'][iso], A['meshpos'][iso]) and (s1[iso] == 0).all()
        # ---- (d)
        ref = R.scalars(B['S'], A['w'], A['vidx'], A['res'], mask, A['pos'], B['fdef'], A['dist'], ns, wv, slots=SL)
        got, worst = R.check_sums(B['parts'], ref, SL)
        fig['sums'] = max(fig['sums'], worst)
        assert got[SL['NPTS']] == N and got[SL['MAXD']] == float(A['dist'].max())
        assert got[SL['STATUS']] == 0
        if not wfunc:
            assert got[SL['T']] == got[SL['SS']] and got[SL['T'] + 1] == got[SL['SS'] + 1] and got[SL['T'] + 2] == got[SL['SS'] + 3]
        # ---- (e)
        sol = R.small_solve(got, np.float32(LAMS[0]), ns, slots=SL)
        assert not sol['singular']
        assert np.array_equal(np.asarray(log['H'], 'f8'), sol['H'].astype('f8')), 'H of the log differs in bits'
        assert np.array_equal(np.asarray(log['G'], 'f8'), sol['G'].astype('f8')), 'G of the log differs in bits'
        assert np.array_equal(np.asarray(log['c'], 'f8'), sol['c'].astype('f8')), 'c of the log differs in bits'
        R.check_update(A['pos'], B['S'], sol['c'], valid, 0, A['meshpos'], ns, C['pos'], C['S'], C['meshpos'])
        assert np.array_equal(C['S'][:, :, :2].view('u4'), B['S'][:, :, :2].view('u4'))
        cpred, wpred = R.predictions(got, sol, ns, SL)
        assert abs(log['cpred'] - cpred) <= 1e-12 * abs(cpred) and abs(log['wpred'] - wpred) <= 1e-12 * abs(wpred)
        assert log['res_norm'] == np.sqrt(got[SL['RES2']]) and log['prefs_norm'] == np.sqrt(got[SL['PP32']])
        rel = float(np.abs(sol['c'].astype('f8') - sol['c64']).max() / np.abs(sol['c64']).max())
        print('%s it %d: |c - c64|/|c64| = %.2e, cond(H) u = %.2e' % (label, it, rel, sol['cond'] * U))
    print('%s: max err/bound w %.3f dist %.3f res %.3f fdef %.3f sums %.3f; bits differing from the float32 restatement: w %d, res %d '
          '(res against the oracle\'s float64-distance form: %d); unclear nearest faces %.2f %%; max |x| %.3g quanta (guard 7e13)'
          % (label, fig['w'], fig['dist'], fig['res'], fig['fdef'], fig['sums'], fig['w_bits'], fig['res_bits'], fig['res_bits_oracle'],
             100 * fig['excluded'], fig['max_x']))
    return fig


def _fit(v, f, pts, sigma_inv, separate, weights=None, data=None, n_iters=2, max_vertices=None, invalid=None, wfunc=False):
    """a fresh optimiser, one block phase by phase; separate: k_attract as its own launch in every iteration (else the workgroups appended
    to the query launch take over from the second iteration on)"""
    from ch_shrinkwrap_amd.trimesh import TriMesh
    from ch_shrinkwrap_amd.mesh_conj_grad import ShrinkwrapMeshConjGrad
    mesh = TriMesh(v.copy(), f, max_vertices=max_vertices)
    cg = ShrinkwrapMeshConjGrad(mesh, pts)
    if invalid is not None:                   # vertex slots in use whose mesh positions must not follow the estimate
        cg._mesh_vertex_mask = cg._mesh_vertex_mask.copy()
        cg._mesh_vertex_mask[invalid] = False
        cg._upload_mesh()
    if wfunc:
        cg.Lfuncs, cg.Lhfuncs = ['wfunc'], ['wfunc']
    cg.separate_attraction(separate)
    run = run_stages(cg, n_iters, pts, sigma_inv, weights, data)
    return cg, mesh, run


def _both_paths(v, f, pts, sigma_inv, label, **kw):
    check = {k: kw.pop(k) for k in list(kw) if k in ('rows_and_scatter',)}
    figs = []
    for separate in (True, False):
        cg, mesh, run = _fit(v, f, pts, sigma_inv, separate, **kw)
        figs.append(check_run(run, np.asarray(mesh.faces), pts, sigma_inv, weights=kw.get('weights'), data=kw.get('data'), wfunc=kw.get('wfunc', False),
                              label='%s [%s]' % (label, 'k_attract' if separate else 'in the query launch'), **check))
        if 'invalid' in kw:
            assert not run['valid'][kw['invalid']].any()
        last = (cg, mesh, run)
    return figs, last


# ---- 1. counts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025])
def test_counts_around_rows_waves_and_workgroups(N):
    """icosphere(2), 162 vertices; N localizations 2-8 nm off the sphere around every boundary of the scatter's grouping: a row of 16 lanes
    (the segmented scan), a wave of 64 (one work item), a workgroup of 256 (one table), and one more."""
    v, f = _jittered_icosphere(2, seed=11)
    pts = _shell_points(N, 100.0, 100 + N)
    _both_paths(v, f, pts, _sigma_inv(N, 200 + N), 'counts N=%d' % N)


# ---- 2. runs --------------------------------------------------------------------------------------------------------------------------------
def test_one_run_across_rows_waves_and_workgroups():
    """600 localizations nearest to the SAME face: whatever their order, every row of 16 lanes is one run, and the face's three vertices
    receive all 600 contributions through every level (run sums, table, flush)."""
    v, f = _jittered_icosphere(2, seed=12)
    pts = _over_faces(v, f, np.full(600, 37), 31, spread=0.03)
    figs, (cg, mesh, run) = _both_paths(v, f, pts, _sigma_inv(600, 32), 'one run of 600')
    for snap in run['iters']:
        assert (snap['A']['face'] == 37).all()
        assert (snap['A']['vacc'][:, 3] != 0).sum() == 3


def test_runs_of_every_length_across_row_boundaries():
    """600 localizations in blocks of 1, 2, 3, 15, 16, 17, 33 per face.  The localizations of a block share their coordinates (they differ in
    their sigmas, hence in their residuals), so they share their Morton key and the stable sort keeps them together: runs of 17 and 33
    lanes with the same face exist in the sorted order by construction, starting at every offset inside a row of 16."""
    v, f = _jittered_icosphere(2, seed=13)
    sizes = []
    while sum(sizes) < 600:
        sizes += [1, 2, 3, 15, 16, 17, 33]
    sizes[-1] -= sum(sizes) - 600
    sizes = [s for s in sizes if s > 0]
    strip = np.argsort(np.arctan2(v[f].mean(1)[:, 1], v[f].mean(1)[:, 0]) + 10.0 * (np.abs(v[f].mean(1)[:, 2]) > 25.0))[:len(sizes)]   # faces round the equator
    one = _over_faces(v, f, strip, 41, spread=0.05)
    block = np.repeat(np.arange(len(sizes)), sizes)
    pts = np.ascontiguousarray(one[block])
    assert pts.shape[0] == 600 and max(sizes) >= 17
    figs, (cg, mesh, run) = _both_paths(v, f, pts, _sigma_inv(600, 42), 'runs of every length')
    for snap in run['iters']:
        face = snap['A']['face']
        for b in np.nonzero(np.array(sizes) >= 17)[0]:
            assert np.unique(face[block == b]).size == 1           # a run of >= 17 equal faces among equal keys
    # the same localization 33 times over gives 33 different residuals (different sigmas): the run sums add different integers
    assert np.unique(run['iters'][0]['A']['res'][block == int(np.argmax(sizes))], axis=0).shape[0] > 1


# ---- 3. hot vertex --------------------------------------------------------------------------------------------------------------------------
def test_thousands_of_contributions_to_one_vertex():
    """5 000 localizations over the five or six faces round one vertex of icosphere(1): thousands of contributions to one accumulator row, from
    every workgroup.  Its sum of weights must be exact in units of 2^-40 (part of the accumulator's equality)."""
    v, f = _jittered_icosphere(1, seed=14)
    fan = np.nonzero((f == 5).any(1))[0]
    assert 5 <= fan.size <= 6
    rng = np.random.default_rng(51)
    pts = _over_faces(v, f, rng.choice(fan, 5000), 52, spread=0.15)
    figs, (cg, mesh, run) = _both_paths(v, f, pts, _sigma_inv(5000, 53), 'hot vertex')
    A = run['iters'][1]['A']
    hot = int((A['vidx'] == 5).sum())
    x = R.quantise(A['w'], A['res'], run['q'], run['qw'])
    print('hot vertex: %d contributions to one row, sum w = %d x 2^-40' % (hot, A['vacc'][5, 3]))
    assert hot >= 4500 and A['vacc'][5, 3] == int(x[:, :, 3][A['vidx'] == 5].sum())


# ---- 4. table overflow ----------------------------------------------------------------------------------------------------------------------
def test_table_overflow_goes_to_memory_and_changes_nothing():
    """icosphere(5), 768 localizations over 768 pairwise vertex-disjoint faces: any 256 of them touch 768 distinct vertices, more than the 512
    slots of k_attract's table -- every workgroup must send contributions straight to memory (pigeonhole).  In the query launch a workgroup
    is two consecutive work items with a table of 256 slots: more than 85 localizations in a pair would force the same there.  Below
    589 824 localizations the work list is cut at 32 per item (build_items), so a pair holds 64 at most, 192 vertices: that table cannot
    be FORCED to overflow by a scene of test size (measured here: 56 items, largest pair 38); the item list is read and the figure printed."""
    v, f = _jittered_icosphere(5, seed=15, jitter=0.05)
    assert v.shape[0] == 10242 and f.shape[0] == 20480
    assert _disjoint_faces(f, 1 << 30).size == 2562
    chosen = _disjoint_faces(f, 768)
    assert np.unique(f[chosen]).size == 3 * 768
    pts = (v[f[chosen]].astype('f8').mean(1) * 1.01).astype('f4')           # 1 % outside each centroid
    figs, (cg, mesh, run) = _both_paths(v, f, pts, _sigma_inv(768, 61), 'table overflow')
    for snap in run['iters']:
        assert np.array_equal(snap['A']['face'], chosen)
        assert np.unique(snap['A']['vidx']).size == 3 * 768                 # 256 localizations of any workgroup: 768 vertices > 512 slots
        assert (snap['B']['pi'] == 0).sum() == 10242 - 3 * 768
    items = _work_items(cg)
    assert items[:, 1].sum() == 768
    pairs = items[:2 * (items.shape[0] // 2), 1].reshape(-1, 2).sum(1)
    forced = int((pairs > 85).sum())
    print('table overflow: k_attract: 3 workgroups x 768 distinct vertices for 512 slots (forced); in the query launch: %d work items, '
          'largest pair %d localizations = %d vertices for 256 slots: %s'
          % (items.shape[0], int(pairs.max()) if pairs.size else 0, 3 * int(pairs.max()) if pairs.size else 0,
             '%d workgroups forced to spill' % forced if forced else 'this scene did not force a spill there'))


# ---- 5. open patch with spare slots ---------------------------------------------------------------------------------------------------------
def _open_patch():
    v, f = _plane_patch(20, 13)
    pts = _over_plane(900, (5.0, 5.0), (90.0, 115.0), 71)                    # one half only
    rng = np.random.default_rng(72)
    weights = rng.uniform(0.5, 1.5, size=(900, 3)).astype('f4')
    weights[rng.uniform(size=(900, 3)) < 0.15] = 0.0
    invalid = np.array([0, 7, 19, 40, 77, 130, 131, 200, 246, 259])
    return v, f, pts, weights, invalid


def test_open_patch_with_spare_slots_invalid_vertices_and_masked_weights():
    """A 20 x 13 plane strip (valences 2, 3, 4, 6; -1 padded rings), 7 unused vertex slots, 10 vertices whose mesh positions must not follow,
    900 localizations over one half, explicit weights with 15 % zeros (the mask bits).  pi on both sides of 1, mesh positions against the
    estimate."""
    v, f, pts, weights, invalid = _open_patch()
    figs, (cg, mesh, run) = _both_paths(v, f, pts, _sigma_inv(900, 73), 'open patch', weights=weights, max_vertices=v.shape[0] + 7, invalid=invalid)
    deg = (run['nbr'] >= 0).sum(1)
    # (the ring table lists an open fan's OUTGOING half-edges only: boundary vertices of valence 2, 3, 4 have rings of 1, 2, 3 entries)
    assert set(np.unique(deg)) == {0, 1, 2, 3, 6} and (deg == 0).sum() == 7
    pi = run['iters'][0]['B']['pi']
    assert ((pi > 0) & (pi < 1)).any() and (pi > 1).any() and (pi == 0).sum() > 100
    C = run['iters'][1]['C']
    moved = (C['pos'] != C['meshpos']).any(1)
    assert moved[invalid].all() and not moved[np.setdiff1d(np.arange(260), invalid)].any()


def test_open_patch_with_the_wfunc_regulariser():
    """the same scene with regulariser 'wfunc': the wv branches of the prior and of the vertex-side sums"""
    v, f, pts, weights, invalid = _open_patch()
    cg, mesh, run = _fit(v, f, pts, _sigma_inv(900, 73), False, weights=weights, max_vertices=v.shape[0] + 7, invalid=invalid, wfunc=True)
    check_run(run, np.asarray(mesh.faces), pts, _sigma_inv(900, 73), weights=weights, wfunc=True, label='open patch, wfunc')


# ---- 6. residual larger than the scene ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['data_3_extents_away', 'offset_1e6'])
def test_residuals_larger_than_the_scene_and_large_coordinates(case):
    """The quantum is derived from (scene extent x largest weight), not from |data - A f|: a residual target three extents away must leave
    the status NW_OK (run_stages raises otherwise) and the scatter exact; so must a scene whose coordinates are 10^6 (float32 spacing 1/16)."""
    v, f = _jittered_icosphere(2, seed=11)
    pts = _shell_points(1025, 100.0, 100 + 1025)
    data = None
    if case == 'data_3_extents_away':
        data = (pts + 3.0 * float((pts.max(0) - pts.min(0)).max())).astype('f4')
    else:
        v, pts = (v + np.float32(1e6)).astype('f4'), (pts + np.float32(1e6)).astype('f4')
    figs, _ = _both_paths(v, f, pts, _sigma_inv(1025, 200 + 1025), case, data=data)
    assert max(g['max_x'] for g in figs) < 7.0e13


# ---- 7. reduction shapes --------------------------------------------------------------------------------------------------------------------
def test_more_partial_sum_rows_than_parts():
    """N = 33 * 256 + 1 on icosphere(3): 34 rows of k_attract's partial sums over 32 parts, the subspace kernel's blocks of 1024 with a tail"""
    v, f = _jittered_icosphere(3, seed=16)
    N = 33 * 256 + 1
    pts = _shell_points(N, 100.0, 81)
    _both_paths(v, f, pts, _sigma_inv(N, 82), 'N=%d' % N)


def test_more_vertices_than_the_vertex_kernels_have_threads():
    """A 363 x 364 plane patch: 132 132 vertices, more than the 512 x 256 threads k_prior_directions and k_solve_update are capped at (the
    grid-stride tail of the first, the second prefetched vertex of the other).  5 000 localizations, one iteration, (c)-(e) only."""
    import time
    t0 = time.perf_counter()
    v, f = _plane_patch(363, 364, seed=17)
    assert v.shape[0] > 512 * 256 + 256
    pts = _over_plane(5000, (100.0, 100.0), (3500.0, 3500.0), 91)
    s = _sigma_inv(5000, 92)
    cg, mesh, run = _fit(v, f, pts, s, True, n_iters=1)
    t1 = time.perf_counter()
    check_run(run, np.asarray(mesh.faces), pts, s, rows_and_scatter=False, label='132 132 vertices')
    print('132 132 vertices: mesh + fit %.1f s, checks %.1f s' % (t1 - t0, time.perf_counter() - t1))
