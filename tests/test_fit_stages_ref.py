"""
CPU tests of tests/fit_stages_ref.py, the stage-by-stage restatement tests/test_hip_fit_stages.py checks the iteration kernels against: the
restatement is pinned to oracle/nanowrap_oracle.py before anything trusts it, the integer scatter is shown to be what it claims (independent
of the order of the points; equal to a plain Python-integer loop), and every assertion the GPU test relies on is shown to turn red on a
snapshot that is wrong in one small way (the mutations at the end).

Each stage is fed the ORACLE's own inputs to that stage (its trace), as the GPU test feeds the device's own: nothing drifts, and each bound
is the restatement's derived bound plus the oracle's own rounding error, which is stated where it is used.
"""
import numpy as np
import pytest

from conftest import load_golden
import fit_stages_ref as R
from oracle import nanowrap_oracle as O

U = R.U32
SL = R.scalar_slots()


def _quantum(pts, pos, wnorm):
    """the library's rule: 2^-36 of (scene extent x largest weight), a power of two"""
    allp = np.concatenate([pts, pos])
    ext = float((allp.max(0) - allp.min(0)).max())
    return 2.0 ** (int(np.ceil(np.log2(ext * float(np.abs(wnorm).max())))) - 36), 2.0 ** -40


def _small_case():
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    from ch_shrinkwrap_amd.synth import sphere_cloud
    v, f = icosphere(2, 105.0)
    mesh = TriMesh(v, f)
    pts = sphere_cloud(500, 100.0, 4.0, seed=21)
    rng = np.random.default_rng(22)
    sigma = rng.uniform(5.0, 15.0, size=pts.shape).astype('f4')
    valid = np.ones(v.shape[0], bool)
    valid[[3, 50, 161]] = False
    return dict(vertices=mesh.vertices.copy(), faces=mesh.faces, normals=mesh.vertex_normals.copy(), nbr=mesh.neighbor_vertex_table(),
                points=pts, sigma=sigma, lams=np.array([10.0]), valid=valid)


def _golden_case():
    g = load_golden('stages_642')
    return dict(vertices=g['vertices'], faces=g['faces'], normals=g['normals'], nbr=g['nbr'], points=g['points'], sigma=g['sigma'],
                lams=g['lams'], valid=g['valid'])


_CASES = {'small_162': _small_case, 'stages_642': _golden_case}
_TRACES = {}


def _traced(name):
    """one oracle run per case, shared by the tests and never modified"""
    if name not in _TRACES:
        c = _CASES[name]()
        s = (1.0 / c['sigma'].ravel()).astype('f4')
        trace = []
        out = O.search(c['vertices'].copy(), c['normals'], c['nbr'], c['faces'], c['points'], [float(c['lams'][0])], 3, s, valid=c['valid'],
                       trace=trace, brute_nn=True)
        assert out.loopcount == 3
        _TRACES[name] = (c, s, trace)
    return _TRACES[name]


def test_scalar_slots_come_from_the_header():
    assert SL['COUNT'] == 29
    assert SL['T'] == SL['SS'] + 11
    assert SL['HC'] == 4 and SL['GC'] == SL['HC'] + 6 and SL['SP'] == SL['SS'] + 6 and SL['MAXD'] == SL['COUNT'] - 1
    # 28 slots carry sums (the status slot is the 29th)
    assert 4 + 6 + 3 + 6 + 3 + 1 + 1 + 3 + 1 == 28


@pytest.mark.parametrize('name', sorted(_CASES))
def test_stage_functions_reproduce_the_oracle(name):
    c, s, trace = _traced(name)
    pts, faces, nrm, nbr, valid = c['points'], c['faces'], c['normals'], c['nbr'], c['valid'].astype(bool)
    M, N = c['vertices'].shape[0], pts.shape[0]
    wn = (s / s.mean()).reshape(N, 3)                 # the oracle's normalisation (float32 mean)
    mask = (s > 0).reshape(N, 3)
    f0 = c['vertices'].astype('f4').copy()
    cur = f0.copy()
    q, qw = _quantum(pts, f0, wn)
    for it, t in enumerate(trace):
        ns = int(t['n_search'])
        # ---- rows
        rows = R.attract_rows(f0, faces, t['face'], pts, None, s.reshape(N, 3), wn, mask)
        rw, rd, rr = R.check_rows(rows, t['v_idx'], t['w'], t['dmean'], t['res'].reshape(N, 3), faces, t['face'])
        nbw = int((rows['w32'].view('u4') != np.asarray(t['w'], 'f4').view('u4')).sum())
        nbr_ = int((rows['res32'].view('u4') != t['res'].reshape(N, 3).view('u4')).sum())
        nb64 = int((rows['res32_d64'].view('u4') != t['res'].reshape(N, 3).view('u4')).sum())
        print('%s it %d: max err/bound w %.3f dist %.3f res %.3f; float32 restatement differs from the oracle in bits at %d weights, %d residuals'
              ' (%d with the float64 distance the oracle keeps)' % (name, it, rw, rd, rr, nbw, nbr_, nb64))
        assert nbw == 0 and nb64 == 0           # the same float32 operations in the same order
        assert np.abs(rows['res32'].view('i4').astype('i8') - t['res'].reshape(N, 3).view('i4').astype('i8')).max() <= 1      # (float32 distance: last bit)
        # ---- scatter: the oracle's serial float32 sums are within deg u sum|terms| of the exact sums; the fixed-point ones within deg q/2
        table, S0, pi = R.scatter_exact(t['v_idx'], t['w'], t['res'], q, qw, M)
        deg, a, sw = R.scatter_abs(t['v_idx'], t['w'], t['res'], M)
        S_or = t['S'].reshape(M, 3, -1)
        b0 = deg[:, None] * U * a + deg[:, None] * q / 2 + U * np.abs(S0.astype('f8'))
        assert R.ratio(np.abs(S0.astype('f8') - S_or[:, :, 0]), b0) <= 1.0
        assert (np.abs(S0.astype('f8') - S_or[:, :, 0]) > 0).any() or N < 10        # (the two are not the same computation)
        bpi = np.sqrt(3.0) * (deg * U * sw + deg * qw / 2) + 6 * U * pi.astype('f8')     # sw's error through sqrt(3 sw^2): three roundings + sqrtf, each side
        assert R.ratio(np.abs(pi.astype('f8') - t['pi']), bpi) <= 1.0
        # ---- prior, from the oracle's pi
        pr = R.prior(cur, f0, nrm, nbr, t['pi'])
        fd_or = t['fdef'].reshape(M, 3)
        bf = 2 * U * np.maximum(np.maximum(np.abs(pr['fdef64']), np.abs(pr['vc'])), np.abs(pr['alpha'])[:, None])
        assert R.ratio(np.abs(pr['fdef64'] - fd_or), bf) <= 1.0
        lo, hi = R.s1_candidates(pr, f0)
        s1 = S_or[:, :, 1]
        assert ((s1 >= lo) & (s1 <= hi)).all()
        assert (lo == hi).mean() > 0.99
        assert np.array_equal(pr['fdef64'][pr['isolated']], cur[pr['isolated']].astype('f8'))
        # ---- the sums, from the oracle's S, w, res, fdef (float64: no rounding of fdef to propagate)
        S_full = np.zeros((M, 3, 3), 'f4')
        S_full[:, :, :S_or.shape[2]] = S_or
        val, ab, bnd = R.scalars(S_full, t['w'], t['v_idx'], t['res'], mask, f0, fd_or, t['dmean'].astype('f4'), ns, slots=SL)
        nm = int(mask.sum())
        for i in range(ns):
            for j in range(ns):
                k = R._tri(i, j)
                # np.dot of float32 arrays: error <= n u sum|terms| whatever the order (n terms)
                assert abs(t['Hc'][i, j] - val[SL['HC'] + k]) <= nm * U * ab[SL['HC'] + k] + bnd[SL['HC'] + k]
                assert abs(t['Hw'][i, j] - val[SL['SS'] + k]) <= 3 * M * U * ab[SL['SS'] + k] + bnd[SL['SS'] + k]
            assert abs(t['Gc'][i] - val[SL['GC'] + i]) <= nm * U * ab[SL['GC'] + i] + bnd[SL['GC'] + i]
            # Gw: a float64 dot of float32(-S) and the float64 prefs
            assert abs(-t['Gw'][i] - val[SL['SP'] + i]) <= 2 * bnd[SL['SP'] + i]
        assert abs(t['c0'] - val[SL['C0']]) <= nm * U * ab[SL['C0']]                  # float32 sum of float32 squares
        # ---- the small system, from the oracle's own matrices
        sc = np.zeros(SL['COUNT'])
        for i in range(ns):
            for j in range(ns):
                sc[SL['HC'] + R._tri(i, j)] = t['Hc'][i, j]
                sc[SL['SS'] + R._tri(i, j)] = t['Hw'][i, j]
            sc[SL['GC'] + i] = t['Gc'][i]
            sc[SL['SP'] + i] = -t['Gw'][i]
        sol = R.small_solve(sc, np.float32(c['lams'][0]), ns, slots=SL)
        assert not sol['singular']
        assert np.array_equal(sol['H'][:ns, :ns], t['H']) and np.array_equal(sol['G'][:ns], t['G'])
        # Gaussian elimination with partial pivoting is backward stable: |dA| <= n^2 (3n u) 2^(n-1) |A| (Higham, Accuracy and Stability,
        # theorem 9.5 with the growth factor's bound), so each of the two float32 solutions (this one divides by the pivot, LAPACK's sgetf2
        # multiplies by its reciprocal) is within cond_inf times that of the exact one
        cond = float(np.linalg.cond(sol['H'][:ns, :ns].astype('f8'), np.inf))
        bc = 2 * (3 * ns ** 3 * 2 ** (ns - 1)) * U * cond * float(np.abs(sol['c64']).max())
        assert np.abs(sol['c'][:ns].astype('f8') - t['c']).max() <= bc
        assert np.abs(sol['c'][:ns].astype('f8') - sol['c64'][:ns]).max() <= bc
        # ---- update, from the oracle's c
        c3 = np.zeros(3, 'f4')
        c3[:ns] = t['c']
        fn, s2, mp = R.update(f0, S_full, c3, valid, 0, cur, ns)
        mag = np.abs(f0.astype('f8')) + (np.abs(S_full.astype('f8')) * np.abs(c3.astype('f8'))).sum(2)
        assert R.ratio(np.abs(fn.astype('f8') - t['fnew'].reshape(M, 3)), (ns + 2) * U * mag) <= 1.0
        # next iteration starts from the ORACLE's state
        f1 = t['fnew'].reshape(M, 3).astype('f4')
        assert np.array_equal(mp[~valid], cur[~valid])
        cur = np.where(valid[:, None], f1, cur)
        f0 = f1


def _scatter_inputs(n=200, M=37, seed=5):
    rng = np.random.default_rng(seed)
    vidx = np.stack([rng.permutation(M)[:3] for _ in range(n)]).astype('i4')
    w = rng.uniform(0.05, 1.0, size=(n, 3)).astype('f4')
    w = (w / w.sum(1)[:, None]).astype('f4')
    res = (rng.normal(size=(n, 3)) * 30).astype('f4')
    res[::17] = 0.0
    return vidx, w, res


def test_scatter_is_independent_of_the_order_of_the_points():
    vidx, w, res = _scatter_inputs(3000, 61, 8)
    q, qw = 2.0 ** -28, 2.0 ** -40
    ref = R.scatter_exact(vidx, w, res, q, qw, 61)[0]
    rng = np.random.default_rng(9)
    for _ in range(5):
        p = rng.permutation(vidx.shape[0])
        assert np.array_equal(R.scatter_exact(vidx[p], w[p], res[p], q, qw, 61)[0], ref)


def test_scatter_equals_a_python_integer_loop():
    vidx, w, res = _scatter_inputs(200, 37, 5)
    q, qw = 2.0 ** -27, 2.0 ** -40
    table = R.scatter_exact(vidx, w, res, q, qw, 37)[0]
    slow = R.scatter_slow(vidx, w, res, q, qw, 37)
    assert [[int(x) for x in row] for row in table] == slow


def test_the_add_and_subtract_rounding_is_half_to_even():
    """nw_round_to_i64 adds 1.5 * 2^52 and reads the low mantissa bits: np.rint on 10^5 random values and on the .5 cases"""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(size=100000) * 10.0 ** rng.uniform(-3, 13, size=100000), np.arange(-2000, 2000) + 0.5, [0.0, -0.0, 2.0 ** 50 + 0.5]])
    magic = 6755399441055744.0
    got = (x + magic).view(np.int64) - np.int64(0x4338000000000000)
    assert np.array_equal(got, np.rint(x).astype(np.int64))


# ---- mutations: a snapshot (or a scratch copy of the restatement) that is wrong in one small way turns an assertion red -----------------
def _snapshot():
    """what a correct device would hold after the first iteration of the small case: the restatement's own outputs"""
    c, s, trace = _traced('small_162')
    t = trace[0]
    pts, faces = c['points'], c['faces']
    M, N = c['vertices'].shape[0], pts.shape[0]
    wn = (s / s.mean()).reshape(N, 3)
    mask = (s > 0).reshape(N, 3)
    f0 = c['vertices'].astype('f4')
    q, qw = _quantum(pts, f0, wn)
    rows = R.attract_rows(f0, faces, t['face'], pts, None, s.reshape(N, 3), wn, mask)
    vacc, S0, pi = R.scatter_exact(rows['vidx'], rows['w32'], rows['res32'], q, qw, M)
    pr = R.prior(f0, f0, c['normals'], c['nbr'], pi)
    S = np.zeros((M, 3, 3), 'f4')
    S[:, :, 0], S[:, :, 1] = S0, pr['S1']
    fdef32 = pr['fdef64'].astype('f4')
    ref = R.scalars(S, rows['w32'], rows['vidx'], rows['res32'], mask, f0, fdef32, rows['dist32'], 2, slots=SL)
    return dict(c=c, rows=rows, vacc=vacc, q=q, qw=qw, M=M, N=N, S=S, ref=ref, f0=f0, face=t['face'], faces=faces)


def _parts_of(val, rng):
    """32 ordered parts per slot that add up to the slot's value (the last takes the remainder)"""
    parts = np.zeros((SL['COUNT'], R.NW_SPARTS))
    for s in range(SL['COUNT']):
        if s == SL['MAXD']:
            parts[s] = val[s] * rng.uniform(0.2, 1.0, R.NW_SPARTS)
            parts[s, 11] = val[s]
            continue
        if s == SL['NPTS']:                            # whole localizations per part
            parts[s, :] = int(val[s]) // R.NW_SPARTS
            parts[s, 0] += int(val[s]) % R.NW_SPARTS
            continue
        share = rng.uniform(0.5, 1.5, R.NW_SPARTS)
        parts[s] = val[s] * share / share.sum()
    return parts


def test_the_unmutated_snapshot_passes():
    sn = _snapshot()
    r = sn['rows']
    R.check_rows(r, r['vidx'], r['w32'], r['dist32'], r['res32'], sn['faces'], sn['face'])
    R.check_scatter(sn['vacc'], r['vidx'], r['w32'], r['res32'], sn['q'], sn['qw'], sn['M'])
    R.check_sums(_parts_of(sn['ref'][0], np.random.default_rng(1)), sn['ref'], SL)


def test_mutation_one_dropped_contribution_is_caught():
    sn = _snapshot()
    r = sn['rows']
    x = R.quantise(r['w32'], r['res32'], sn['q'], sn['qw'])
    bad = sn['vacc'].copy()
    bad[r['vidx'][7, 1]] -= x[7, 1]                   # point 7's contribution to its second corner never arrived
    with pytest.raises(AssertionError, match='accumulator differs at 1 vertices'):
        R.check_scatter(bad, r['vidx'], r['w32'], r['res32'], sn['q'], sn['qw'], sn['M'])
    # ... even the smallest one: the weight column alone, one unit of 2^-40
    bad = sn['vacc'].copy()
    bad[r['vidx'][7, 1], 3] -= 1
    with pytest.raises(AssertionError, match='accumulator differs'):
        R.check_scatter(bad, r['vidx'], r['w32'], r['res32'], sn['q'], sn['qw'], sn['M'])


def test_mutation_two_corners_weights_swapped_is_caught():
    sn = _snapshot()
    r = sn['rows']
    w = r['w32'].copy()
    i = int(np.argmax(np.abs(w[:, 0] - w[:, 2])))
    w[i, 0], w[i, 2] = w[i, 2], w[i, 0]
    with pytest.raises(AssertionError, match='weights: max err/bound'):
        R.check_rows(r, r['vidx'], w, r['dist32'], r['res32'], sn['faces'], sn['face'])
    # the scatter a device with that slip would have made, against the rows it reports
    swapped = R.scatter_exact(r['vidx'], w, r['res32'], sn['q'], sn['qw'], sn['M'])[0]
    with pytest.raises(AssertionError, match='accumulator differs at 2 vertices'):
        R.check_scatter(swapped, r['vidx'], r['w32'], r['res32'], sn['q'], sn['qw'], sn['M'])


def test_mutation_half_up_instead_of_half_even_is_caught():
    q, qw = 2.0 ** -10, 2.0 ** -40
    k = np.arange(1, 41)
    res = np.zeros((40, 3), 'f4')
    res[:, 0] = (2 * k + 1) * q                      # w = 0.5: c / q = k + 0.5 exactly
    w = np.tile(np.array([0.5, 0.25, 0.25], 'f4'), (40, 1))
    vidx = np.tile(np.array([0, 1, 2], 'i4'), (40, 1))

    def half_up(x):
        return np.floor(x + 0.5)
    wrong = R.scatter_exact(vidx, w, res, q, qw, 3, rint=half_up)[0]
    assert wrong[0, 0] - R.scatter_exact(vidx, w, res, q, qw, 3)[0][0, 0] == 20        # every even k rounds the other way
    with pytest.raises(AssertionError, match='accumulator differs'):
        R.check_scatter(wrong, vidx, w, res, q, qw, 3)


def test_mutation_parts_out_of_order_with_one_omitted_is_caught():
    sn = _snapshot()
    rng = np.random.default_rng(2)
    parts = _parts_of(sn['ref'][0], rng)
    shuffled = parts[:, rng.permutation(R.NW_SPARTS)]
    R.check_sums(shuffled, sn['ref'], SL)             # the order alone is inside every bound (it is what the bound allows for)
    for slot in ('RES2', 'HC', 'GC', 'SS', 'SP', 'PP64', 'T'):
        bad = shuffled.copy()
        bad[SL[slot], 5] = 0.0
        with pytest.raises(AssertionError, match='sum SC_%s' % slot):
            R.check_sums(bad, sn['ref'], SL)
    bad = parts.copy()
    bad[SL['MAXD'], 11] = 0.0
    with pytest.raises(AssertionError, match='SC_MAXD'):
        R.check_sums(bad, sn['ref'], SL)


def test_mutation_mesh_position_written_at_an_invalid_vertex_is_caught():
    sn = _snapshot()
    c = sn['c']
    valid = c['valid'].astype(bool)
    cvec = np.array([0.01, 0.2, 0.0], 'f4')
    fn, s2, mp = R.update(sn['f0'], sn['S'], cvec, valid, 0, sn['f0'], 2)
    S_after = sn['S'].copy()
    S_after[:, :, 2] = s2
    R.check_update(sn['f0'], sn['S'], cvec, valid, 0, sn['f0'], 2, fn, S_after, mp)
    bad = mp.copy()
    v = int(np.nonzero(~valid)[0][0])
    bad[v] = fn[v]
    assert not np.array_equal(bad[v], mp[v])
    with pytest.raises(AssertionError, match='invalid vertex'):
        R.check_update(sn['f0'], sn['S'], cvec, valid, 0, sn['f0'], 2, fn, S_after, bad)
