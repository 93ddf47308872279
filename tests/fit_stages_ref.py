"""
Plain restatement of one fit iteration, stage by stage (NumPy float64 / exact integers; no GPU, no library call).

Every function takes the arrays the device READ for one stage and returns what it must have WRITTEN, so a test can check each kernel from
the device's own inputs to that stage: nothing drifts from stage to stage, the bounds are per element and derived here, and the integer
scatter is checked for equality.  tests/test_fit_stages_ref.py pins these functions against oracle/nanowrap_oracle.py on the CPU;
tests/test_hip_fit_stages.py uses them on the device's snapshots.

u = 2^-24 is the unit roundoff of float32 (relative error of ONE correctly rounded operation), 2^-53 that of float64.

Stages (kernels in ch_shrinkwrap_amd/csrc):
  attract_rows    nw_attract_point (nw_attract.h): row of the weight matrix, nearest-centroid distance, de-weighted residual
  scatter_exact   nw_attract_point's quantisation + the table / flush (integers: any order of addition gives the same sums) and the
                  conversions k_prior_directions makes of them (S0, pi)
  prior           nw_prior_ring_vertex (nw_device.h) + k_prior_directions (nw_kernels.h): fdef, prefs, S1
  scalars         k_prior_directions / k_subspace_point_sums / k_attract partial sums -> the 28 sums of k_reduce_scalars
  small_solve     nw_solve_small (float32, same pivoting, same order)
  update          k_solve_update's vertex loop
"""
import math
import os
import re

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW_SPARTS = 32


# ------------------------------------------------------------------------------------------------------------------------------------------
# slot indices of NW_ARR_SCALARS, read from the header (a renumbering must not silently shift the tests)
# ------------------------------------------------------------------------------------------------------------------------------------------
def scalar_slots(header=None):
    """{'RES2': 0, 'C0': 1, ...} from the `SC_*` enum of csrc/nw_kernels.h (text parse: `SC_NAME = <int>`)."""
    header = header or os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_kernels.h')
    with open(header) as fh:
        text = fh.read()
    m = re.search(r'enum\s*\{([^}]*SC_COUNT[^}]*)\}', text)
    if m is None:
        raise ValueError('no SC_* enum in %s' % header)
    body = re.sub(r'//[^\n]*', '', m.group(1))
    slots = {}
    for name, val in re.findall(r'\bSC_(\w+)\s*=\s*(\d+)', body):
        slots[name] = int(val)
    if 'COUNT' not in slots:
        raise ValueError('SC_COUNT missing')
    return slots


def _tri(r, c):
    """index of (r, c) in the packed upper triangle {00, 01, 02, 11, 12, 22} (nw_tri)"""
    r, c = min(r, c), max(r, c)
    return c if r == 0 else (2 + c if r == 1 else 5)


# ------------------------------------------------------------------------------------------------------------------------------------------
# per-point rows
# ------------------------------------------------------------------------------------------------------------------------------------------
def face_centroids32(pos, faces):
    """k_face_centroids: ((v0 + v1) + v2) / 3 in float32 (what the distance and the query use)."""
    p = np.asarray(pos, F32)
    return ((p[faces[:, 0]] + p[faces[:, 1]]) + p[faces[:, 2]]) / F32(3.0)


def attract_rows(pos, faces, face, pts, data, sinv, wnorm, mask=None):
    """pos (M,3) f4 the estimate the iteration started from, faces (F,3), face (N,) nearest face per point, pts (N,3) f4, data (N,3) f4
    target of the residual or None (= pts), sinv / wnorm: scalar or (N,3) f4 (sigma_inv un-normalised; weights divided by their mean),
    mask (N,3) bool (not used by the rows themselves: carried for the caller's sums).

    Returns a dict: vidx (N,3); w64, dist64, res64 in float64 from the float32 inputs (no intermediate rounding); bw, bd, br the bounds
    on |device - float64|; and w32, dist32, res32: the same arithmetic in float32 in the kernel's order (for bit comparisons).  The kernel
    forms the de-weighting factor from the distance ROUNDED to float32 (the array it stores); the reference keeps the float64 distance
    of its k-d tree: res32_d64 is that form (bit-equal to the oracle's residual; res32 differs from it in the last bit now and then).

    Bounds (first order in u; every float32 operation contributes a relative error <= u; the inputs are exact float32 values):
      w     d_j^2 = sum_k (fv_jk - p_k)^2: the subtraction (1 rounding) enters squared (2u), the product 1, the two additions of positive
            terms <= 2: 5u on d_j^2, so 2.5u after the square root, + 1 for sqrtf, + 1 for the reciprocal: 4.5u on 1/d_j.  The row sum
            (positive terms) inherits 4.5u and adds 2 roundings: 6.5u.  The quotient: 4.5 + 6.5 + 1 = 12 roundings.   |w - w64| <= 16u w64.
      dist  float64 arithmetic (errors ~2^-52, i.e. 1e-8 u) and ONE rounding to float32.                       |d - d64| <= 1.01u d64.
      res   A f = sum_j fv_jk w_j: each product carries w's 16u + 1 for the product, the three additions (the first to 0 is exact)
            <= 2 more, rounded up to 3: 20u sum_j |fv_jk| w_j.  (t - A f): 1 rounding of a quantity <= |t| + sum |fv| w; times the
            weight: 1; the float64 product with the de-weighting factor, rounded to float32: 1; slack 1.  24u (|t_k| + sum_j |fv_jk| w_j)
            wt wd.  The de-weighting factor wd = 1/(d s/2 + 1) is formed in float64 from the float32 distance: relative error
            <= 1.01u; with the final rounding's share of |res| itself: 4u |res64|.
            |res_k - res64_k| <= wt wd 24u (|t_k| + sum_j |fv_jk| w_j) + 4u |res64_k|."""
    pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
    N = pts.shape[0]
    tgt = pts if data is None else np.ascontiguousarray(data, F32).reshape(-1, 3)
    si = np.broadcast_to(np.asarray(sinv, F32).reshape(-1, 3) if np.ndim(sinv) else F32(sinv), (N, 3))
    wt = np.broadcast_to(np.asarray(wnorm, F32).reshape(-1, 3) if np.ndim(wnorm) else F32(wnorm), (N, 3))
    face = np.asarray(face).astype(np.int64)
    vidx = np.asarray(faces)[face].astype(np.int32)                   # (N, 3)
    fv = pos[vidx]                                                     # (N, corner, comp) f4
    # ---- float32, the kernel's order
    d = fv - pts[:, None, :]
    sq = d * d
    dj = np.sqrt((sq[:, :, 0] + sq[:, :, 1]) + sq[:, :, 2])
    wr = F32(1.0) / np.maximum(dj, F32(1e-6))
    wsum = (wr[:, 0] + wr[:, 1]) + wr[:, 2]
    w32 = wr / wsum[:, None]
    cent = face_centroids32(pos, np.asarray(faces))[face]
    dc = pts.astype('f8') - cent.astype('f8')
    dist64 = np.sqrt(dc[:, 2] * dc[:, 2] + (dc[:, 1] * dc[:, 1] + dc[:, 0] * dc[:, 0]))
    dist32 = dist64.astype(F32)
    af = F32(0.0) + fv[:, 0, :] * w32[:, 0:1]
    af = af + fv[:, 1, :] * w32[:, 1:2]
    af = af + fv[:, 2, :] * w32[:, 2:3]
    r0 = wt * (tgt - af)
    wd32 = 1.0 / (dist32.astype('f8')[:, None] * si.astype('f8') / 2.0 + 1.0)
    res32 = (r0.astype('f8') * wd32).astype(F32)
    res32_d64 = (r0.astype('f8') * (1.0 / (dist64[:, None] * si.astype('f8') / 2.0 + 1.0))).astype(F32)      # the reference's form: the distance never rounded
    # ---- float64 from the same inputs
    fv64, p64 = fv.astype('f8'), pts.astype('f8')
    dj64 = np.sqrt(((fv64 - p64[:, None, :]) ** 2).sum(2))
    wr64 = 1.0 / np.maximum(dj64, float(F32(1e-6)))
    w64 = wr64 / wr64.sum(1)[:, None]
    af64 = (fv64 * w64[:, :, None]).sum(1)
    wd64 = 1.0 / (dist64[:, None] * si.astype('f8') / 2.0 + 1.0)
    res64 = wt.astype('f8') * (tgt.astype('f8') - af64) * wd64
    mag = np.abs(tgt.astype('f8')) + (np.abs(fv64) * w64[:, :, None]).sum(1)
    return dict(vidx=vidx, w64=w64, dist64=dist64, res64=res64,
                bw=16 * U32 * w64, bd=1.01 * U32 * dist64, br=np.abs(wt.astype('f8')) * wd64 * 24 * U32 * mag + 4 * U32 * np.abs(res64),
                w32=w32, dist32=dist32, res32=res32, res32_d64=res32_d64, mask=mask)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the scatter, in integers
# ------------------------------------------------------------------------------------------------------------------------------------------
def quantise(w, res, q, qw, rint=np.rint):
    """nw_attract_point's twelve integers per point: (N, corner, 4) int64.  c = float32(w_j r_k) (the float32 product the reference forms),
    x = rint(float64(c) / q), half to even (the kernel adds 1.5 * 2^52: the same rounding for |x| < 2^51); the fourth: rint(w_j / qw).
    q and qw are powers of two, so the scaling is exact."""
    w = np.ascontiguousarray(w, F32).reshape(-1, 3)
    r = np.ascontiguousarray(res, F32).reshape(-1, 3)
    c = w[:, :, None] * r[:, None, :]
    assert c.dtype == np.float32
    x = rint(c.astype('f8') / float(q))
    xw = rint(w.astype('f8') / float(qw))
    return np.concatenate([x, xw[:, :, None]], axis=2).astype(np.int64)


def scatter_exact(vidx, w, res, q, qw, M, rint=np.rint):
    """Returns (table (M,4) int64, S0 (M,3) f4, pi (M,) f4): the accumulator after the attraction step and what k_prior_directions makes
    of it: S0 = float32(float64(sum) * q), sw = float32(float64(sum w) * qw), pi = sqrtf((sw^2 + sw^2) + sw^2) in float32."""
    x = quantise(w, res, q, qw, rint)
    table = np.zeros((int(M), 4), np.int64)
    np.add.at(table, np.asarray(vidx).reshape(-1).astype(np.int64), x.reshape(-1, 4))
    S0, pi = accumulator_to_float(table, q, qw)
    return table, S0, pi


def accumulator_to_float(table, q, qw):
    S0 = (table[:, :3].astype('f8') * float(q)).astype(F32)
    sw = (table[:, 3].astype('f8') * float(qw)).astype(F32)
    pi = np.sqrt((sw * sw + sw * sw) + sw * sw)
    assert pi.dtype == np.float32
    return S0, pi


def scatter_slow(vidx, w, res, q, qw, M):
    """the same table with Python integers and an explicit half-to-even rule (no NumPy rounding, no vectorised addition)"""
    from fractions import Fraction
    w = np.ascontiguousarray(w, F32).reshape(-1, 3)
    r = np.ascontiguousarray(res, F32).reshape(-1, 3)
    vidx = np.asarray(vidx).reshape(-1, 3)

    def half_even(fr):
        fl = fr.numerator // fr.denominator
        rem = fr - fl
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
            return fl + 1
        return fl
    table = [[0, 0, 0, 0] for _ in range(int(M))]
    fq, fqw = Fraction(float(q)), Fraction(float(qw))
    for i in range(w.shape[0]):
        for j in range(3):
            for k in range(3):
                c = F32(w[i, j] * r[i, k])
                table[int(vidx[i, j])][k] += half_even(Fraction(float(c)) / fq)
            table[int(vidx[i, j])][3] += half_even(Fraction(float(w[i, j])) / fqw)
    return table


def scatter_abs(vidx, w, res, M):
    """per vertex: number of contributions, sum |w_j r_k| (M,3) and sum w_j (M,) in float64 -- the serial float32 scatter of the reference
    (conj_grad_utils.c:153-162) is within deg * u * sum|terms| of the exact sum"""
    w = np.ascontiguousarray(w, F32).reshape(-1, 3).astype('f8')
    r = np.ascontiguousarray(res, F32).reshape(-1, 3).astype('f8')
    v = np.asarray(vidx).reshape(-1).astype(np.int64)
    deg = np.bincount(v, minlength=int(M)).astype('f8')
    a = np.zeros((int(M), 3))
    np.add.at(a, v, (np.abs(w)[:, :, None] * np.abs(r)[:, None, :]).reshape(-1, 3))
    sw = np.bincount(v, weights=w.reshape(-1), minlength=int(M))
    return deg, a, sw


# ------------------------------------------------------------------------------------------------------------------------------------------
# curvature prior
# ------------------------------------------------------------------------------------------------------------------------------------------
def vertex_area_weights(f, nbr):
    """k_vertex_area_weights: 1/sqrt(sum_n |f_n - f_i|^2 + 1), float32 sums in slot order up to the first -1; 0 without neighbours"""
    f = np.ascontiguousarray(f, F32).reshape(-1, 3)
    M, NB = nbr.shape
    acc = np.zeros(M, F32)
    alive = np.ones(M, bool)
    for s in range(NB):
        n = nbr[:, s]
        alive &= n != -1
        nn = np.where(alive, n, 0)
        d2 = np.zeros(M, F32)
        for j in range(3):
            dd = f[nn, j] - f[:, j]
            d2 = d2 + dd * dd
        acc = np.where(alive, acc + d2, acc).astype(F32)
    out = (1.0 / np.sqrt(acc + F32(1.0)).astype('f8')).astype(F32)
    return np.where(acc > 0, out, F32(0.0)).astype(F32)


def prior(meshpos, pos, nrm, nbr, pi, wv=None):
    """meshpos (M,3) f4 mesh positions (valid vertices follow the estimate), pos (M,3) f4 the estimate, nrm (M,3) f4 block-stale normals,
    nbr (M,NB) 1-ring ids (-1 padded), pi (M,) f4, wv (M,) f4 weights of the 'wfunc' regulariser or None.

    oracle.ncc_prior is the model; the order of the float32 ring sum and of the float64 sums is the kernel's (slot order).  An isolated
    vertex (no neighbour) keeps its mesh position; the gate is min(pi^2, 1) in float32.
    Returns fdef64 (M,3), prefs64 (M,3) (already times wv for wfunc), S1 (M,3) f4, and vc, alpha, ms for the bounds."""
    meshpos = np.ascontiguousarray(meshpos, F32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, F32).reshape(-1, 3)
    pi = np.ascontiguousarray(pi, F32).reshape(-1)
    M, NB = nbr.shape
    s = np.zeros((M, 3), F32)
    ms = np.zeros(M, np.int64)
    for k in range(NB):
        ok = nbr[:, k] >= 0
        nn = np.where(ok, nbr[:, k], 0)
        s = np.where(ok[:, None], s + meshpos[nn], s).astype(F32)
        ms += ok
    with np.errstate(invalid='ignore', divide='ignore'):
        vc = s.astype('f8') / ms[:, None]
        asum = np.zeros(M)
        for k in range(NB):
            ok = nbr[:, k] >= 0
            nn = np.where(ok, nbr[:, k], 0)
            qn, un = meshpos[nn].astype('f8'), nrm[nn]
            cn = qn - vc
            u8 = un.astype('f8')
            cdot = (cn[:, 0] * u8[:, 0] + cn[:, 1] * u8[:, 1]) + cn[:, 2] * u8[:, 2]
            ndn = (un[:, 0] * nrm[:, 0] + un[:, 1] * nrm[:, 1]) + un[:, 2] * nrm[:, 2]
            den = np.sqrt(F32(2.0) * (np.maximum(ndn, F32(0.0)) + F32(1.0)))
            assert den.dtype == np.float32
            asum = np.where(ok, asum + cdot / den.astype('f8'), asum)
        gate = np.minimum(pi * pi, F32(1.0))
        alpha = (asum / ms) * gate.astype('f8')
        fd = vc + alpha[:, None] * nrm.astype('f8')
    iso = ms == 0
    fd[iso] = meshpos[iso].astype('f8')
    vc[iso] = 0.0
    alpha[iso] = 0.0
    p64 = pos.astype('f8') - fd
    if wv is not None:
        lw = np.ascontiguousarray(wv, F32)
        p64 = p64 * lw.astype('f8')[:, None]
        p32 = p64.astype(F32)
        S1 = F32(-1.0) * (p32 * lw[:, None])
    else:
        S1 = F32(-1.0) * p64.astype(F32)
    return dict(fdef64=fd, prefs64=p64, S1=S1.astype(F32), vc=vc, alpha=alpha, ms=ms, isolated=iso)


def s1_candidates(pr, pos, wv=None):
    """S[:,1] must equal -float32(prefs64) wherever prefs64 lies more than 4 float64 ulps of its operands from a float32 rounding boundary:
    returns (lo, hi) = the float32 images of prefs64 -+ 4 ulp(max(|pos|, |fdef|)); where they coincide the value is pinned, elsewhere the
    two differ by one float32 ulp and either is accepted."""
    tol = 4 * 2.0 ** -52 * np.maximum(np.abs(np.asarray(pos, 'f8').reshape(-1, 3)), np.abs(pr['fdef64']))
    lw = None if wv is None else np.ascontiguousarray(wv, F32)
    if lw is not None:
        tol = tol * lw.astype('f8')[:, None]
    a, b = (pr['prefs64'] - tol).astype(F32), (pr['prefs64'] + tol).astype(F32)
    if lw is not None:
        a, b = a * lw[:, None], b * lw[:, None]
    a, b = F32(-1.0) * a, F32(-1.0) * b
    return np.minimum(a, b), np.maximum(a, b)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the 28 sums
# ------------------------------------------------------------------------------------------------------------------------------------------
def subspace_rows(S, vidx, w, n_search):
    """AS_k[i, c] = sum_j w_ij S_k[v_ij, c] in float32, corner order, starting from 0 (k_subspace_point_sums; -ffp-contract=off is a build
    flag, so every product and every sum is rounded on its own).  Returns (N, comp, 3) f4; direction 2 is zero while n_search is 2."""
    S = np.ascontiguousarray(S, F32).reshape(-1, 3, 3)                # (vertex, comp, direction)
    if n_search <= 2:                                                 # (a block's first iteration: the device's third column is not written yet)
        S = S.copy()
        S[:, :, 2] = 0.0
    w = np.ascontiguousarray(w, F32).reshape(-1, 3)
    vidx = np.asarray(vidx).reshape(-1, 3)
    a = np.zeros((w.shape[0], 3, 3), F32)
    for j in range(3):
        a = a + S[vidx[:, j]] * w[:, j][:, None, None]
    assert a.dtype == np.float32
    return a


def scalars(S, w, vidx, res, mask, pos, fdef, dist, n_search, wv=None, slots=None):
    """The sums k_reduce_scalars leaves (one value per slot: its 32 parts added), from the arrays the device read:
    S (M,9)/(3M,3) f4 with columns 0, 1 of this iteration and the last step in column 2; w, vidx, res (N,3); mask (N,3) bool; pos (M,3) f4
    the estimate; fdef (M,3): float32 as the device stores it (then the sums fed by p64 = pos - fdef carry that rounding, u |fdef| per
    element, propagated) or float64 (exact); dist (N,) f4; wv: wfunc weights or None.

    Every sum is math.fsum of its terms (products of float32 values are exact in float64).  Returns (value, abssum, bound), arrays over the
    slots: bound = n 2^-53 sum|terms| (n terms: n - 1 float64 additions in any order, and one rounding for a term that is a product with
    a float64 factor) + the propagated rounding of fdef where it applies."""
    sl = slots or scalar_slots()
    S3 = np.ascontiguousarray(S, F32).reshape(-1, 3, 3)
    M = S3.shape[0]
    r = np.ascontiguousarray(res, F32).reshape(-1, 3).astype('f8')
    mask = np.asarray(mask, bool).reshape(-1, 3)
    N = r.shape[0]
    val, ab, bnd = np.zeros(sl['COUNT']), np.zeros(sl['COUNT']), np.zeros(sl['COUNT'])

    def put(slot, terms, extra=0.0):
        t = np.asarray(terms, 'f8').ravel()
        val[slot] = math.fsum(t)
        ab[slot] = math.fsum(np.abs(t))
        bnd[slot] = t.size * U64 * ab[slot] + extra

    put(sl['RES2'], r * r)
    put(sl['C0'], (r * r)[mask])
    d = np.ascontiguousarray(dist, F32).astype('f8')
    put(sl['SUMD'], d)
    val[sl['NPTS']], ab[sl['NPTS']] = N, N
    val[sl['MAXD']] = d.max() if N else 0.0
    a = subspace_rows(S3, vidx, w, n_search).astype('f8')
    for i in range(3):
        for j in range(i, 3):
            put(sl['HC'] + _tri(i, j), (a[:, :, i] * a[:, :, j])[mask])
        put(sl['GC'] + i, (a[:, :, i] * r)[mask])
    # vertex side
    lw = None if wv is None else np.ascontiguousarray(wv, F32)
    s_raw = S3.copy()
    if n_search <= 2:
        s_raw[:, :, 2] = 0.0
    l = s_raw if lw is None else (s_raw * lw[:, None, None]).astype(F32)
    l8 = l.astype('f8')
    f_is32 = np.asarray(fdef).dtype == np.float32
    fd = np.asarray(fdef, 'f8').reshape(-1, 3)
    p64 = np.asarray(pos, F32).reshape(-1, 3).astype('f8') - fd
    e64 = (U32 * np.abs(fd)) if f_is32 else np.zeros_like(fd)          # what float32(fdef) may have lost
    if lw is not None:
        p64 = p64 * lw.astype('f8')[:, None]
        e64 = e64 * lw.astype('f8')[:, None]
    for i in range(3):
        for j in range(i, 3):
            put(sl['SS'] + _tri(i, j), l8[:, :, i] * l8[:, :, j])
        put(sl['SP'] + i, l8[:, :, i] * p64, extra=math.fsum((np.abs(l8[:, :, i]) * e64).ravel()))
    put(sl['PP64'], p64 * p64, extra=math.fsum((2 * np.abs(p64) * e64 + e64 * e64).ravel()))
    if lw is None:
        p32 = (F32(-1.0) * s_raw[:, :, 1]).astype('f8')               # S1 = -float32(p64): the float32 prefs are in the device's own S
        put(sl['PP32'], p32 * p32)
    else:                                                            # wfunc: S1 = -(p32 wv), p32 itself is not stored
        p32 = p64.astype(F32).astype('f8')
        e32 = e64 + U32 * np.abs(p64)
        put(sl['PP32'], p32 * p32, extra=math.fsum((2 * np.abs(p32) * e32 + e32 * e32).ravel()))
    s8 = s_raw.astype('f8')
    put(sl['T'] + 0, s8[:, :, 0] * s8[:, :, 0])
    put(sl['T'] + 1, s8[:, :, 0] * s8[:, :, 1])
    put(sl['T'] + 2, s8[:, :, 1] * s8[:, :, 1])
    return val, ab, bnd


def add_parts(parts, slots=None):
    """(SC_COUNT * 32,) doubles as the device leaves them -> one value per slot, the 32 parts added IN ORDER as k_solve_update adds them
    (the largest-distance slot: their maximum)"""
    sl = slots or scalar_slots()
    p = np.asarray(parts, 'f8').reshape(-1, NW_SPARTS)[:sl['COUNT']]
    out = np.zeros(sl['COUNT'])
    for s in range(sl['COUNT']):
        t = 0.0
        for b in range(NW_SPARTS):
            t = max(t, float(p[s, b])) if s == sl['MAXD'] else t + float(p[s, b])
        out[s] = t
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# normal equations and update
# ------------------------------------------------------------------------------------------------------------------------------------------
def small_solve(sc, lam, n_search, slots=None):
    """nw_solve_small in float32: H = float32(float64(float32(Hc)) + lam^2 float64(float32(Hw))), G likewise with Gw = -SP in float64;
    Gaussian elimination with partial pivoting (strict >, so the first of equal pivots stays), back substitution, all float32 in the
    kernel's order.  Returns dict(H (3,3) f4, G (3,) f4, c (3,) f4, singular, c64: numpy.linalg.solve of the same float32 system in
    float64, cond: its 2-norm condition number)."""
    sl = slots or scalar_slots()
    n = 3 if n_search > 2 else 2
    lam = F32(lam)
    l2 = float(lam) * float(lam)
    A = np.zeros((3, 4), F32)
    H = np.zeros((3, 3), F32)
    G = np.zeros(3, F32)
    for r in range(3):
        for c in range(3):
            hc = F32(sc[sl['HC'] + _tri(r, c)])
            hw = F32(sc[sl['SS'] + _tri(r, c)])
            H[r, c] = F32(float(hc) + l2 * float(hw))
            A[r, c] = H[r, c]
        gc = F32(sc[sl['GC'] + r])
        gw = -float(sc[sl['SP'] + r])
        G[r] = F32(float(gc) + l2 * gw)
        A[r, 3] = G[r]
    singular = False
    with np.errstate(all='ignore'):
        for k in range(n):
            mx = abs(A[k, k])
            for r in range(k + 1, n):
                if abs(A[r, k]) > mx:
                    mx = abs(A[r, k])
                    A[[k, r]] = A[[r, k]]
            singular = singular or not (mx > 0)
            for r in range(k + 1, n):
                lf = F32(A[r, k] / A[k, k])
                for c in range(k, 4):
                    A[r, c] = F32(A[r, c] - F32(lf * A[k, c]))
        x = np.zeros(3, F32)
        for k in range(n - 1, -1, -1):
            sacc = A[k, 3]
            for c in range(k + 1, n):
                sacc = F32(sacc - F32(A[k, c] * x[c]))
            x[k] = F32(sacc / A[k, k])
    c = np.zeros(3, F32) if singular else x
    out = dict(H=H, G=G, c=c, singular=singular, c64=None, cond=np.inf)
    if not singular:
        H8, G8 = H[:n, :n].astype('f8'), G[:n].astype('f8')
        out['c64'] = np.concatenate([np.linalg.solve(H8, G8), np.zeros(3 - n)])
        out['cond'] = float(np.linalg.cond(H8))
    return out


def predictions(sc, sol, n_search, slots=None):
    """cpred and wpred of k_solve_update's log block, in float64"""
    sl = slots or scalar_slots()
    c, H, G = sol['c'].astype('f8'), sol['H'].astype('f8'), sol['G'].astype('f8')
    n = 3 if n_search > 2 else 2
    cHc = cG = cHwc = cGw = 0.0
    for r in range(n):
        cG += c[r] * G[r]
        cGw += c[r] * (-sc[sl['SP'] + r])
        for k in range(n):
            cHc += c[r] * H[r, k] * c[k]
            cHwc += c[r] * float(F32(sc[sl['SS'] + _tri(r, k)])) * c[k]
    return sc[sl['C0']] + cHc - cG, sc[sl['PP64']] + cHwc - cGw


def update(pos, S, c, valid, flags, meshpos=None, n_search=3):
    """k_solve_update's vertex loop: step = S0 c0, + S1 c1, (+ S2 c2 from the second iteration on), fnew = f + step, all float32 in that
    order; flags bit 0: fnew * (fnew > 0); bit 1: no last-step direction.  Returns (fnew (M,3), S2 = fnew - f (M,3), meshpos after
    the write-back: fnew at valid vertices, untouched elsewhere)."""
    pos = np.ascontiguousarray(pos, F32).reshape(-1, 3)
    S3 = np.ascontiguousarray(S, F32).reshape(-1, 3, 3)
    c = np.asarray(c, F32)
    step = S3[:, :, 0] * c[0]
    step = step + S3[:, :, 1] * c[1]
    if n_search > 2:
        step = step + S3[:, :, 2] * c[2]
    fn = pos + step
    assert fn.dtype == np.float32
    if flags & 1:
        fn = np.where(fn > 0, fn, fn * F32(0.0)).astype(F32)
    s2 = S3[:, :, 2].copy() if (flags & 2) else (fn - pos)
    mp = None
    if meshpos is not None:
        ok = np.ones(pos.shape[0], bool) if valid is None else np.asarray(valid).astype(bool)
        mp = np.where(ok[:, None], fn, np.ascontiguousarray(meshpos, F32).reshape(-1, 3)).astype(F32)
    return fn, s2.astype(F32), mp


# ------------------------------------------------------------------------------------------------------------------------------------------
# the assertions both test files share (the GPU test on the device's snapshots, the CPU test on the oracle's trace and on mutated copies)
# ------------------------------------------------------------------------------------------------------------------------------------------
def ratio(err, bound):
    """largest err / bound (0/0 counts as 0: an exact value against a zero bound)"""
    err, bound = np.asarray(err, 'f8'), np.asarray(bound, 'f8')
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def check_rows(rows, vidx, w, dist, res, faces, face):
    """(a): vidx == faces[face]; w, dist, res within their bounds.  Returns the three max err/bound figures."""
    assert np.array_equal(np.asarray(vidx).reshape(-1, 3), np.asarray(faces)[np.asarray(face)]), 'vidx != faces[face]'
    rw = ratio(np.abs(np.asarray(w, 'f8').reshape(-1, 3) - rows['w64']), rows['bw'])
    rd = ratio(np.abs(np.asarray(dist, 'f8') - rows['dist64']), rows['bd'])
    rr = ratio(np.abs(np.asarray(res, 'f8').reshape(-1, 3) - rows['res64']), rows['br'])
    assert rw <= 1.0, 'weights: max err/bound %.3f' % rw
    assert rd <= 1.0, 'distance: max err/bound %.3f' % rd
    assert rr <= 1.0, 'residual: max err/bound %.3f' % rr
    return rw, rd, rr


def check_scatter(vacc, vidx, w, res, q, qw, M):
    """(b): the accumulator equals the integer restatement, as exact int64"""
    table, S0, pi = scatter_exact(vidx, w, res, q, qw, M)
    got = np.asarray(vacc, np.int64).reshape(-1, 4)
    bad = np.nonzero((got != table).any(1))[0]
    assert bad.size == 0, 'accumulator differs at %d vertices, first %d: device %s, exact %s' % (bad.size, bad[0], got[bad[0]], table[bad[0]])
    return table, S0, pi


def check_sums(parts, ref, slots=None):
    """(d): each slot, its 32 parts added in order, within its bound; the count and the largest distance exact.  ref = scalars(...)."""
    sl = slots or scalar_slots()
    val, ab, bnd = ref
    got = add_parts(parts, sl)
    worst = 0.0
    for name, width in (('RES2', 1), ('C0', 1), ('SUMD', 1), ('HC', 6), ('GC', 3), ('SS', 6), ('SP', 3), ('PP64', 1), ('PP32', 1), ('T', 3)):
        for k in range(width):
            s = sl[name] + k
            rr = ratio(abs(got[s] - val[s]), bnd[s])
            worst = max(worst, rr)
            assert rr <= 1.0, 'sum SC_%s[%d]: device %.17g, reference %.17g, bound %.3g (err/bound %.3f)' % (name, k, got[s], val[s], bnd[s], rr)
    assert got[sl['NPTS']] == val[sl['NPTS']], 'SC_NPTS %r != %r' % (got[sl['NPTS']], val[sl['NPTS']])
    assert got[sl['MAXD']] == val[sl['MAXD']], 'SC_MAXD %r != %r' % (got[sl['MAXD']], val[sl['MAXD']])
    return got, worst


def check_update(pos0, S, c, valid, flags, meshpos0, n_search, pos1, S_after, meshpos1):
    """(e): fnew, S[:,2] and the mesh positions bit for bit; mesh positions untouched where valid == 0"""
    fn, s2, mp = update(pos0, S, c, valid, flags, meshpos0, n_search)
    assert np.array_equal(np.asarray(pos1, F32).reshape(-1, 3), fn), 'fnew differs in bits'
    assert np.array_equal(np.asarray(S_after, F32).reshape(-1, 3, 3)[:, :, 2], s2), 'S[:,2] differs in bits'
    got = np.asarray(meshpos1, F32).reshape(-1, 3)
    inv = ~(np.ones(fn.shape[0], bool) if valid is None else np.asarray(valid).astype(bool))
    assert np.array_equal(got[inv], np.asarray(meshpos0, F32).reshape(-1, 3)[inv]), 'mesh position of an invalid vertex was written'
    assert np.array_equal(got, mp), 'mesh positions differ in bits'
    return fn
