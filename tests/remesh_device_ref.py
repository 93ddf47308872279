"""
A plain restatement of nw_remesh_device (csrc/nw_remesh_dev.hip) for the tests: NumPy and the standard library only, no GPU, not the package.

The device unit is built without contraction of a*b+c, keeps positions in float64, takes priorities from a hash of the half-edge and ids from
prefix sums over list order: its arrays are a function of its input, and this file writes that function down -- sequentially, one operation
after another, where the kernels run a round's winners at once.  What decides the arrays is restated: the set-up (twins, vhe = lowest outgoing
half-edge, frozen vertices), per pass the candidate list in half-edge order, per round the bids (the admission tests of
HalfEdgeMesh::split / collapse / flip of csrc/remesh.cpp in the device's order), the winners (a key that is the largest in every vertex of its
footprint), the ids of what the splits create, the stop rules, the Jacobi relaxation, and the result (live faces in slot order, used vertices in
stable Morton order).  A round's winners are applied one after another in list order; while doing so the restatement CHECKS what lets the
kernels apply them at once: their footprints are pairwise disjoint, every write lands inside the writer's footprint (or in what it creates),
and after every round twin is an involution on live half-edges, every vhe is a live outgoing half-edge and val is the ring's length wherever
the fan closes.

    remesh_device_ref(v, f, n, L, l=0.5, n_relax=0, max_valence=16) -> (vertices float32, faces int32, info)

info: n_split / n_collapse / n_flip, rounds and non-empty passes per kind (the fewest rounds the host loop can launch: it may run up to two
more per pass, which find nothing to do), max_valence (of the result; `peak_valence`: after any pass), mean_edge_length, `margin` = the smallest relative distance from equality of any
floating-point comparison made (|lhs - rhs| over the sum of the absolute terms; `margin_nonzero`: of those that were not exact ties; `margin_rounded`: of those
whose operands went through a square root or a division, the two operations that the device might round in another way), `log` = how often every admission branch was taken.
"""
import collections
import math

import numpy as np

RING_MAX = 64
R_MAX = (24, 32, 24)          # rounds of a split / collapse / flip pass at most
_M32 = 0xffffffff


def pass_goes_on(bids_of, r):
    """is round r of a pass run?  bids_of: the bidders of its rounds 0 .. r-1.  Not after a round without a bidder, and not after a round, the
    last one aside, with so few that the next iteration may as well have them"""
    return not (any(b == 0 for b in bids_of) or any(0 < b < 8 and 500 * b < bids_of[0] for b in bids_of[:max(r - 1, 0)]))


def sweeps_end(n_list, first_list):
    """a split sweep over a handful of edges is left to the next iteration"""
    return n_list < 32 and n_list * 200 < first_list


def iterations_end(n_relax, before, now):
    """before, now: (splits, collapses, flips) so far; an iteration that changed nothing would be repeated unchanged by every later one"""
    return n_relax == 0 and tuple(before) == tuple(now)


class Refused(ValueError):
    """what the device refuses: .code is 'bad argument' or 'non-manifold'"""
    def __init__(self, code, why):
        ValueError.__init__(self, '%s: %s' % (code, why))
        self.code = code


def key_of(seed, h):
    """rm_key without the round's number on top (keys are only compared within a round): (16 bits of hash, half-edge)"""
    x = ((h * 2654435761) & _M32) ^ ((seed * 0x9e3779b9) & _M32)
    x ^= x >> 16
    x = (x * 0x7feb352d) & _M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & _M32
    x ^= x >> 16
    return ((x & 0xffff) << 32) | h


def _nx(h):
    return h - 2 if h % 3 == 2 else h + 1


def _pv(h):
    return h + 2 if h % 3 == 0 else h - 1


def _sub(p, q):
    return (p[0] - q[0], p[1] - q[1], p[2] - q[2])


def _dot(p, q):
    return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _absdot(p, q):
    return abs(p[0] * q[0]) + abs(p[1] * q[1]) + abs(p[2] * q[2])


def ring_lengths(F, twin, vhe):
    """for every vertex at once: (steps of the walk from vhe, closed within RING_MAX steps)"""
    nv = vhe.shape[0]
    n = np.zeros(nv, np.int64)
    closed = np.zeros(nv, bool)
    idx = np.nonzero(vhe >= 0)[0]
    h = vhe[idx].astype(np.int64)
    h0 = h.copy()
    for _ in range(RING_MAX):
        if idx.size == 0:
            break
        h = twin[np.where(h % 3 == 0, h + 2, h - 1)]
        n[idx] += 1
        back = h == h0
        closed[idx[back]] = True
        go = ~back & (h >= 0)
        idx, h, h0 = idx[go], h[go], h0[go]
    return n, closed


class _Mesh:
    def __init__(self, v, f, L, max_valence, check):
        v = np.ascontiguousarray(v, np.float32)
        f = np.ascontiguousarray(f, np.int32)
        if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
            raise ValueError('vertices must be (V,3) and faces (F,3)')
        nv, nf = v.shape[0], f.shape[0]
        L = float(np.float32(L))
        if nv < 3 or nf < 1 or not L > 0:
            raise Refused('bad argument', 'sizes or target')
        self.high, self.low = 4.0 / 3.0 * L, 4.0 / 5.0 * L
        self.high2, self.low2 = self.high * self.high, self.low * self.low
        self.max_valence = min(int(max_valence), 60) if max_valence > 0 else 16
        self.check = check
        self.margin = self.margin_nonzero = self.margin_rounded = math.inf
        self.log = collections.Counter()
        if not np.isfinite(v).all():
            raise Refused('bad argument', 'a coordinate that is not finite')
        if (f < 0).any() or (f >= nv).any():
            raise Refused('bad argument', 'a face refers to a vertex that is not there')
        if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any():
            raise Refused('bad argument', 'a face with a repeated corner')
        P = v.astype(np.float64)
        e = np.sqrt(((P[f] - P[np.roll(f, -1, 1)]) ** 2).sum(2))
        e.sort(1)
        pieces = float(((e[:, 2] / self.high + 1.0) * (e[:, 1] / self.high + 1.0)).sum())
        if not pieces < 67108864.0:
            raise Refused('bad argument', 'the lengths call for 2^26 faces or more')
        # twins from the directed edges
        o = f.ravel().astype(np.int64)
        t = np.roll(f, -1, 1).ravel().astype(np.int64)
        code, back = o * nv + t, t * nv + o
        order = np.argsort(code, kind='stable')
        sc = code[order]
        if (sc[1:] == sc[:-1]).any():
            raise Refused('non-manifold', 'a directed edge that occurs twice')
        at = np.searchsorted(sc, back)
        at[at >= sc.size] = 0
        twin = np.where(sc[at] == back, order[at], -1)
        nh = 3 * nf
        val = np.bincount(o, minlength=nv)
        vhe = np.full(nv, nh, np.int64)
        np.minimum.at(vhe, o, np.arange(nh))                          # the lowest outgoing half-edge
        vhe[vhe == nh] = -1
        bnd = np.zeros(nv, bool)
        bnd[o[twin < 0]] = True
        bnd[t[twin < 0]] = True
        n, closed = ring_lengths(o, twin, vhe)
        bnd |= (vhe >= 0) & ~bnd & (~closed | (n != val))
        self.nv_in = nv
        self.lo = P.min(0)
        self.ext = max(float((P.max(0) - self.lo).max()), 1e-30)
        self.P = [tuple(p) for p in P.tolist()]
        self.F, self.twin, self.vhe, self.val, self.bnd = o.tolist(), twin.tolist(), vhe.tolist(), val.tolist(), bnd.tolist()
        self.n_split = self.n_collapse = self.n_flip = 0
        self.rounds, self.passes = [0, 0, 0], [0, 0, 0]
        self.pass_seq = 0
        self.peak_valence = int(val.max())
        self._wh, self._wv = None, None

    # ---- comparisons (every one leaves its distance from equality behind) ----
    def _mg(self, lhs, rhs, scale=None, rounded=False):
        s = abs(lhs) + abs(rhs) if scale is None else scale
        m = abs(lhs - rhs) / s if s > 0 else 0.0
        if m < self.margin:
            self.margin = m
        if 0.0 < m < self.margin_nonzero:
            self.margin_nonzero = m
        if rounded and 0.0 < m < self.margin_rounded:
            self.margin_rounded = m

    def _mg_array(self, lhs, rhs):
        if lhs.size:
            s = np.abs(lhs) + abs(rhs)
            m = np.where(s > 0, np.abs(lhs - rhs) / np.where(s > 0, s, 1.0), 0.0)
            self.margin = min(self.margin, float(m.min()))
            if (m > 0).any():
                self.margin_nonzero = min(self.margin_nonzero, float(m[m > 0].min()))

    def _len2(self, a, b):
        p, q = self.P[a], self.P[b]
        x, y, z = p[0] - q[0], p[1] - q[1], p[2] - q[2]
        return x * x + y * y + z * z

    def _normal(self, a, b, c):
        P = self.P
        return _cross(_sub(P[b], P[a]), _sub(P[c], P[a]))

    def ring(self, v):
        """outgoing half-edges of v from vhe on, as rm_ring visits them; closed?"""
        twin = self.twin
        h0 = self.vhe[v]
        if h0 < 0:
            return [], False
        out, h = [], h0
        while True:
            out.append(h)
            h = twin[_pv(h)]
            if len(out) > RING_MAX:
                return out, False
            if h == h0 or h < 0:
                return out, h == h0

    def quad(self, h):
        F = self.F
        t = self.twin[h]
        hn, hp, tn, tp = _nx(h), _pv(h), _nx(t), _pv(t)
        return t, hn, hp, tn, tp, F[h], F[hn], F[hp], F[tp]

    # ---- candidate lists: all live half-edges with h < twin and c != d, in half-edge order ----
    def candidates(self, kind):
        F, T = np.asarray(self.F, np.int64), np.asarray(self.twin, np.int64)
        h = np.arange(F.shape[0])
        ok = (F >= 0) & (T >= 0) & (h < T)
        h = h[ok]
        t = T[h]
        nxt = lambda x: np.where(x % 3 == 2, x - 2, x + 1)
        prv = lambda x: np.where(x % 3 == 0, x + 2, x - 1)
        a, b, c, d = F[h], F[nxt(h)], F[prv(h)], F[prv(t)]
        ok = c != d
        h, a, b, c, d = h[ok], a[ok], b[ok], c[ok], d[ok]
        if kind == 2:
            val = np.asarray(self.val, np.int64)
            before = abs(val[a] - 6) + abs(val[b] - 6) + abs(val[c] - 6) + abs(val[d] - 6)
            after = abs(val[a] - 7) + abs(val[b] - 7) + abs(val[c] - 5) + abs(val[d] - 5)
            return h[after < before].tolist()
        P = np.asarray(self.P, np.float64).reshape(-1, 3)
        e = P[a] - P[b]
        l2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        if kind == 0:
            self._mg_array(l2, self.high2)
            bnd = np.asarray(self.bnd, bool)
            return h[(l2 > self.high2) & np.isfinite(l2) & ~(bnd[a] & bnd[b])].tolist()
        self._mg_array(l2, self.low2)
        return h[l2 < self.low2].tolist()

    # ---- admission tests ----
    def split_bids(self, lst):
        """a split's admission tests over the whole list at once (the list of a split pass is long, and most of it has been split already)"""
        F, T, bnd = np.asarray(self.F, np.int64), np.asarray(self.twin, np.int64), np.asarray(self.bnd, bool)
        P = np.asarray(self.P, np.float64).reshape(-1, 3)
        h = np.asarray(lst, np.int64)
        i = np.arange(h.shape[0])
        t = T[h]
        ok = (F[h] >= 0) & (t >= 0) & (h < t)
        i, h, t = i[ok], h[ok], t[ok]
        a, b = F[h], F[np.where(h % 3 == 2, h - 2, h + 1)]
        c, d = F[np.where(h % 3 == 0, h + 2, h - 1)], F[np.where(t % 3 == 0, t + 2, t - 1)]
        ok = c != d
        frozen = ok & bnd[a] & bnd[b]
        if frozen.any():
            self.log['split:both_frozen'] += int(frozen.sum())
        ok &= ~frozen
        e = P[a] - P[b]
        l2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        self._mg_array(l2[ok], self.high2)
        bid = ok & (l2 > self.high2) & np.isfinite(l2)
        self.log['split:short_enough_now'] += int((ok & ~bid).sum())
        self.log['split:bid'] += int(bid.sum())
        return [(ii, hh, fp) for ii, hh, fp in zip(i[bid].tolist(), h[bid].tolist(), zip(a[bid].tolist(), b[bid].tolist(), c[bid].tolist(), d[bid].tolist()))]

    def collapse_ok(self, h):
        """a = origin of h into its end b; returns the ring of a (vertices) or None"""
        log, val, bnd, P, F = self.log, self.val, self.bnd, self.P, self.F
        t, hn, hp, tn, tp, a, b, c, d = self.quad(h)
        if bnd[a] or bnd[b] or bnd[c] or bnd[d]:
            log['collapse:frozen'] += 1
            return None
        if c == d:
            log['collapse:c_is_d'] += 1
            return None
        if val[a] < 3 or val[b] < 3:
            log['collapse:degree_ab_below_3'] += 1
            return None
        if val[c] <= 3 or val[d] <= 3:
            log['collapse:degree_cd_at_most_3'] += 1
            return None
        if val[a] + val[b] - 4 > self.max_valence:
            log['collapse:degree_sum_above_max'] += 1
            return None
        if val[a] + val[b] - 4 < 3:
            log['collapse:degree_sum_below_3'] += 1
            return None
        rh, closed = self.ring(a)
        if not closed or len(rh) > RING_MAX or len(rh) != val[a]:
            log['collapse:ring_of_a'] += 1
            return None
        ra = [F[_nx(o)] for o in rh]
        pb = P[b]
        for x in ra:
            if x == b:
                continue
            q = P[x]
            ex, ey, ez = q[0] - pb[0], q[1] - pb[1], q[2] - pb[2]
            l2 = ex * ex + ey * ey + ez * ez
            self._mg(l2, self.high2)
            if l2 > self.high2:
                log['collapse:long_edge'] += 1
                return None
        rb, closed_b = self.ring(b)
        common = 0
        for o in rb:
            common += ra.count(F[_nx(o)])
        if not closed_b:
            log['collapse:ring_of_b'] += 1
            return None
        if common != 2:
            log['collapse:link_%d' % common] += 1
            return None
        for o in rh:
            x, y = F[_nx(o)], F[_pv(o)]
            if x == b or y == b:
                continue
            n0, n1 = self._normal(a, x, y), self._normal(b, x, y)
            d01 = _dot(n0, n1)
            self._mg(d01, 0.0, _absdot(n0, n1))
            if not d01 > 0.0:
                log['collapse:fold_sign'] += 1
                return None
            lhs, rhs = d01 * d01, 0.04 * _dot(n0, n0) * _dot(n1, n1)
            self._mg(lhs, rhs)
            if lhs < rhs:
                log['collapse:fold_cosine'] += 1
                return None
        if self.twin[hn] < 0 or self.twin[hp] < 0 or self.twin[tn] < 0 or self.twin[tp] < 0:
            log['collapse:open_twin'] += 1
            return None
        return ra

    def collapse_bid(self, h):
        """the edge of list entry h: (the half-edge whose origin goes, footprint) or None"""
        if self.F[h] < 0:
            return None
        t = self.twin[h]
        if t < 0 or h > t:
            return None
        a0, b0 = self.F[h], self.F[_nx(h)]
        l2 = self._len2(a0, b0)
        self._mg(l2, self.low2)
        if not l2 < self.low2:
            self.log['collapse:long_enough_now'] += 1
            return None
        for e, name in ((h, 'collapse:bid_h'), (t, 'collapse:bid_twin')):
            ra = self.collapse_ok(e)
            if ra is not None:
                self.log[name] += 1
                return e, [self.F[e]] + ra
        return None

    def flip_bid(self, h):
        log, val, bnd = self.log, self.val, self.bnd
        if self.F[h] < 0 or self.twin[h] < 0:
            return None
        t, hn, hp, tn, tp, a, b, c, d = self.quad(h)
        if h > t:
            return None
        if bnd[a] or bnd[b] or bnd[c] or bnd[d]:
            log['flip:frozen'] += 1
            return None
        if c == d:
            log['flip:c_is_d'] += 1
            return None
        if val[a] <= 3 or val[b] <= 3:
            log['flip:degree_ab_at_most_3'] += 1
            return None
        if val[c] + 1 > self.max_valence or val[d] + 1 > self.max_valence:
            log['flip:max_valence'] += 1
            return None
        before = abs(val[a] - 6) + abs(val[b] - 6) + abs(val[c] - 6) + abs(val[d] - 6)
        after = abs(val[a] - 7) + abs(val[b] - 7) + abs(val[c] - 5) + abs(val[d] - 5)
        if after >= before:
            log['flip:no_gain_now'] += 1
            return None
        rc, closed = self.ring(c)
        if not closed:
            log['flip:ring_of_c'] += 1
            return None
        if any(self.F[_nx(o)] == d for o in rc):
            log['flip:already_joined'] += 1
            return None
        n0, n1 = self._normal(a, b, c), self._normal(b, a, d)
        l0, l1 = _dot(n0, n0), _dot(n1, n1)
        if not l0 > 0 or not l1 > 0:
            log['flip:no_area'] += 1
            return None
        lhs, rhs = _dot(n0, n1), 0.3 * math.sqrt(l0 * l1)
        self._mg(lhs, rhs, _absdot(n0, n1) + abs(rhs), rounded=True)
        if lhs < rhs:
            log['flip:dihedral'] += 1
            return None
        m0, m1 = self._normal(a, d, c), self._normal(d, b, c)
        s0, s1 = 1.0 / math.sqrt(l0), 1.0 / math.sqrt(l1)
        navg = (n0[0] * s0 + n1[0] * s1, n0[1] * s0 + n1[1] * s1, n0[2] * s0 + n1[2] * s1)
        q0, q1 = _dot(m0, navg), _dot(m1, navg)
        self._mg(q0, 0.0, _absdot(m0, navg), rounded=True)
        if not q0 > 0:
            log['flip:orientation_0'] += 1
            return None
        self._mg(q1, 0.0, _absdot(m1, navg), rounded=True)
        if not q1 > 0:
            log['flip:orientation_1'] += 1
            return None
        nm0, nm1, na = _dot(m0, m0), _dot(m1, m1), _dot(navg, navg)
        r0 = 0.04 * nm0 * na
        self._mg(q0 * q0, r0, rounded=True)
        if q0 * q0 < r0:
            log['flip:skew'] += 1
            return None
        r1 = 0.04 * nm1 * na
        self._mg(q1 * q1, r1, rounded=True)
        if q1 * q1 < r1:
            log['flip:skew'] += 1
            return None
        amin = 0.01 * min(l0, l1)
        self._mg(nm0, amin)
        if nm0 < amin:
            log['flip:area'] += 1
            return None
        self._mg(nm1, amin)
        if nm1 < amin:
            log['flip:area'] += 1
            return None
        log['flip:bid'] += 1
        if max(val[c], val[d]) + 1 == self.max_valence:
            log['flip:bid_at_max_valence'] += 1            # (the flip brings c or d to max_valence exactly)
        return (a, b, c, d)

    # ---- writes (logged while a round's winners are applied) ----
    def _touch(self, hs=(), vs=()):
        if self._wh is not None:
            self._wh.update(hs)
            self._wv.update(vs)

    def split_apply(self, h, mv, f2, f3):
        F, twin, vhe, val = self.F, self.twin, self.vhe, self.val
        t, hn, hp, tn, tp, a, b, c, d = self.quad(h)
        hn_t, tn_t = twin[hn], twin[tn]
        pa, pb = self.P[a], self.P[b]
        self.P[mv] = ((pa[0] + pb[0]) * 0.5, (pa[1] + pb[1]) * 0.5, (pa[2] + pb[2]) * 0.5)
        val[mv], self.bnd[mv], vhe[mv] = 4, False, 3 * f2
        F[hn] = mv
        F[tn] = mv
        F[3 * f2:3 * f2 + 3] = [mv, b, c]
        F[3 * f3:3 * f3 + 3] = [mv, a, d]
        twin[h], twin[3 * f3] = 3 * f3, h
        twin[t], twin[3 * f2] = 3 * f2, t
        twin[hn], twin[3 * f2 + 2] = 3 * f2 + 2, hn
        twin[tn], twin[3 * f3 + 2] = 3 * f3 + 2, tn
        twin[3 * f2 + 1] = hn_t
        twin[3 * f3 + 1] = tn_t
        self._touch([h, t, hn, tn], [mv, c, d])
        if hn_t >= 0:
            twin[hn_t] = 3 * f2 + 1
            self._touch([hn_t])
        if tn_t >= 0:
            twin[tn_t] = 3 * f3 + 1
            self._touch([tn_t])
        if vhe[b] == hn:
            vhe[b] = 3 * f2 + 1
            self._touch(vs=[b])
        if vhe[a] == tn:
            vhe[a] = 3 * f3 + 1
            self._touch(vs=[a])
        val[c] += 1
        val[d] += 1
        self.n_split += 1

    def collapse_apply(self, h):
        F, twin, vhe, val = self.F, self.twin, self.vhe, self.val
        t, hn, hp, tn, tp, a, b, c, d = self.quad(h)
        rh, closed = self.ring(a)
        assert closed
        hn_t, hp_t, tn_t, tp_t = twin[hn], twin[hp], twin[tn], twin[tp]
        for o in rh:
            F[o] = b
        twin[hn_t], twin[hp_t] = hp_t, hn_t
        twin[tn_t], twin[tp_t] = tp_t, tn_t
        vhe[b] = tp_t
        if vhe[c] == hp:
            vhe[c] = hn_t
        if vhe[d] == tp:
            vhe[d] = tn_t
        for k in (h, hn, hp, t, tn, tp):
            F[k] = -1
            twin[k] = -1
        val[b] = val[a] + val[b] - 4
        val[c] -= 1
        val[d] -= 1
        val[a], vhe[a] = 0, -1
        self._touch(rh + [hn_t, hp_t, tn_t, tp_t, h, hn, hp, t, tn, tp], [a, b, c, d])
        self.n_collapse += 1

    def flip_apply(self, h):
        F, twin, vhe, val = self.F, self.twin, self.vhe, self.val
        t, hn, hp, tn, tp, a, b, c, d = self.quad(h)
        hn_t, tn_t = twin[hn], twin[tn]
        F[hn] = d
        F[tn] = c
        twin[h] = tn_t
        twin[t] = hn_t
        self._touch([h, t, hn, tn], [a, b, c, d])
        if tn_t >= 0:
            twin[tn_t] = h
            self._touch([tn_t])
        if hn_t >= 0:
            twin[hn_t] = t
            self._touch([hn_t])
        twin[hn], twin[tn] = tn, hn
        if vhe[a] == tn:
            vhe[a] = h
        if vhe[b] == hn:
            vhe[b] = t
        val[a] -= 1
        val[b] -= 1
        val[c] += 1
        val[d] += 1
        self.n_flip += 1

    # ---- a round ----
    def winners(self, bids):
        """bids: list of (list index, half-edge whose key is bid, footprint); a winner's key is the largest in every footprint vertex"""
        owner = {}
        keyed = []
        for i, e, fp in bids:
            k = key_of(self.seed, e)
            keyed.append((i, e, fp, k))
            for v in fp:
                if owner.get(v, 0) < k:
                    owner[v] = k
        return [(i, e, fp) for i, e, fp, k in keyed if all(owner[v] == k for v in fp)]

    def apply_checked(self, wins, do, nh0=None, nv0=None):
        """one after another in list order; the checks that let the device do them all at once (nh0, nv0: the sizes before the round)"""
        if not self.check:
            for w in wins:
                do(*w)
            return
        F0 = list(self.F)
        nh0, nv0 = len(F0) if nh0 is None else nh0, len(self.P) if nv0 is None else nv0
        taken = set()
        for w in wins:
            fp = set(w[2])
            assert not (fp & taken), 'two winners of a round share a footprint vertex'
            taken |= fp
            self._wh, self._wv = set(), set()
            do(*w)
            for v in self._wv:
                assert v in fp or v >= nv0, 'a write to vertex %d outside the footprint' % v
            for x in self._wh:
                assert x >= nh0 or (F0[x] in fp and F0[_nx(x)] in fp), 'a write to half-edge %d outside the footprint' % x
            self._wh = self._wv = None
        self.check_structure()

    def check_structure(self):
        F, T = np.asarray(self.F, np.int64), np.asarray(self.twin, np.int64)
        vhe, val, bnd = np.asarray(self.vhe, np.int64), np.asarray(self.val, np.int64), np.asarray(self.bnd, bool)
        h = np.nonzero(F >= 0)[0]
        t = T[h]
        m = t >= 0
        hm, tm = h[m], t[m]
        nxt = lambda x: np.where(x % 3 == 2, x - 2, x + 1)
        assert (T[tm] == hm).all() and (F[tm] >= 0).all(), 'twin is no involution on the live half-edges'
        assert (F[tm] == F[nxt(hm)]).all() and (F[nxt(tm)] == F[hm]).all(), 'a twin that does not run the other way'
        assert (T[F < 0] == -1).all()
        deg = np.bincount(F[h], minlength=vhe.shape[0])
        assert ((vhe >= 0) == (deg > 0)).all(), 'a vertex in use without vhe, or a vhe on a vertex of no face'
        u = np.nonzero(vhe >= 0)[0]
        assert (F[vhe[u]] == u).all(), 'a vhe that is no live outgoing half-edge of its vertex'
        n, closed = ring_lengths(F, T, vhe)
        whole = closed & ~bnd                              # (a bow-tie's val counts both fans, the walk one: frozen at set-up)
        assert (n[whole] == val[whole]).all() and (n[whole] == deg[whole]).all(), 'val is not the length of the ring'
        assert closed[u][~bnd[u] & (val[u] <= RING_MAX)].all(), 'an interior vertex whose fan does not close'

    def run_pass(self, kind):
        """returns the length of the candidate list"""
        lst = self.candidates(kind)
        n_list = len(lst)
        if not lst:
            return 0
        self.pass_seq += 1
        self.passes[kind] += 1
        bids_of = []
        for r in range(R_MAX[kind]):
            if not pass_goes_on(bids_of, r):
                break
            self.seed = (self.pass_seq * 64 + r) & _M32
            self.rounds[kind] += 1
            if kind == 0:
                bids = self.split_bids(lst)
                wins = self.winners(bids)
                nv0, nf0 = len(self.P), len(self.F) // 3
                W = len(wins)
                self.P += [None] * W
                self.vhe += [-1] * W
                self.val += [0] * W
                self.bnd += [False] * W
                self.F += [-1] * (6 * W)
                self.twin += [-1] * (6 * W)
                rank = {w[0]: k for k, w in enumerate(wins)}
                self.apply_checked(wins, lambda i, h, fp: self.split_apply(h, nv0 + rank[i], nf0 + 2 * rank[i], nf0 + 2 * rank[i] + 1), 3 * nf0, nv0)
            elif kind == 1:
                bids, keep = [], []
                for i, h in enumerate(lst):
                    got = self.collapse_bid(h)
                    if got is not None:
                        bids.append((i, got[0], got[1]))
                        keep.append(h)
                self.apply_checked(self.winners(bids), lambda i, e, fp: self.collapse_apply(e))
                if r == 0:
                    lst = keep                         # only the first round's bidders stay listed
            else:
                bids = []
                for i, h in enumerate(lst):
                    fp = self.flip_bid(h)
                    if fp is not None:
                        bids.append((i, h, fp))
                self.apply_checked(self.winners(bids), lambda i, h, fp: self.flip_apply(h))
            bids_of.append(len(bids))
        self.peak_valence = max(self.peak_valence, max(self.val))
        return n_list

    def relax(self, l):
        P, F = self.P, self.F
        upd = list(P)
        for v in range(len(P)):
            if self.vhe[v] < 0 or self.bnd[v] or self.val[v] < 3:
                continue
            rh, closed = self.ring(v)
            if not closed:
                continue
            p = P[v]
            gx = gy = gz = nx = ny = nz = 0.0
            for o in rh:
                x, y = P[F[_nx(o)]], P[F[_pv(o)]]
                gx, gy, gz = gx + x[0], gy + x[1], gz + x[2]
                c = _cross(_sub(x, p), _sub(y, p))
                nx, ny, nz = nx + c[0], ny + c[1], nz + c[2]
            s = 1.0 / len(rh)
            d = (gx * s - p[0], gy * s - p[1], gz * s - p[2])
            nrm = (nx, ny, nz)
            nn = _dot(nrm, nrm)
            tang = d
            if nn > 0:
                k = _dot(d, nrm) / nn
                tang = (d[0] - nx * k, d[1] - ny * k, d[2] - nz * k)
            upd[v] = (p[0] + tang[0] * l, p[1] + tang[1] * l, p[2] + tang[2] * l)
        self.P = upd

    def result(self):
        F = np.asarray(self.F, np.int64).reshape(-1, 3)
        P = np.asarray(self.P, np.float64).reshape(-1, 3)
        faces = F[F[:, 0] >= 0]
        used = np.zeros(P.shape[0], bool)
        used[faces.ravel()] = True
        slot = np.nonzero(used)[0]
        q = np.minimum(1023.0, np.maximum(0.0, (P[slot] - self.lo) * (1024.0 / self.ext))).astype(np.uint32)

        def spread(v):
            v = v & 0x3ff
            v = (v | (v << 16)) & 0x030000ff
            v = (v | (v << 8)) & 0x0300f00f
            v = (v | (v << 4)) & 0x030c30c3
            v = (v | (v << 2)) & 0x09249249
            return v
        key = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
        order = np.argsort(key, kind='stable')
        new_id = np.full(P.shape[0], -1, np.int64)
        new_id[slot[order]] = np.arange(slot.size)
        e = np.sqrt(((P[faces] - P[np.roll(faces, -1, 1)]) ** 2).sum(2))
        mean = float(e.sum() / (3.0 * faces.shape[0])) if faces.shape[0] else 0.0
        val = np.asarray(self.val, np.int64)
        return P[slot[order]].astype(np.float32), new_id[faces].astype(np.int32), mean, int(val[slot].max()) if slot.size else 0


def remesh_device_ref(v, f, n, L, l=0.5, n_relax=0, max_valence=16, check=True):
    m = _Mesh(v, f, L, max_valence, check)
    l = float(np.float32(l))
    if check:
        m.check_structure()
    for _ in range(int(n)):
        before = (m.n_split, m.n_collapse, m.n_flip)
        first_list = 0
        for sweep in range(4):
            n_list = m.run_pass(0)
            if n_list == 0:
                break
            if sweep == 0:
                first_list = n_list
            if sweeps_end(n_list, first_list):
                break
        m.run_pass(1)
        m.run_pass(2)
        for _k in range(int(n_relax)):
            m.relax(l)
        if iterations_end(n_relax, before, (m.n_split, m.n_collapse, m.n_flip)):
            break
    ov, of, mean, mv = m.result()
    info = dict(n_split=m.n_split, n_collapse=m.n_collapse, n_flip=m.n_flip, rounds=tuple(m.rounds), passes=tuple(m.passes), max_valence=mv,
                mean_edge_length=mean, margin=m.margin, margin_nonzero=m.margin_nonzero, margin_rounded=m.margin_rounded, peak_valence=m.peak_valence, log=dict(m.log), frozen=int(sum(m.bnd)))
    return ov, of, info
