#!/usr/bin/env python3
"""
CPU model of which 64 localizations share a wave of the nearest-face query (no GPU; NumPy and SciPy only).

The cost of a wave is set by the union of its lanes' balls (localization, distance to its nearest centroid): the bounding box of the
balls is what the walk visits, the cells some ball reaches are what every lane streams.  This script cuts the work list of a
configuration (default C3: synth.make_config('c3', seed=0), the zero-level mesh, 10 nm cells, Morton unit = extent / 1024) in several
ways and counts, over a sample of waves scaled to the whole list:

  candidates   centroids in the non-empty cells some lane's ball reaches
  reached      those cells
  box          the non-empty cells in the bounding box of the lanes' balls
  faces        distinct nearest faces in a wave

Lanes far out (r^2 > 6.25 mean r^2 and r > 1.5 cells, at most 8 of them) are left out of the union, as the kernel resolves them apart.
The k-d lists follow ch_shrinkwrap_amd/csrc/nw_partition_core.h (widest axis of the segment's box, 16-bit keys, cut rank a whole number of
leaves, stable), with every segment sorted -- the parting of large segments gives the same leaves up to ties.

    python tools/partition_model.py [--config c3] [--cell 10] [--waves 1500] [--levels-up 2]
"""
import argparse
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEAF = 64


def morton(q):
    key = np.zeros(len(q), np.uint32)
    for b in range(10):
        for a in range(3):
            key |= (((q[:, a] >> b) & 1) << (3 * b + a)).astype(np.uint32)
    return key


def blocks_of(key, level):
    """[start, end) of the aligned Morton blocks of a sorted key list"""
    b = key >> np.uint32(3 * level)
    heads = np.concatenate([[0], np.flatnonzero(np.diff(b)) + 1, [len(key)]])
    return list(zip(heads[:-1], heads[1:]))


def todays_list(key, level):
    out = []
    for p0, p1 in blocks_of(key, level):
        n = -(-(p1 - p0) // LEAF)
        per = -(-(p1 - p0) // n)
        out += [(p, min(p + per, p1)) for p in range(p0, p1, per)]
    return np.arange(len(key)), out


def kd_list(key, level, coords):
    """coords: (N, k) float32 in key order -> (order, leaves)"""
    order = np.arange(len(key))
    leaves = []

    def split(s0, n):
        if n <= LEAF:
            return
        c = coords[order[s0:s0 + n]]
        lo, hi = c.min(0), c.max(0)
        ext = hi - lo
        a = int(np.argmax(ext))                                   # (the first of equal maxima: the lowest axis)
        if ext[a] > 0:
            k16 = np.minimum(((c[:, a] - lo[a]) * (np.float32(65535.0) / ext[a])).astype(np.int64), 65535)
            order[s0:s0 + n] = order[s0:s0 + n][np.argsort(k16, kind='stable')]
        nl = (-(-n // LEAF) // 2) * LEAF
        split(s0, nl)
        split(s0 + nl, n - nl)

    for p0, p1 in blocks_of(key, level):
        split(p0, p1 - p0)
        leaves += [(p, min(p + LEAF, p1)) for p in range(p0, p1, LEAF)]
    return order, leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='c3')
    ap.add_argument('--cell', type=float, default=10.0)
    ap.add_argument('--waves', type=int, default=1500)
    ap.add_argument('--levels-up', type=int, default=2, help='start segments of the k-d lists: Morton blocks this many levels above the item level')
    args = ap.parse_args()
    from ch_shrinkwrap_amd import synth
    cfg = synth.make_config(args.config, seed=0)
    pts = cfg['points'].astype(np.float32)
    v, f = cfg['surface']
    cent = v[f].astype(np.float64).mean(1).astype(np.float32)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    nrm = np.cross(e1, e2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    r, face = cKDTree(cent).query(pts, workers=-1)
    foot = cent[face]
    height = ((pts - foot) * nrm[face]).sum(1).astype(np.float32)
    lo = np.minimum(pts.min(0), cent.min(0))
    ext = float((np.maximum(pts.max(0), cent.max(0)) - lo).max())
    unit = ext / 1024.0
    key = morton(np.clip(((foot - lo) / unit).astype(np.int64), 0, 1023))
    o = np.argsort(key, kind='stable')
    key, pts, foot, height, face, r = key[o], pts[o], foot[o], height[o], face[o], r[o]
    level = int(np.clip(round(np.log2(max(4.0 * args.cell / unit, 1.0))), 0, 10))
    # the centroid grid
    h = args.cell
    cq = np.floor((cent - lo) / h).astype(np.int64)
    dims = cq.max(0) + 1
    cid = (cq[:, 2] * dims[1] + cq[:, 1]) * dims[0] + cq[:, 0]
    count = np.bincount(cid, minlength=int(dims.prod()))
    grid = count.reshape(dims[2], dims[1], dims[0])

    def wave_cost(idx):
        p, rr = pts[idx].astype(np.float64), r[idx]
        far = (rr ** 2 > 6.25 * (rr ** 2).mean()) & (rr > 1.5 * h)
        if far.sum() > 8:
            far[np.argsort(-rr)[8:]] = False
        p, rr = p[~far], rr[~far]
        blo = np.clip(np.floor((p - rr[:, None] - lo).min(0) / h).astype(int), 0, dims - 1)
        bhi = np.clip(np.floor((p + rr[:, None] - lo).max(0) / h).astype(int), 0, dims - 1)
        sub = grid[blo[2]:bhi[2] + 1, blo[1]:bhi[1] + 1, blo[0]:bhi[0] + 1]
        zz, yy, xx = np.nonzero(sub)
        c0 = lo + (np.stack([xx + blo[0], yy + blo[1], zz + blo[2]], 1)) * h          # the non-empty cells' low corners
        reached = np.zeros(len(c0), bool)
        for q, rq in zip(p, rr):
            d = np.maximum(np.maximum(c0 - q, q - (c0 + h)), 0.0)
            reached |= (d ** 2).sum(1) <= rq * rq
        return sub[zz, yy, xx][reached].sum(), int(reached.sum()), len(c0), len(np.unique(face[idx]))

    rng = np.random.default_rng(0)
    c4 = np.concatenate([foot, (0.5 * height)[:, None]], 1).astype(np.float32)
    blend = (foot + 0.5 * (pts - foot)).astype(np.float32)
    lists = [('today: Morton runs inside aligned blocks', todays_list(key, level)),
             ('plain runs of 64 of the same order', (np.arange(len(key)), [(p, min(p + LEAF, len(key))) for p in range(0, len(key), LEAF)])),
             ('k-d of the foot points', kd_list(key, min(level + args.levels_up, 10), foot)),
             ('k-d of foot x, y, z and 0.5 x signed height', kd_list(key, min(level + args.levels_up, 10), c4)),
             ('k-d of the blend foot + 0.5 (p - foot)', kd_list(key, min(level + args.levels_up, 10), blend))]
    print('%s: %d localizations, %d centroids, cell %.1f, Morton unit %.3f, item level %d' % (args.config, len(pts), len(cent), h, unit, level))
    print('%-46s %7s %12s %10s %10s %7s' % ('work list', 'waves', 'candidates', 'reached', 'box', 'faces'))
    for name, (order, leaves) in lists:
        pick = rng.choice(len(leaves), min(args.waves, len(leaves)), replace=False)
        tot = np.array([wave_cost(order[leaves[k][0]:leaves[k][1]]) for k in pick], np.float64).mean(0)
        n = len(leaves)
        print('%-46s %7d %11.2fM %9.0fk %9.0fk %7.1f' % (name, n, tot[0] * n / 1e6, tot[1] * n / 1e3, tot[2] * n / 1e3, tot[3]))


if __name__ == '__main__':
    main()
