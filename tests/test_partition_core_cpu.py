"""
The rules of the query's k-d work list, without a GPU: ch_shrinkwrap_amd/csrc/nw_partition_core.h.  The stand-alone program of
tests/partition_ref.py (its own main around the header's host restatement of the whole partition) is built with g++ plain and with
-fsanitize=address,undefined and run on small clouds; it partitions every input twice and fails if the two runs differ.  What it leaves
is checked here: a permutation, leaves that tile [0, n), full leaves but one per start segment, faces in order inside a leaf -- and, on the
inputs made for it, which localizations the cuts put together.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import partition_ref as P

BUILDS = {'plain': [], 'address_undefined': ['-fsanitize=address,undefined']}
CAP = 4096


def cloud(n, seed):
    """n foot points on a sphere, heights in +-25, a few hundred faces; in the order of their Morton keys"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    foot = np.concatenate([100.0 * d, rng.uniform(-25, 25, (n, 1))], 1).astype(np.float32)
    face = rng.integers(0, 320, n).astype(np.int32)
    key = P.morton_keys(foot[:, :3], -128.0, 0.25)
    o = np.argsort(key, kind='stable')
    return key[o], foot[o], face[o]


def one_block(foot, face=None):
    n = len(foot)
    return np.zeros(n, np.uint32), np.asarray(foot, np.float32), np.zeros(n, np.int32) if face is None else np.asarray(face, np.int32)


def _cases():
    c = {}
    for n in (1, 63, 64, 65, 128, 129, 4097):
        c['sphere-%d' % n] = cloud(n, n) + (64, CAP)
    c['sphere-33-leaf32'] = cloud(33, 33) + (32, CAP)
    c['sphere-4097-cap256'] = cloud(4097, 4097) + (64, 256)
    c['sphere-4097-part'] = cloud(4097, 4097) + (64, CAP)
    # all points identical: one Morton block at every level, larger than the cap: cut into runs
    c['identical-4097'] = one_block(np.tile(np.float32([3.0, -2.0, 7.0, 1.5]), (4097, 1)), np.arange(4097)[::-1] % 7) + (64, CAP)
    c['identical-129'] = one_block(np.tile(np.float32([3.0, -2.0, 7.0, 1.5]), (129, 1)), np.arange(129)[::-1] % 7) + (64, CAP)
    # an axis-parallel line (y), shuffled
    rng = np.random.default_rng(5)
    line = np.zeros((300, 4), np.float32)
    line[:, 1] = rng.permutation(300).astype(np.float32)
    c['line-300'] = one_block(line) + (64, CAP)
    # equal coordinates on both sides of the cut rank 64: 32 x 0, 64 x 1, 32 x 2 on x, shuffled
    st = np.zeros((128, 4), np.float32)
    st[:, 0] = rng.permutation(np.repeat([0.0, 1.0, 2.0], [32, 64, 32]))
    c['straddle-128'] = one_block(st) + (64, CAP)
    c['straddle-128-part'] = one_block(st) + (64, CAP)
    # a NaN height (and an infinite one): they count as height 0
    key, foot, face = cloud(200, 9)
    foot[17, 3] = np.nan
    foot[90, 3] = np.inf
    c['nan-height-200'] = (key, foot, face, 64, CAP)
    zero = foot.copy()
    zero[[17, 90], 3] = 0.0
    c['zero-height-200'] = (key, zero, face, 64, CAP)
    return c


CASES = _cases()


@pytest.fixture(scope='module', params=list(BUILDS))
def results(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp('partition_' + request.param))
    flags = BUILDS[request.param]
    if flags:
        one = os.path.join(d, 'one.cpp')
        with open(one, 'w') as fh:
            fh.write('int main() { return 0; }\n')
        if subprocess.run([P.CXX] + flags + ['-o', os.path.join(d, 'one'), one], capture_output=True).returncode != 0:
            pytest.skip('%s cannot link a program with %s' % (P.CXX, ' '.join(flags)))
    exe = P.build(d, flags)
    # (the clouds whose name says so are cut with a sort_max of 100: their first levels part instead of sorting)
    return {name: P.run(exe, d, key, foot, face, leaf, cap, 0.5, 100 if 'part' in name else 1024) for name, (key, foot, face, leaf, cap) in CASES.items()}


def test_the_header_includes_no_hip_header():
    txt = open(P.HEADER).read()
    assert 'hip_runtime' not in txt and '#include <hip' not in txt
    assert not re.search(r'\bhip[A-Z]\w*\s*\(', txt)


@pytest.mark.parametrize('name', list(CASES))
def test_partition_properties(results, name):
    key, foot, face, leaf, cap = CASES[name]
    n = len(key)
    level, order, seg_start, leaf_start = results[name]
    assert sorted(order.tolist()) == list(range(n))                                   # a permutation
    assert leaf_start[0] == 0 and leaf_start[-1] == n and (np.diff(leaf_start) > 0).all()      # the leaves tile [0, n)
    assert seg_start[0] == 0 and seg_start[-1] == n and (np.diff(seg_start) > 0).all()
    assert np.diff(seg_start).max() <= cap
    assert np.isin(seg_start, leaf_start).all()                                       # no leaf crosses a start segment
    sizes = np.diff(leaf_start)
    assert sizes.max() <= leaf
    for s0, s1 in zip(seg_start[:-1], seg_start[1:]):                                 # ... and all leaves of a segment but its last are full
        mine = sizes[(leaf_start[:-1] >= s0) & (leaf_start[:-1] < s1)]
        assert (mine[:-1] == leaf).all() and len(mine) == -(-(s1 - s0) // leaf)
        assert sorted(order[s0:s1].tolist()) == list(range(s0, s1))                   # nothing leaves its start segment
    assert len(sizes) <= -(-n // leaf) + len(seg_start) - 1
    # start segments are whole Morton blocks of the chosen level, or runs of one block that is too large at level 0
    blocks = key >> np.uint32(3 * level)
    for s0, s1 in zip(seg_start[:-1], seg_start[1:]):
        assert (blocks[s0:s1] == blocks[s0]).all()
    heads = np.flatnonzero(np.diff(blocks)) + 1
    assert np.isin(heads, seg_start).all()
    for l0, l1 in zip(leaf_start[:-1], leaf_start[1:]):                               # inside a leaf: by face id, then by the order before
        f = face[order[l0:l1]]
        assert (np.diff(f) >= 0).all()


def test_identical_points_keep_their_order_up_to_the_faces(results):
    """no extent on any axis: every key is 0, every sort keeps the order, and a leaf is its run of positions ordered by face"""
    for name in ('identical-129', 'identical-4097'):
        key, foot, face, leaf, cap = CASES[name]
        level, order, seg_start, leaf_start = results[name]
        assert level == (0 if len(key) > cap else 10)
        for l0, l1 in zip(leaf_start[:-1], leaf_start[1:]):
            assert order[l0:l1].tolist() == (l0 + np.argsort(face[l0:l1], kind='stable')).tolist()


def test_a_line_is_cut_into_intervals(results):
    key, foot, face, leaf, cap = CASES['line-300']
    level, order, seg_start, leaf_start = results['line-300']
    y = foot[order, 1]
    assert np.diff(leaf_start).tolist() == [64, 64, 64, 64, 44]
    for a, b, c in zip(leaf_start[:-2], leaf_start[1:-1], leaf_start[2:]):
        assert y[a:b].max() < y[b:c].min()


def test_equal_coordinates_across_the_cut_keep_their_order(results):
    key, foot, face, leaf, cap = CASES['straddle-128']
    level, order, seg_start, leaf_start = results['straddle-128']
    assert order.tolist() == np.argsort(foot[:, 0], kind='stable').tolist()           # (one face: the leaves keep the sorted order)
    # parted instead of sorted: the same 64 go left (all zeros and the first 32 ones), and both halves keep the order they came in
    order = results['straddle-128-part'][1]
    by_key = np.argsort(foot[:, 0], kind='stable')
    assert order[:64].tolist() == sorted(by_key[:64].tolist()) and order[64:].tolist() == sorted(by_key[64:].tolist())


def test_a_non_finite_height_counts_as_zero(results):
    """the same cloud with those heights written as 0 partitions alike"""
    assert results['nan-height-200'][1].tolist() == results['zero-height-200'][1].tolist()
