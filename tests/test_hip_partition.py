"""
GPU tests (run with -m gpu on an MI355X) of the query's k-d work list: the device partition of the second sort against the host
restatement of csrc/nw_partition_core.h, element for element, on small clouds over a sphere of 320 faces; and the exactness of the
nearest faces through the new layout on C1's shape, against a float64 brute force, with the list on (the default) and off
(NW_KD_SORT=0, read once per process: a child process).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import partition_ref as P
from conftest import ROOT, rel_rms

pytestmark = pytest.mark.gpu

CAP = 16384                 # NWP_CAP of csrc/nw_partition.h


def _cloud(kind, n):
    from ch_shrinkwrap_amd.synth import sphere_cloud
    if kind == 'sphere':
        return sphere_cloud(n, 100.0, 10.0, seed=n)
    if kind == 'identical':
        return np.tile(np.float32([60.0, -50.0, 70.0]), (n, 1))
    if kind == 'line':                                          # parallel to y, through the sphere
        p = np.zeros((n, 3), 'f4')
        p[:, 0], p[:, 2] = 30.0, 95.0
        p[:, 1] = np.random.default_rng(5).permutation(n).astype('f4') * (150.0 / n) - 75.0
        return p
    if kind == 'duplicates':                                    # every position four times: equal coordinates on both sides of a cut
        return np.repeat(sphere_cloud(n // 4, 100.0, 10.0, seed=3), 4, axis=0)[np.random.default_rng(2).permutation(n // 4 * 4)]
    if kind == 'masked':                                        # (two of them get zero weights below: masked localizations)
        return sphere_cloud(n, 100.0, 10.0, seed=9)
    raise ValueError(kind)


CASES = [('sphere', n, 64) for n in (1, 63, 64, 65, 128, 129, 4097)] + [('sphere', 33, 32), ('identical', 4097, 64), ('identical', 16385, 64), ('line', 300, 64),
                                                                        ('duplicates', 128, 64), ('masked', 200, 64)]


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('partition_gpu'))
    return P.build(d), d


@pytest.mark.parametrize('kind,n,leaf', CASES, ids=['%s-%d-leaf%d' % c for c in CASES])
def test_device_partition_equals_the_restatement(program, monkeypatch, kind, n, leaf):
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    from ch_shrinkwrap_amd.mesh_conj_grad import ShrinkwrapMeshConjGrad
    exe, d = program
    monkeypatch.setenv('NW_KD_KEEP', '1')
    monkeypatch.setenv('NW_ITEM_PTS', str(leaf))
    v, f = icosphere(2, 110.0)
    assert f.shape[0] == 320
    pts = np.ascontiguousarray(_cloud(kind, n), 'f4')
    cg = ShrinkwrapMeshConjGrad(TriMesh(v, f), pts)
    weights = None
    if kind == 'masked':
        weights = np.ones(pts.size, 'f4')
        weights[3 * 17:3 * 18] = 0.0
        weights[3 * 90 + 1] = 0.0
    cg.search(pts, lams=[10.0], num_iters=2, sigma_inv=0.1, weights=weights)
    cg.search(pts, lams=[10.0], num_iters=1, sigma_inv=0.1, weights=weights)      # the second block begins with the second sort; nothing re-orders its list yet
    perm, info, items = P.layout(cg)
    assert info['leaf'] == leaf and info['leaves'] == len(items)
    key, foot, face, perm_in = P.partition_inputs(cg)
    assert (np.diff(key.astype(np.int64)) >= 0).all() and sorted(perm_in.tolist()) == list(range(n))
    level, order, seg_start, leaf_start = P.run(exe, d, key, foot, face, leaf, CAP // leaf * leaf, info['w'])
    assert info['level'] == level and info['segments'] == len(seg_start) - 1
    assert np.array_equal(items[:, 0], leaf_start[:-1]) and np.array_equal(items[:, 1], np.diff(leaf_start))
    assert np.array_equal(perm, perm_in[order])


@pytest.fixture(scope='module')
def c1_runs(tmp_path_factory):
    """the same two blocks with the k-d list (in this process) and without it (a child process)"""
    on = P.run_c1()
    out = os.path.join(str(tmp_path_factory.mktemp('partition_c1')), 'off.npz')
    env = dict(os.environ, NW_KD_SORT='0', PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests')] + os.environ.get('PYTHONPATH', '').split(os.pathsep)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'partition_ref.py'), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return on, dict(np.load(out))


@pytest.fixture(scope='module')
def c1_brute():
    """-> function(positions) = (float64 argmin over all centroids with the lowest face id on ties, how many localizations are tied)"""
    from oracle import nanowrap_oracle as O
    v, nrm, nbr, faces, pts, weights = P.c1_scene()
    cache = {}

    def brute(pos):
        k = pos.tobytes()
        if k not in cache:
            cent = O.face_centroids(pos, faces).astype('f8')
            want, ties = np.full(len(pts), -1, np.int64), 0
            for c0 in range(0, len(pts), 1000):
                i = np.arange(c0, min(c0 + 1000, len(pts)))
                p = pts[i].astype('f8')
                d2 = (p[:, None, 0] - cent[None, :, 0]) ** 2 + (p[:, None, 1] - cent[None, :, 1]) ** 2 + (p[:, None, 2] - cent[None, :, 2]) ** 2
                want[i] = d2.argmin(1)                          # (the first of equal minima: the lowest id)
                ties += int(((d2 == d2.min(1, keepdims=True)).sum(1) > 1).sum())
            cache[k] = (want, ties)
        return cache[k]
    return brute


@pytest.mark.parametrize('which', ['kd', 'kd_off'])
def test_nearest_faces_are_exact_through_the_layout(c1_runs, c1_brute, which):
    run = c1_runs[0 if which == 'kd' else 1]
    want, ties = c1_brute(np.ascontiguousarray(run['out1'], 'f4'))
    print('%s: %d localizations exactly equidistant from two centroids' % (which, ties))
    assert ties >= 2
    wrong = np.flatnonzero(run['face'] != want)
    assert wrong.size == 0, (wrong[:10], run['face'][wrong[:10]], want[wrong[:10]])


def test_the_two_layouts_give_the_same_fit(c1_runs):
    on, off = c1_runs
    assert np.isfinite(on['out2']).all()
    # (the bound tests/test_hip_parity.py puts on the vertex RMS against the oracle, relative to the bounding-box diagonal)
    print('vertex RMS between the layouts: %.3e after one block, %.3e after two' % (rel_rms(on['out1'], off['out1']), rel_rms(on['out2'], off['out2'])))
    assert rel_rms(on['out2'], off['out2']) <= 1e-4


def test_the_work_list_of_the_layout(c1_runs):
    on, off = c1_runs
    N = 10000
    leaves, segments, level, leaf = (int(x) for x in on['kd'])
    assert leaf == 32 and leaves > 0 and segments > 0
    assert leaves <= -(-N // leaf) + segments
    assert int(off['kd'][0]) == 0                                  # NW_KD_SORT=0: no such list
    assert sorted(on['perm'].tolist()) == list(range(N))
    # the query's list on top of it (a small cloud's heavy leaves are cut into pieces): still tiles [0, N) in runs of at most a leaf
    items = on['items'][np.argsort(on['items'][:, 0])]
    assert items[0, 0] == 0 and np.array_equal(items[:-1, 0] + items[:-1, 1], items[1:, 0]) and items[-1, 0] + items[-1, 1] == N
    assert items[:, 1].max() <= leaf and len(items) >= leaves
