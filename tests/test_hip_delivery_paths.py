"""
GPU test (run with -m gpu on an MI355X) of the ways a block's result reaches the host, through the C-ABI: straight from the block's last
kernel into the staging buffer (the default below 4 MB), in slices announced through the flag word (NW_DIRECT_OUT=0), and as
device-to-host copies that host threads wait for on events (NW_SPIN_WAIT=0) -- each into a contiguous `pos_out` and into strided vertex
records under a valid mask, and the sliced one also with the records written behind the caller's back (NW_FLAG_ROWS_ASYNC).  The knobs
are read once per process: every variant is a child process of its own.  The children run with NW_VERBOSE=3, which changes no result:
nw_search_end then names the path it took on stderr, and that line is what tells the flag-word path from the one on events (the counters
of nw_debug cannot: both count one write-back).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# (name, environment, NW_FLAG_ROWS_ASYNC, (staged copy-outs, write-backs) the block must count: nw_debug, what = 2, what nw_search_end says)
SAYS_DIRECT, SAYS_SLICED, SAYS_EVENTS = 'copy-out of the staged result alone', '3 slices through the flag word', 'wait + sliced write-back'
VARIANTS = [
    ('direct', {}, False, (1, 0), SAYS_DIRECT),
    ('sliced', {'NW_DIRECT_OUT': '0', 'NW_SLICE_ROWS': '4096'}, False, (0, 1), SAYS_SLICED),
    ('events', {'NW_DIRECT_OUT': '0', 'NW_SPIN_WAIT': '0', 'NW_WB_ROWS_PER_THREAD': '1000'}, False, (0, 1), SAYS_EVENTS),      # eight slices
    ('sliced_rows_async', {'NW_DIRECT_OUT': '0', 'NW_SLICE_ROWS': '4096'}, True, (0, 1), SAYS_SLICED),
]
STRIDE, SENTINEL = 40, 0xA5

CHILD = r'''
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from ch_shrinkwrap_amd import _lib as nw
from ch_shrinkwrap_amd.mesh_conj_grad import NativeContext
from ch_shrinkwrap_amd.synth import sphere_cloud
from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
out_path, rows_async, want_staged, want_write_backs = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
STRIDE, SENTINEL = %d, %d
v, f = icosphere(5, 120.0)
mesh = TriMesh(v, f)
M = v.shape[0]
assert M == 10242
pos = np.ascontiguousarray(mesh.vertices, 'f4')
nrm = np.ascontiguousarray(mesh.vertex_normals, 'f4')
nbr = np.ascontiguousarray(mesh.neighbor_vertex_table(), 'i4')
faces = np.ascontiguousarray(mesh.faces, 'i4')
valid = np.ones(M, 'u1')
valid[::7] = 0
pts = np.ascontiguousarray(sphere_cloud(4000, 100.0, 10.0, seed=7), 'f4')
nat = NativeContext(0)
L, h = nat.L, nat.h
nat.check(L.nw_set_mesh(h, nw.ptr(pos), nw.ptr(nrm), nw.ptr(nbr), nw.ptr(valid), nw.ptr(faces), M, faces.shape[0], nbr.shape[1]))
nat.check(L.nw_set_points(h, nw.ptr(pts), pts.shape[0], None, 0.1, nw.NW_WEIGHTS_FROM_SIGMA_INV, None, 1.0))
records = np.full((M, STRIDE), SENTINEL, np.uint8)
pos_out = np.full((M, 3), np.nan, 'f4')
nat.check(L.nw_set_write_back(h, nw.ptr(records), STRIDE))
lams = np.array([10.0], 'f4')
logs = (nw.IterLog * 5)()
lc = ctypes.c_int(0)
n0, n1 = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
nat.check(L.nw_debug(h, 2, n0, None, 0, None))
nat.check(L.nw_search(h, nw.ptr(lams), 1, 5, nw.NW_FLAG_ROWS_ASYNC if rows_async else 0, nw.ptr(pos_out), logs, ctypes.byref(lc)))
if rows_async:
    nat.check(L.nw_synchronize(h))              # (the records are complete behind this)
nat.check(L.nw_debug(h, 2, n1, None, 0, None))
nat.check(L.nw_set_write_back(h, None, 0))
assert lc.value == 5, lc.value
assert (n1[0] - n0[0], n1[1] - n0[1]) == (want_staged, want_write_backs), (n1[0] - n0[0], n1[1] - n0[1])
dev = np.empty((M, 3), 'f4')
nat.check(L.nw_get(h, nw.NW_ARR_POS, nw.ptr(dev), dev.nbytes))
assert np.isfinite(dev).all() and not np.array_equal(dev, pos)
assert pos_out.tobytes() == dev.tobytes(), 'pos_out differs from the estimate on the device'
ok = valid != 0
assert records[ok, :12].tobytes() == dev.view(np.uint8).reshape(M, 12)[ok].tobytes(), 'records of valid vertices'
assert (records[ok, 12:] == SENTINEL).all() and (records[~ok] == SENTINEL).all(), 'bytes outside the valid position rows were written'
np.save(out_path, np.concatenate([pos_out.view(np.uint8).reshape(M, 12), records], 1))
nat.close()
print('OK')
''' % (ROOT, STRIDE, SENTINEL)


def run_variants(out_dir):
    """every variant in a fresh child under its own time limit, one after the other (a child that fails ends the run: nothing more is started
    on the device) -> {name: (M, 12 + STRIDE) uint8: pos_out's bytes and the records}"""
    got = {}
    for name, knobs, rows_async, (staged, write_backs), says in VARIANTS:
        env = dict(os.environ, NW_VERBOSE='3', **knobs)
        out = os.path.join(str(out_dir), name + '.npy')
        r = subprocess.run([sys.executable, '-c', CHILD, out, str(int(rows_async)), str(staged), str(write_backs)], env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip().endswith('OK'), (name, r.returncode, r.stderr[-2000:])
        took = [t for t in (SAYS_DIRECT, SAYS_SLICED, SAYS_EVENTS) if t in r.stderr]
        assert took == [says], (name, took, r.stderr[-2000:])
        got[name] = np.load(out)
    return got


def test_every_delivery_path_hands_back_the_same_result(tmp_path):
    """In every child: pos_out equals the device's estimate byte for byte, the records equal it where `valid` is set and keep their sentinel
    elsewhere, and the block took the path its knobs name.  Here: the four children's results are identical."""
    got = run_variants(tmp_path)
    first = got[VARIANTS[0][0]]
    for name in [v[0] for v in VARIANTS[1:]]:
        assert got[name].tobytes() == first.tobytes(), name
