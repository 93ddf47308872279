"""CPU test: libnanowrap_hip.so exports every function include/nw_skeleton.h declares, the binding names the same set and repeats its
constants, the unit is built without fma contraction as an object of its own on its core header, its kernels have budget rows and stay
within them without scratch at eight waves per SIMD, the calls check their arguments before they touch a GPU and write nothing when they
refuse, the host layer on top works on plain arrays, and nothing falls back to the host."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import mesh_skeleton_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ['k_sk_bands', 'k_sk_totals', 'k_sk_init', 'k_sk_hook', 'k_sk_compress', 'k_sk_number', 'k_sk_sums', 'k_sk_arcs', 'k_sk_vertex']


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'nw_skeleton.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(nwa_[a-zA-Z0-9_]+)\s*\(', txt)))


def test_library_exports_the_skeleton_header():
    from ch_shrinkwrap_amd import build, _lib, skeleton
    build.build_hip_library()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ['nwa_abi_version', 'nwa_create', 'nwa_destroy', 'nwa_fetch', 'nwa_last_error', 'nwa_set_mesh', 'nwa_skeleton']
    for n in names:
        assert hasattr(L, n), 'libnanowrap_hip.so does not export %s' % n
    assert sorted(skeleton.SYMBOLS) == names
    assert skeleton.load().nwa_abi_version() == skeleton.ABI_VERSION == 1
    txt = open(os.path.join(ROOT, 'include', 'nw_skeleton.h')).read()
    for i, name in enumerate(skeleton.INFO_NAMES):
        assert int(re.search(r'#define NWA_INFO_%s\s+(\d+)' % name.upper(), txt).group(1)) == i
    assert int(re.search(r'#define NWA_INFO_WORDS\s+(\d+)', txt).group(1)) == skeleton.NWA_INFO_WORDS >= len(skeleton.INFO_NAMES)
    assert int(re.search(r'#define NWA_SUM_COLUMNS\s+(\d+)', txt).group(1)) == skeleton.NWA_SUM_COLUMNS == R.COLUMNS
    assert int(re.search(r'#define NWA_FLAG_TIMING\s+(\d+)', txt).group(1)) == skeleton.NWA_FLAG_TIMING
    for name in ('BADARG', 'HIP', 'NONFINITE', 'NOMEM', 'NOMESH', 'NORESULT'):
        assert int(re.search(r'NWA_ERR_%s = (-\d+)' % name, txt).group(1)) == getattr(skeleton, 'NWA_ERR_' + name)
        assert getattr(skeleton, 'NWA_ERR_' + name) in skeleton.ERRORS
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_skeleton_core.h')).read()
    for name, value in (('NWA_MAX_N', 'MAX_N'), ('NWA_MAX_FACES', 'MAX_FACES'), ('NWA_MAX_BAND', 'MAX_BAND'), ('NWA_MAX_PIECES', 'MAX_PIECES')):
        shift = int(re.search(r'#define %s \(1ll << (\d+)\)' % name, core).group(1))
        assert 1 << shift == getattr(skeleton, value) and (value not in ('MAX_BAND', 'MAX_PIECES') or 1 << shift == getattr(R, value))
    for name, col in (('PIECES', 0), ('CENTROID', 1), ('SEGMENTS', 4), ('LENGTH', 5), ('MOMENT_LO', 6), ('MOMENT_HI', 9)):
        assert int(re.search(r'#define NWA_S_%s\s+(\d+)' % name, core).group(1)) == col == getattr(skeleton, 'S_' + name) == getattr(R, 'S_' + name)
    assert int(re.search(r'#define NWA_COORD_BITS\s+(\d+)', core).group(1)) == skeleton.COORD_BITS == R.COORD_BITS
    assert int(re.search(r'#define NWA_LEN_SHIFT\s+(\d+)', core).group(1)) == skeleton.LEN_SHIFT == R.LEN_SHIFT
    # the scheduling-dependent info words are named as such, in the header and in the binding
    assert 'NOT DETERMINISTIC' in txt and {'hook_retries', 'atomics', 'hook_us', 'dedup_us'} <= set(skeleton.NOT_DETERMINISTIC)
    assert not set(skeleton.NOT_DETERMINISTIC) & {'pieces', 'nodes', 'arcs', 'segments', 'live_faces', 'live_vertices', 'max_band', 'arc_keys'}
    # what the skeleton is not, where a reader meets it first
    for doc in (txt, core):
        flat = re.sub(r'[\s/*]+', ' ', doc)
        assert 'LOOP NARROWER THAN A BAND VANISHES' in flat and 'depends on the field' in flat
    assert 'Proof that no sum' in core and 'What it costs' in core


def test_unit_is_built_without_contraction_and_budgeted():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    unit = [u for u in build.UNITS if u[1] == build.OBJ_SKELETON]
    assert len(unit) == 1 and '-ffp-contract=off' in unit[0][3] and unit[0][3] == build._QUERY
    assert unit[0][0].endswith('nw_skeleton.hip') and build.OBJ_SKELETON.endswith('nw_skeleton.o')
    deps = unit[0][2]
    assert os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_skeleton_core.h') in deps
    assert os.path.join(ROOT, 'include', 'nw_skeleton.h') in deps and set(build._BQ_H) <= set(deps)
    assert build.OBJ_SKELETON in build.BUDGETED_OBJECTS
    in_object = build.kernel_resources(build.OBJ_SKELETON)
    assert sorted(in_object) == sorted(KERNELS)                  # every kernel of the unit has a row, and no row is stale
    assert sorted(k for k in build.KERNEL_BUDGETS if k.startswith('k_sk_')) == sorted(KERNELS)
    res = build.check_kernel_budgets()
    for k in KERNELS:
        r = res[k]
        assert r['scratch'] == 0 and r['vgpr_spill'] == 0 and r['sgpr_spill'] == 0, (k, r)
        assert r['vgpr'] <= build.KERNEL_BUDGETS[k][0] <= 64 and r['lds'] <= build.KERNEL_BUDGETS[k][1] <= 2048, (k, r)      # eight waves per SIMD


def test_the_unit_is_new_and_its_core_is_hip_free():
    from ch_shrinkwrap_amd import build
    build.build_hip_library()
    core = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_skeleton_core.h')).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', core) == ['cmath', 'cstdint']                      # HIP-free, and nothing of the project's
    assert len(re.findall(r'NWA_HD\s+[\w ]+\bnwa_\w+\s*\(', core)) >= 12
    assert 'fma(' not in core and 'hip_runtime' not in core
    src = open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_skeleton.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert '"nw_skeleton_core.h"' in src and '"nw_bq.h"' in src
    for name in ('nwa_band(', 'nwa_face(', 'nwa_edge_range(', 'nwa_piece_face(', 'nwa_piece_terms(', 'nwa_arc_key(', 'atomicCAS(', 'atomicMin(', 'atomicAdd(',
                 'bq::scan_exclusive(', 'bq::scan_total('):
        assert name in code, name
    # no workgroup waits on another: no cooperative launch, no grid barrier, nothing sleeps
    for name in ('cooperative', 'grid_group', 'this_grid', 'sleep', '__threadfence'):
        assert name not in code, name
    for obj in build.BUDGETED_OBJECTS:
        names = build.kernel_resources(obj)
        if obj == build.OBJ_SKELETON:
            assert not [k for k in names if not k.startswith('k_sk_')]
        else:
            assert not [k for k in names if k.startswith('k_sk_')], obj
    for tree in ('include', 'ch_shrinkwrap_amd'):
        for d, _, files in os.walk(os.path.join(ROOT, tree)):
            for fn in files:
                if fn.endswith(('.h', '.hip', '.cpp', '.py')) and 'skeleton' not in fn:
                    assert not re.search(r'\bnwa_\w+', open(os.path.join(d, fn), errors='replace').read()), fn


def test_arguments_are_refused_before_any_hip_call():
    """No context exists without a GPU, and none is needed: every check of the mesh, the field and the band width that can be made without
    the context comes before its first use, and a refused call writes nothing."""
    from ch_shrinkwrap_amd import skeleton as C
    L = C.load()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    BAD = C.NWA_ERR_BADARG
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    twin = np.array([-1, 3, -1, 1, -1, -1], np.int32)
    quantum = np.full(4, 7.0)

    def m(P=pos, nv=4, F=faces, nf=2, T=twin, dev=0):
        return L.nwa_set_mesh(None, p(P), nv, p(F), nf, p(T), dev, p(quantum))
    assert m() == BAD                                                                                   # all is well but the context
    assert m(P=None) == BAD and m(F=None) == BAD and m(T=None) == BAD and m(nv=0) == BAD and m(nf=0) == BAD and m(dev=2) == BAD
    assert m(nv=(1 << 30) + 1) == BAD and m(nf=(1 << 30) + 1) == BAD
    for bad in (np.nan, np.inf, -np.inf):
        q = pos.copy()
        q[3, 1] = bad
        assert m(P=q) == C.NWA_ERR_NONFINITE
    for bad in (4, -1):
        f = faces.copy()
        f[1, 2] = bad
        assert m(F=f) == BAD
    for h, t in ((1, 4), (1, 6), (1, -2), (0, 0), (1, -1)):                                             # a twin table that is not mutual
        tw = twin.copy()
        tw[h] = t
        assert m(T=tw) == BAD
    assert (quantum == 7).all()

    field, info = np.array([0.0, 1.0, 2.0, np.inf]), np.full(C.NWA_INFO_WORDS, -7, np.int64)

    def s(D=field, dev=0, w=1.0, flags=0, inf=info):
        return L.nwa_skeleton(None, p(D), dev, float(w), flags, p(inf))
    assert s() == BAD and s(flags=C.NWA_FLAG_TIMING) == BAD                                             # all is well but the context
    assert s(D=None) == BAD and s(inf=None) == BAD and s(dev=2) == BAD and s(flags=2) == BAD
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        assert s(w=bad) == BAD
    assert (info == -7).all()                                                                           # nothing was written
    out = np.full(8, -7, np.int32)
    assert L.nwa_fetch(None, p(out), None, None, None, None, None) == BAD and (out == -7).all()
    h = ctypes.c_void_p()
    assert L.nwa_create(-1, ctypes.byref(h)) == BAD and L.nwa_create(0, None) == BAD
    assert L.nwa_last_error(None) == b'null ctx'
    # in the source: the host checks of a call stand before its first HIP call
    src = re.sub(r'//.*', '', open(os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc', 'nw_skeleton.hip')).read())
    body = src[src.index('NWA_EXPORT int nwa_skeleton('):src.index('NWA_EXPORT int nwa_fetch(')]
    assert body.index('nwa_width_ok(') < body.index('nwa_field_ok(') < body.index('hipSetDevice(')
    body = src[src.index('NWA_EXPORT int nwa_set_mesh('):src.index('NWA_EXPORT int nwa_skeleton(')]
    assert body.index('nwa_twins_ok(') < body.index('nwa_box(') < body.index('hipSetDevice(')


def test_there_is_no_host_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from ch_shrinkwrap_amd import skeleton as C
    from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
    v, f = icosphere(1, 10.0)
    z = v[:, 2].astype(np.float64) + 10.0
    with pytest.raises(RuntimeError):
        C.SkeletonContext()
    with pytest.raises(RuntimeError):
        C.level_set_skeleton((v, f), field=z, band_width=2.0)
    with pytest.raises(RuntimeError):
        C.level_set_skeleton((v, f))
    with pytest.raises(RuntimeError):
        C.level_set_skeleton((v, f), sources=[0])
    with pytest.raises(RuntimeError):
        TriMesh(v, f).skeleton()
    with pytest.raises(RuntimeError):
        C.SkeletonizeMembrane().execute({'membrane': TriMesh(v, f)})
    with pytest.raises(ValueError):
        C.level_set_skeleton((v, f), field=z, band_width=0.0)
    with pytest.raises(Exception):
        C.level_set_skeleton((v, np.concatenate([f, f[:1]])), field=z, band_width=2.0)                   # a non-manifold edge raises
    assert not [n for n in dir(C) if 'scipy' in n.lower() or n.endswith('_host') or n.endswith('_cpu')]
    src = open(C.__file__).read()
    assert 'import scipy' not in src and 'from scipy' not in src and 'connected_components' not in src


def _result(V, F, D, w):
    """what level_set_skeleton returns, made from the restatement: the host layer on top needs no GPU"""
    from ch_shrinkwrap_amd import skeleton as C
    r = R.level_sets(V, F, D, w)
    return dict(nodes=C.nodes_from_sums(r['node_sums'], r['node_band'], r['low'], r['q']), arcs=r['arcs'], vertex_node=r['vertex_node'],
                piece_start=r['piece_start'], piece_node=r['piece_node']), r


def test_signatures_docstrings_and_what_runs_on_the_host():
    from ch_shrinkwrap_amd import skeleton as C
    from ch_shrinkwrap_amd.trimesh import TriMesh
    assert list(inspect.signature(C.level_set_skeleton).parameters) == ['mesh', 'field', 'band_width', 'sources', 'context', 'device']
    sig = inspect.signature(C.level_set_skeleton).parameters
    assert sig['field'].default is None and sig['band_width'].default is None and sig['sources'].default is None and sig['context'].default is None
    assert list(inspect.signature(C.SkeletonContext.set_mesh).parameters) == ['self', 'vertices', 'faces', 'twin']
    assert list(inspect.signature(C.SkeletonContext.level_sets).parameters)[:3] == ['self', 'field', 'band_width']
    assert list(inspect.signature(C.skeleton_graph).parameters) == ['result', 'prune'] and inspect.signature(C.skeleton_graph).parameters['prune'].default == 0.0
    assert list(inspect.signature(TriMesh.skeleton).parameters)[:1] == ['self']
    for doc in (C.__doc__, C.level_set_skeleton.__doc__, C.SkeletonContext.level_sets.__doc__, C.SkeletonizeMembrane.__doc__, TriMesh.skeleton.__doc__):
        flat = re.sub(r'\s+', ' ', doc).lower()
        assert 'level-set diagram of one field' in flat and 'narrower than a band vanish' in flat, doc[:40]
    assert 'no exactness claim' in C.skeleton_graph.__doc__ and 'no exactness claim' in C.branch_of_vertex.__doc__
    assert 'NOT DETERMINISTIC' in C.SkeletonContext.level_sets.__doc__
    m = C.SkeletonizeMembrane()
    assert (m.input, m.output_nodes, m.output_branches, m.band_width, m.sources, m.prune) == ('membrane', 'skeleton_nodes', 'skeleton_branches', None, None, 0.0)
    assert C.SkeletonizeMembrane(prune=2.0).prune == 2.0
    with pytest.raises(AttributeError):
        C.SkeletonizeMembrane(band_widht=3.0)

    # nodes_from_sums is the restatement's arithmetic
    V, F = R.torus_mesh()
    res, r = _result(V, F, R.edge_dijkstra(V, F, 0), R.mean_edge(V, F))
    n = R.nodes(r)
    for k in ('position', 'perimeter', 'radius'):
        assert np.array_equal(res['nodes'][k], n[k], equal_nan=True)
    # a torus from one vertex: two ends are not there (the field's source and its antipode are single nodes of degree 2 or 1) and one loop
    g = C.skeleton_graph(res)
    assert g['n_loops'] == 1 == R.graph_numbers(r)[3] and g['n_components'] == 1 and g['kept'].all()
    assert (g['degree'] == R.degrees(r)).all() and g['n_branches'] == len(g['branches']) >= 1
    assert abs(g['total_length'] - sum(b['length'] for b in g['branches'])) < 1e-12
    covered = np.concatenate([np.stack([b['nodes'][:-1], b['nodes'][1:]], 1) for b in g['branches']])
    assert sorted(map(tuple, np.sort(covered, 1).tolist())) == sorted(map(tuple, r['arcs'].tolist()))     # every arc lies in exactly one branch
    bv = C.branch_of_vertex(res, g)
    assert bv.shape == (V.shape[0],) and bv.dtype == np.int32 and bv.max() < g['n_branches']

    # a tube is one branch between two ends, as long as the tube and of the ring's radius
    Vt, Ft = R.tube_mesh()
    res, r = _result(Vt, Ft, Vt[:, 2].astype(np.float64) + 0.011, 0.5)
    g = C.skeleton_graph(res)
    assert g['n_branches'] == 1 and g['ends'].size == 2 and g['junctions'].size == 0 and g['n_loops'] == 0
    b = g['branches'][0]
    assert 3.9 < b['length'] < 4.5 + 1e-9 and abs(b['mean_radius'] - 12 * np.sin(np.pi / 12) / np.pi) < 1e-4
    assert (C.branch_of_vertex(res, g) == 0).all()

    # pruning: a Y of three arms, one of them short, on a hand-made result
    pos = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [2, 0.3, 0], [4, 0, 0]], np.float64)
    hand = dict(nodes=dict(position=pos, radius=np.full(6, 0.5)), arcs=np.array([[0, 1], [1, 2], [2, 3], [2, 4], [3, 5]], np.int32),
                vertex_node=np.array([0, 4, 2, -1, 5], np.int32))
    g = C.skeleton_graph(hand)
    assert g['n_branches'] == 3 and g['junctions'].tolist() == [2] and sorted(g['ends'].tolist()) == [0, 4, 5] and g['n_loops'] == 0
    assert C.branch_of_vertex(hand, g)[[2, 3]].tolist() == [-1, -1]                                     # the junction's vertex and a dead one
    g = C.skeleton_graph(hand, prune=1.0)                                                                # the arm of length 0.3 < 1.0 x 0.5 goes
    assert g['n_branches'] == 1 and not g['kept'][4] and g['kept'].sum() == 5 and sorted(g['ends'].tolist()) == [0, 5] and g['n_loops'] == 0
    assert g['degree'].tolist() == [1, 2, 2, 2, -1, 1] and abs(g['branches'][0]['length'] - 4.0) < 1e-12
    assert C.branch_of_vertex(hand, g).tolist() == [0, -1, 0, -1, 0]
    ring = dict(nodes=dict(position=pos[:4], radius=np.zeros(4)), arcs=np.array([[0, 1], [1, 2], [2, 3], [0, 3]], np.int32), vertex_node=np.zeros(1, np.int32))
    g = C.skeleton_graph(ring)                                                                           # a cycle without a junction is one closed branch
    assert g['n_loops'] == 1 and g['n_branches'] == 1 and g['branches'][0]['ends'][0] == g['branches'][0]['ends'][1] and np.isnan(g['branches'][0]['mean_radius'])
