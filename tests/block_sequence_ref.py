"""
TEST INFRASTRUCTURE -- one driver for a scripted sequence of blocks on ONE live fit context, and the table of sequences that
tests/test_hip_block_transitions.py (GPU) and tests/test_block_sequence_ref.py (CPU) run.

A sequence is a list of steps.  A step is a dict:

    pre     list of (name, argument) pairs: what the caller does before the block, in order
              ('new_cg', dict(mesh=NAME, reuse=BOOL))   a new optimiser on the shared native context (membrane_mesh.py's block loop)
              ('points', NAME)                          cg.points = another cloud
              ('edit_positions', FACTOR)                host positions scaled in place + update_geometry (test_host_edit_between_two_fits...)
              ('refresh_normals', None)                 cg.refresh_normals()
              ('optimize_layout', None)                 transport only
              ('separate_attraction', BOOL)             transport only
              ('quantum', FACTOR or None)               nw_accumulator_quantum: override = local quantum * FACTOR / dropped (no oracle parameter)
              ('raise_status', NAME)                    nw_debug(what = 8): the next block starts with that status in its device state
                                                        (NAME in STATUS_CODES; a plain integer is passed on as it is, 0 disarms)
    search  the block's search() arguments; arrays by NAME in the scene (the same object every time, as a caller that keeps its arrays):
              lams, num_iters, sigma_inv, weights, data, pos, last_step, to_host, regulariser ('I' / 'wfunc': cg.Lfuncs, cg.Lhfuncs)
    raises  the block ends in that status: 'nan' (NW_ERR_NAN, AssertionError), 'singular' (NW_ERR_SINGULAR, LinAlgError), 'internal',
            'handoff' (NanoWrapError with that code); the mesh stays at the last good iterate
    stated  the GPU test states how many recordings the block makes at level 0 (see build())

run_device(steps, level) plays them through ShrinkwrapMeshConjGrad on one NativeContext (level 0: blocks as hipGraphs; 1: every launch
from the host; 4: head graph + live last iteration); run_oracle(steps) through oracle.nanowrap_oracle.search block after block (positions
carried over, block-stale normals, the `tests` history carried or reset).  No GPU import at module level.
"""
import ctypes
import time
import numpy as np

BASE = dict(lams=[10.0], num_iters=3, sigma_inv='s6', weights=None, data=None, pos=False, last_step=True, to_host=True, regulariser='I')
OPENING = 5          # identical blocks every sequence opens with: the first four of a context differ in structure on purpose (cold query,
                     # projection re-sort + k-d list, tune_grid, order_items_by_cost); from the fifth on a replay of a cached graph is the normal case


# ---- the scene ---------------------------------------------------------------------------------------------------------------
class Scene(object):
    """icosphere(3, 120) (642 vertices, 1280 faces) + sphere_cloud(6000, 100, 8, seed=9): the smallest scene at which all ten launches of
    an iteration are real; a second cloud of 9000 (on a sphere of radius 90: going there and back leaves a trace), a second mesh of 162 vertices, the first mesh with two spare vertex slots; and the
    small well-posed sphere on which the stop condition fires (test_stop_condition_fires_on_the_device, on this scene's second mesh)."""

    def __init__(self):
        self._a = {}

    def mesh(self, name):
        from ch_shrinkwrap_amd.trimesh import TriMesh, icosphere
        v, f = icosphere(2 if name == 'm2' else 3, 120.0)
        return TriMesh(v, f, max_vertices=v.shape[0] + 2) if name == 'm3s' else TriMesh(v, f)

    def get(self, name):
        if name is None or not isinstance(name, str):
            return name
        if name not in self._a:
            self._a[name] = self._make(name)
            self._a[name].setflags(write=False)
        return self._a[name]

    def _make(self, name):
        from ch_shrinkwrap_amd.synth import sphere_cloud
        rng = np.random.default_rng(77)
        if name == 'p6':
            return sphere_cloud(6000, 100.0, 8.0, seed=9)
        if name == 'p9':
            return sphere_cloud(9000, 90.0, 8.0, seed=10)
        if name == 'p4':
            return sphere_cloud(4000, 100.0, 2.0, seed=3)
        if name == 's6':
            return 1.0 / np.full(3 * 6000, 8.0, 'f4')
        if name == 's9':
            return 1.0 / np.full(3 * 9000, 8.0, 'f4')
        if name == 's4':
            return 1.0 / np.full(3 * 4000, 2.0, 'f4')
        if name == 's6b':          # per-localization precisions between 4 and 16 nm
            return (1.0 / np.repeat(rng.uniform(4.0, 16.0, 6000), 3)).astype('f4')
        if name == 's6c':          # the same buffer sizes, other values
            return (1.0 / np.repeat(rng.uniform(4.0, 16.0, 6000)[::-1] * 0.5, 3)).astype('f4')
        if name == 'w6mask':       # weights with zeros: a mask that drops a quarter of the localizations (one octant and a bit)
            p = self.get('p6')
            keep = ~((p[:, 0] > 0) & (p[:, 1] > 0)) | (p[:, 2] < 0)
            return (np.repeat(keep, 3) * np.repeat(rng.uniform(0.05, 0.25, 6000), 3)).astype('f4')
        if name == 'd6':           # another residual target of equal shape: the cloud pulled towards a sphere of radius 80
            return (self.get('p6') * np.float32(0.8)).astype('f4')
        if name == 's6nan':
            s = self.get('s6').copy()
            s[3 * 1234 + 1] = np.nan
            return s
        raise KeyError(name)


_scene = None


def scene():
    global _scene
    if _scene is None:
        _scene = Scene()
    return _scene


# ---- the sequences -----------------------------------------------------------------------------------------------------------
def _step(state, pre=(), raises=None, stated=False):
    return dict(pre=list(pre), search=dict(state), raises=raises, stated=stated)


def build(changes, base=None, after=OPENING, tail=2, steady=False):
    """`after` identical blocks, one block per change (a dict: 'pre', 'raises', 'stated' and search-argument overrides, which stay for
    the blocks that follow), then `tail` more blocks identical to the last: the first of them uses the other half of the result's
    staging buffer, the second is the first block that can replay a graph recorded for the changed shape.  Returns (steps, control):
    control = the same number of blocks with no change at all.

    `stated`: the test states how many recordings the block makes at level 0 (tests/test_hip_block_transitions.py restates the ring of
    recorded graphs and what block_graph_key() holds).  The opening blocks of a full opening are stated, a change where it says so, and
    with `steady` everything after the opening: the change does not move the surface enough for the cell-size rule to lay a new grid."""
    state = dict(BASE)
    state.update(base or {})
    first = dict(state)
    steps = [_step(state, stated=after >= OPENING) for i in range(after)]
    for ch in changes:
        ch = dict(ch)
        pre, raises, stated = ch.pop('pre', ()), ch.pop('raises', None), ch.pop('stated', False)
        state.update(ch)
        steps.append(_step(state, pre, raises, (stated or steady) and after >= OPENING))
    steps += [_step(state, stated=steady and after >= OPENING) for _ in range(tail)]
    control = [_step(first) for _ in steps]
    return steps, control


class Case(object):
    """changes: see build().  kind: 'value' (the block after the change must differ from the control's) or 'transport' (every block
    equals the control's, bit for bit).  anchor: the oracle has a parameter for the change, and the change moves the oracle's final
    positions by at least ten times the anchor's bound (tests/test_block_sequence_ref.py checks that on the CPU); None: the oracle is
    compared, no margin applies (transport only, or no oracle parameter); False: dropped from the anchor, `why` says why.  early: also run
    with the change made after block 1, while the layout is still changing (nothing stated about recordings there).  steady: see build()."""

    def __init__(self, name, changes, kind='value', anchor=True, early=False, base=None, why='', steady=False):
        self.name, self.changes, self.kind, self.anchor, self.early, self.base, self.why, self.steady = name, changes, kind, anchor, early, base, why, steady

    def steps(self, early=False):
        return build(self.changes, self.base, after=1 if early else OPENING, steady=self.steady)


def new_cg(mesh='m3', reuse=True):
    return ('new_cg', dict(mesh=mesh, reuse=reuse))


# stated=True on a change: its block makes exactly one recording whatever else happens (a by-value argument or pointer of the key is new).
# Nothing is stated after a change that moves the surface (the cell-size rule may lay a new grid: another generation, another key) or
# uploads something (the structural blocks start again: re-sort, tuner, cost order).
CASES = [
    Case('lams_10_to_2', [dict(lams=[2.0], stated=True)], early=True),
    Case('second_lambda_appended', [dict(lams=[10.0, 3.0])], kind='transport', anchor=None, steady=True),
    Case('num_iters_3_5_3_1', [dict(num_iters=5), dict(num_iters=3), dict(num_iters=1)], early=True, steady=True),
    Case('pos_on', [dict(pos=True, stated=True)]),
    Case('last_step_off', [dict(last_step=False)], anchor=False, steady=True,
         why='dropping the third search direction moves the oracle by less than the anchor\'s bound (5e-6 of the bbox diagonal)'),
    Case('wfunc_and_back', [dict(regulariser='wfunc', stated=True), dict(regulariser='I')]),
    Case('sigma_inv_scalar_scalar_array_array', [dict(sigma_inv=0.05), dict(sigma_inv='s6b'), dict(sigma_inv='s6c')], base=dict(sigma_inv=0.125), early=True),
    Case('weights_none_scalar_mask_none', [dict(weights=0.05), dict(weights='w6mask'), dict(weights=None)]),
    Case('data_other_then_points', [dict(data='d6', stated=True), dict(data=None)]),
    Case('accumulator_quantum_set_then_dropped', [dict(pre=[('quantum', 65536.0)]), dict(pre=[('quantum', None)])], anchor=None, steady=True,
         why='no oracle parameter (the quantum is the fixed-point scale of exact sums): the oracle is compared, no margin applies'),
    Case('points_9000_then_6000', [dict(pre=[('points', 'p9')], sigma_inv='s9'), dict(pre=[('points', 'p6')], sigma_inv='s6')], early=True),
    Case('new_optimiser_reset_history_only', [dict(pre=[new_cg('m3', True)])], kind='transport', anchor=None, steady=True),
    Case('new_optimiser_162_then_642_vertices', [dict(pre=[new_cg('m2', True)]), dict(pre=[new_cg('m3', True)])]),
    Case('mesh_with_spare_slots', [dict(pre=[new_cg('m3s', True)])]),
    Case('host_edit_then_fresh_optimiser', [dict(pre=[('edit_positions', 1.1), new_cg('m3', False)])]),
    Case('refresh_normals', [dict(pre=[('refresh_normals', None)])], anchor=False, steady=True,
         why='fresh normals move the oracle by less than ten times the anchor\'s bound (7e-4 of the bbox diagonal)'),
    Case('optimize_layout', [dict(pre=[('optimize_layout', None)])], kind='transport', anchor=None, steady=True),
    Case('separate_attraction_on_off', [dict(pre=[('separate_attraction', True)]), dict(pre=[('separate_attraction', False)])],
         kind='transport', anchor=None, steady=True),
    Case('to_host_off_on', [dict(to_host=False), dict(to_host=True)], kind='transport', anchor=None, steady=True),
]

# a stop that fires on the device inside a block, then nw_reset_history and a block that must run all three iterations: the small
# well-posed sphere of test_stop_condition_fires_on_the_device on this scene's second mesh
STOP_BASE = dict(sigma_inv='s4')
STOP_LONG = 400


def stop_case():
    steps = [_step(dict(BASE, **STOP_BASE)) for _ in range(OPENING)]
    steps.append(_step(dict(BASE, num_iters=STOP_LONG, **STOP_BASE)))
    steps.append(_step(dict(BASE, **STOP_BASE), pre=[new_cg('m2', True)]))
    return steps


def nan_case():
    """a block that ends in NW_ERR_NAN (test_nan_inside_an_iteration...: one non-finite sigma_inv entry), then the same block repaired"""
    steps, _ = build([dict(sigma_inv='s6nan', raises='nan'), dict(sigma_inv='s6')])
    return steps


STATUS_CODES = dict(nan=-3, singular=-4, internal=-7, handoff=-9)          # the statuses a kernel of a single-rank block can raise (include/nanowrap.h)
STATUS_TAIL = 3


def status_case(name, early=False):
    """OPENING identical blocks (1 with `early`), a block that starts with the status `name` armed in its device state (nw_debug(what = 8):
    the path of a status raised in the first iteration's attraction step), then three more blocks identical to the opening.  Returns
    (steps, control): control = as many blocks with nothing armed.  The armed block's index is OPENING, or 1 with `early`."""
    assert name in STATUS_CODES
    return build([dict(pre=[('raise_status', name)], raises=name)], after=1 if early else OPENING, tail=STATUS_TAIL)


EVICTION_REVISITS = 3


def eviction_case():
    """ten distinct block shapes in a row (num_iters 2..6 x pos on / off), then the first three again, three times over: the 8-slot
    ring has evicted them and records them again on the first visit; the second visit falls on the other half of the staging buffer
    (another pointer in the key: recorded too); the third is the second visit with the same half and replays what the first recorded"""
    shapes = [(n, p) for p in (True, False) for n in (2, 3, 4, 5, 6)]
    steps = [_step(BASE) for _ in range(OPENING)]
    for n, p in shapes + shapes[:3] * EVICTION_REVISITS:
        steps.append(_step(dict(BASE, num_iters=n, pos=p)))
    return steps, len(shapes)


# ---- the device --------------------------------------------------------------------------------------------------------------
def _tail(seq, n):
    return np.array(seq[len(seq) - n:] if n else [], 'f4')


def status_words(nat, code=0):
    """nw_debug(what = 8) with `code`: (its return value, the code that was armed before the call, handoff_off)"""
    out = (ctypes.c_int64 * 2)()
    rc = nat.L.nw_debug(nat.h, 8, out, None, int(code), None)
    return rc, int(out[0]), int(out[1])


def run_device(steps, level, mesh0='m3', points0='p6', handoff_retries=1):
    """One NativeContext, one TriMesh per mesh name.  Returns (blocks, stats): per block a dict of positions (None with to_host=False),
    mesh_positions, nearest_face, S, res, tests / ress (this block's entries), loopcount, error (None or the name of the status the block
    ended in) and message (the exception's text), seconds (of search()) and graph_stats() before the block's
    pre-steps / after the block; armed = what every 'raise_status' step of the block returned (status_words), status_before /
    status_info = (the code armed, handoff_off) just before the block's search() and after it; stats = graph_stats() after the sequence.
    handoff_retries: ShrinkwrapMeshConjGrad.handoff_retries of every optimiser (0: NW_ERR_HANDOFF reaches the caller)."""
    from ch_shrinkwrap_amd.mesh_conj_grad import ShrinkwrapMeshConjGrad, NativeContext
    from ch_shrinkwrap_amd._lib import NanoWrapError
    sc = scene()
    nat = NativeContext(0)
    meshes = {}
    names = {v: k for k, v in STATUS_CODES.items()}

    def mesh_of(name):
        if name not in meshes:
            meshes[name] = sc.mesh(name)
        return meshes[name]

    def make(mesh_name, reuse, points):
        cg = ShrinkwrapMeshConjGrad(mesh_of(mesh_name), points, native=nat, reuse_device_mesh=reuse)
        cg.set_profiling(level)
        cg.handoff_retries = handoff_retries
        return cg

    cg = make(mesh0, False, sc.get(points0))
    blocks = []
    for st in steps:
        before = cg.graph_stats()
        armed = []
        for what, arg in st['pre']:
            if what == 'new_cg':
                cg = make(arg['mesh'], arg['reuse'], cg.points)
            elif what == 'points':
                cg.points = sc.get(arg)
            elif what == 'edit_positions':
                m = cg.mesh
                m._vertices['position'][:] = (m._vertices['position'] * arg).astype('f4')
                m.update_geometry()
            elif what == 'refresh_normals':
                cg.refresh_normals()
            elif what == 'optimize_layout':
                cg.optimize_layout()
            elif what == 'separate_attraction':
                cg.separate_attraction(arg)
            elif what == 'quantum':
                q = ctypes.c_double(0.0)
                nat.check(nat.L.nw_accumulator_quantum(nat.h, ctypes.byref(q)))
                q = ctypes.c_double(q.value * arg if arg else -1.0)
                nat.check(nat.L.nw_accumulator_quantum(nat.h, ctypes.byref(q)))
            elif what == 'raise_status':
                armed.append(status_words(nat, STATUS_CODES.get(arg, arg)))          # (not checked: a refusal is something a test looks at)
            else:
                raise ValueError(what)
        _, code_armed, off = status_words(nat, 0)          # the getter disarms: what it found is armed again
        if code_armed:
            status_words(nat, code_armed)
        status_before = (code_armed, off)
        a = st['search']
        cg.Lfuncs, cg.Lhfuncs = [a['regulariser']], [a['regulariser']]
        data = cg.points if a['data'] is None else sc.get(a['data'])
        n_before, error, message, out = len(cg.tests), None, None, None
        t0 = time.perf_counter()
        try:
            out = cg.search(data, lams=a['lams'], num_iters=a['num_iters'], weights=sc.get(a['weights']), sigma_inv=sc.get(a['sigma_inv']),
                            pos=a['pos'], last_step=a['last_step'], to_host=a['to_host'])
        except AssertionError as e:
            error, message = 'nan', str(e)
        except np.linalg.LinAlgError as e:
            error, message = 'singular', str(e)
        except NanoWrapError as e:
            if e.code not in (STATUS_CODES['internal'], STATUS_CODES['handoff']):
                raise
            error, message = names[e.code], str(e)
        seconds = time.perf_counter() - t0
        n = len(cg.tests) - n_before
        b = dict(seconds=seconds, error=error, message=message, loopcount=None if error else cg.loopcount, positions=None if out is None else out.copy(),
                 mesh_positions=cg.mesh.vertices.copy(), tests=_tail(cg.tests, n), ress=_tail(cg.ress, n), before=before, after=cg.graph_stats(),
                 armed=armed, status_before=status_before, status_info=status_words(nat, 0)[1:])
        if error is None:
            b.update(nearest_face=cg.nearest_face.copy(), S=cg.S.copy(), res=cg.res.copy())
        blocks.append(b)
    stats = cg.graph_stats()
    cg.synchronize()
    nat.close()
    return blocks, stats


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def run_oracle(steps, mesh0='m3', points0='p6', brute_nn=None):
    """The same steps through oracle.nanowrap_oracle.search.  What the device keeps between blocks is kept here by hand: the mesh
    positions (valid rows of the last iterate), the normals the device holds (block-stale: as uploaded, or as last refreshed), the
    normals in the host records (what a fresh optimiser uploads), and the `tests` history of the optimiser object.
    brute_nn: the oracle's exhaustive float64 nearest-centroid search, which gives an exact tie to the lowest face id as the device does;
    None = in the blocks that run with positivity on or after it (it folds an octant of faces onto one point; among such ties the k-d
    tree's choice is arbitrary: the two searches end 5e-3 of the bbox diagonal apart on `pos_on`, the device with the exhaustive one)."""
    from oracle import nanowrap_oracle as O
    sc = scene()
    meshes, host_nrm = {}, {}

    def mesh_of(name):
        if name not in meshes:
            meshes[name] = sc.mesh(name)
            host_nrm[name] = meshes[name].vertex_normals.copy()
        return meshes[name]

    def normals_of(m):
        m.update_geometry()
        return m.vertex_normals.copy()

    cur = mesh0
    mesh_of(cur)
    nrm_dev = host_nrm[cur].copy()
    points = sc.get(points0)
    tests = []
    blocks = []
    folded = False
    for st in steps:
        for what, arg in st['pre']:
            if what == 'new_cg':
                same = arg['reuse'] and arg['mesh'] == cur
                cur = arg['mesh']
                mesh_of(cur)
                if not same:
                    nrm_dev = host_nrm[cur].copy()          # uploaded with the mesh
                tests = []
            elif what == 'points':
                points = sc.get(arg)
            elif what == 'edit_positions':
                m = meshes[cur]
                m._vertices['position'][:] = (m._vertices['position'] * arg).astype('f4')
                host_nrm[cur] = normals_of(m)
            elif what == 'refresh_normals':
                nrm_dev = normals_of(meshes[cur])
                host_nrm[cur] = nrm_dev.copy()
            elif what in ('optimize_layout', 'separate_attraction', 'quantum', 'raise_status'):
                pass                                        # transport only / no parameter / see below
            else:
                raise ValueError(what)
        a = st['search']
        m = meshes[cur]
        n_before = len(tests)
        b = dict(error=None)
        folded = folded or a['pos']
        if st['raises'] and any(what == 'raise_status' for what, _ in st['pre']):
            # a status armed on the device with inputs that are in order: the reference has nothing to raise it from.  It raises before
            # `self.f[:] = fnew` (mesh_conj_grad.py:514,548,580 vs :288), so the step is left out: positions and history carry over
            b.update(error=st['raises'], loopcount=None, positions=None, tests=np.zeros(0), ress=np.zeros(0), mesh_positions=m.vertices.copy())
            blocks.append(b)
            continue
        try:
            r = O.search(m.vertices.copy(), nrm_dev.copy(), m.neighbor_vertex_table(), m.faces, points, list(a['lams']), a['num_iters'],
                         sc.get(a['sigma_inv']), weights=sc.get(a['weights']), valid=m.valid_vertex_mask(), pos_constraint=a['pos'],
                         last_step=a['last_step'], tests=tests, regulariser=a['regulariser'], data=sc.get(a['data']), brute_nn=folded if brute_nn is None else brute_nn,
                         workers=1)          # (a few thousand queries of a few hundred centroids: a thread pool per query costs more than it saves)
            m._vertices['position'][:] = r.mesh_positions
            b.update(loopcount=r.loopcount, positions=r.positions.copy(), tests=np.array(tests[n_before:], 'f8'), ress=np.array(r.ress, 'f8'))
        except AssertionError:
            del tests[n_before:]                            # (the optimiser's log of the failed block is not taken either)
            b.update(error='nan', loopcount=None, positions=None, tests=np.zeros(0), ress=np.zeros(0))
        b['mesh_positions'] = m.vertices.copy()
        blocks.append(b)
    return blocks


def rel_rms(a, b):
    """vertex RMS difference relative to the bounding-box diagonal of `b` (conftest.rel_rms)"""
    a, b = np.asarray(a, 'f8').reshape(-1, 3), np.asarray(b, 'f8').reshape(-1, 3)
    return float(np.sqrt(((a - b) ** 2).sum(1).mean()) / np.linalg.norm(b.max(0) - b.min(0)))
