"""bench.py's output contract (one JSON line with the fields the driver and the judge read), on a scaled-down workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600, extra_env=None):
    env = dict(os.environ)
    env.update(extra_env or {})
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):           # the parent of an N-rank run is started plainly
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout, universal_newlines=True)
    return p


def test_help_parses_without_a_gpu():
    p = _run(['--help'], timeout=120)
    assert p.returncode == 0
    for flag in ('--gpus', '--steps', '--warmup', '--config', '--full', '--dump-outputs'):
        assert flag in p.stdout


def test_plain_python_with_gpus_2_starts_its_own_ranks_and_reports_their_failure():
    """`python bench.py --gpus N` as the driver invokes it (no torchrun): the parent starts N ranks of itself.  Without a GPU every rank
    refuses loudly (there is no CPU fallback) -- the parent must come back promptly with that failure, not hang and not pretend."""
    p = _run(['--gpus', '2', '--steps', '5', '--warmup', '5', '--scale', '0.05'], timeout=300)
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present: the ranks would run (covered by the gpu tests)')
    assert p.returncode != 0
    assert 'needs an MI355X' in p.stderr and 'rank' in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith('{')]


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize('mode', ['tiles', 'halo'])
def test_two_ranks_started_by_plain_python_print_one_json_line(mode):
    """The N > 1 entry point on hardware, as the driver runs it: `python3 bench.py --gpus 2 ...` starts its two ranks itself; on this
    one-GPU box they share cuda:0 and gloo carries the collectives (NW_BENCH_BACKEND=gloo; RCCL refuses duplicate devices).  Both
    decompositions: 'tiles' (one vesicle per rank, weak scaling) and 'halo' (ONE mesh sharded over the ranks, strong scaling)."""
    p = _run(['--gpus', '2', '--steps', '10', '--warmup', '5', '--scale', '0.05', '--mode', mode, '--full'], timeout=800, extra_env={'NW_BENCH_BACKEND': 'gloo'})
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    # (a sharded mesh gets new shares at layout time: one more untimed block for the library's own set-up on the new sub-mesh)
    assert j['n_gpus'] == 2 and j['steps'] == 10 and j['warmup'] == 5 and j['warmup_executed'] == 15
    assert j['scaling'] == ('strong' if mode == 'halo' else 'weak') and j['config']['mode'] == mode
    assert j['rccl']['backend'] == 'gloo' and j['rccl']['world_size_seen'] == 2 and len(j['rccl']['devices']) == 2
    c = j['collectives']
    assert c['per_iter'] == (4 if mode == 'halo' else 1) and 0 < c['share_of_device_time'] < 1       # 'halo': three neighbour exchanges + the sums
    assert j['value'] > 0 and j['roofline']['launches'] >= 2
    if mode == 'halo':
        h = j['halo']
        assert h['per_localization_halos'] and h['boundary_vertices'] > 0 and h['exchange'] == 'peers' and 7168 < h['exchange_bytes'] < 44 * h['boundary_vertices'] + 7168 and h['max_nn_distance_nm'] + h['drift_since_partition_nm'] <= h['margin_nm'] <= h['radius_nm']
        assert j['config']['vertices_per_gpu'] < j['config']['localizations_per_gpu']       # a share, not the whole mesh
        # one mesh: value counts its vertices once
        assert abs(j['value'] - float(j['config']['workload'].split(' vertices')[0].split(', ')[-1]) * 1e3 / j['ms_per_step']) <= 1e-6 * j['value']


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize('mode', ['tiles', 'halo'])
def test_rccl_path_replays_blocks_with_their_collectives(mode):
    """The N > 1 code path over RCCL itself, as far as one GPU allows: NW_BENCH_FORCE_DIST=1 runs bench.py's multi-rank branch with ONE
    nccl rank -- the library's own communicator (nw_comm_init), every block one nw_search call whose collectives are nodes of the block's
    hipGraph."""
    p = _run(['--gpus', '1', '--steps', '20', '--warmup', '10', '--scale', '0.05', '--mode', mode, '--full', '--no-cpu-baseline'], timeout=800, extra_env={'NW_BENCH_FORCE_DIST': '1'})
    assert p.returncode == 0, p.stderr[-3000:]
    j = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
    assert j['rccl']['backend'] == 'nccl' and j['rccl']['world_size_seen'] == 1 and j['rccl']['collectives_issued_by'].startswith('the library')
    assert j['collectives']['per_iter'] == (3 if mode == 'halo' else 1)
    assert j['config']['mode'] == mode and j['steps'] == 20


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize('mode,extra,env', [('tiles', [], {}), ('halo', [], {}), ('halo', ['--exchange', 'dense'], {}),
                                            ('tiles', ['--collectives', 'group'], {}), ('halo', [], {'NW_GRAPH_COMM': '0'})])
def test_two_ranks_over_rccl_when_two_gpus_are_visible(mode, extra, env):
    """The first thing a multi-GPU box should run (skipped on the one-GPU boxes this was built on): TWO ranks on TWO devices over RCCL --
    the library's communicator with its grouped ncclSend / ncclRecv of the owner-wise exchange and the all-reduces recorded into the
    block's hipGraph ('tiles', 'halo', 'halo' with the dense exchange), and the two fall-backs: the split-phase C-ABI over torch's process
    group (--collectives group) and multi-rank blocks launched one by one (NW_GRAPH_COMM=0)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs (RCCL refuses two ranks on one device)')
    p = _run(['--gpus', '2', '--steps', '10', '--warmup', '5', '--scale', '0.1', '--mode', mode, '--full', '--no-cpu-baseline'] + extra, timeout=800, extra_env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j['n_gpus'] == 2 and j['rccl']['backend'] == 'nccl' and j['rccl']['world_size_seen'] == 2
    assert len({d['device'] for d in j['rccl']['devices']}) == 2
    assert j['value'] > 0 and j['config']['mode'] == mode
    assert j['rccl']['collectives_issued_by'].startswith('the process group' if '--collectives' in extra else 'the library')


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_fall_backs_of_the_multi_rank_path_run_with_one_rank():
    """What a one-GPU box can check of the two fall-backs: ONE nccl rank through torch's process group with the split-phase
    C-ABI (--collectives group) and through the library's communicator with NW_GRAPH_COMM=0 (blocks launched one by one, never recorded)."""
    for extra, env in ((['--collectives', 'group'], {}), ([], {'NW_GRAPH_COMM': '0'})):
        e = dict(env, NW_BENCH_FORCE_DIST='1')
        p = _run(['--gpus', '1', '--steps', '10', '--warmup', '5', '--scale', '0.05', '--mode', 'tiles', '--full', '--no-cpu-baseline'] + extra, timeout=800, extra_env=e)
        assert p.returncode == 0, p.stderr[-3000:]
        j = json.loads([l for l in p.stdout.splitlines() if l.startswith('{')][0])
        assert j['rccl']['backend'] == 'nccl' and j['steps'] == 10 and j['value'] > 0
        assert j['rccl']['collectives_issued_by'].startswith('the process group' if extra else 'the library')


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_two_ranks_started_by_the_drivers_launcher_print_one_json_line():
    """The driver's own command for N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N --steps K --warmup W` (RANK / LOCAL_RANK / WORLD_SIZE come from the launcher; bench.py must not start
    ranks of its own).  Two gloo ranks sharing cuda:0 here (NW_BENCH_BACKEND=gloo: RCCL refuses duplicate devices)."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env['NW_BENCH_BACKEND'] = 'gloo'
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1', '--master-port', str(port),
                        os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '10', '--warmup', '5', '--scale', '0.05', '--full'],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=800, universal_newlines=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]                          # rank 0 only
    j = json.loads(lines[0])
    assert j['n_gpus'] == 2 and j['steps'] == 10 and j['scaling'] == 'weak' and j['config']['mode'] == 'tiles'
    assert j['rccl']['world_size_seen'] == 2 and j['value'] > 0 and 'roofline' in j


@pytest.mark.gpu
def test_one_json_line_with_roofline_and_cpu_baseline():
    p = _run(['--gpus', '1', '--steps', '10', '--warmup', '5', '--scale', '0.05', '--full', '--cpu-iters', '2'])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j['n_gpus'] == 1 and j['steps'] == 10 and j['warmup'] == 5 and j['warmup_executed'] == 15      # (W, then two untimed blocks behind the one-off set-up)
    assert j['unit'] == 'vertex-updates/s' and j['higher_is_better'] is True and j['scaling'] == 'weak'
    assert j['data'] == 'synthetic' and j['dtype'] == 'f32' and j['vs_baseline'] is None
    assert 'SCALED' in j['config']['workload']                      # a debug-sized run says so
    # value = valid vertices x steps / time
    assert abs(j['value'] - j['config']['vertices_per_gpu'] * 1e3 / j['ms_per_step']) <= 1e-6 * j['value']
    r = j['roofline']
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] == 'GB/s' and r['peak'] == 8000.0
    assert r['launches'] == 2 and r['avg_launch_ms'] > 0           # one live sample per block of 5 of the timed region
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-12
    c = j['cpu_baseline']
    assert c['kind'] == 'port' and c['value'] > 0 and c['cores'] >= 1 and c['unit'] == j['unit']
    assert j['value'] > c['value']


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline fields only; --dump-outputs writes the positions the
    last timed block returned, and a second run with the same arguments writes the same array (seeded inputs, deterministic fit)."""
    got = []
    for k in range(2):
        d = str(tmp_path / ('run%d' % k))
        p = _run(['--gpus', '1', '--steps', '7', '--warmup', '5', '--scale', '0.05', '--dump-outputs', d])
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, p.stdout[-2000:]
        j = json.loads(lines[0])
        assert j['steps'] == 7 and j['warmup'] == 5 and j['unit'] == 'vertex-updates/s' and j['higher_is_better'] is True and j['dtype'] == 'f32'
        assert abs(j['value'] - j['config']['vertices_per_gpu'] * 1e3 / j['ms_per_step']) <= 1e-6 * j['value']
        assert not {'roofline', 'stage_ms_per_iter', 'cpu_baseline', 'ms_per_step_graph_replay'} & set(j)
        a = np.load(os.path.join(d, 'positions.npy'))
        assert a.dtype == np.float32 and a.shape == (j['config']['vertices_per_gpu'], 3) and np.isfinite(a).all()
        got.append(a)
    assert np.array_equal(got[0], got[1])
