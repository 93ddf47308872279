"""
What the host driver of the device remesher decides, without a GPU: ch_shrinkwrap_amd/csrc/nw_remesh_plan.h holds the room of an attempt and
the retry schedule, the rule that ends a pass, the rules that end the split sweeps and the iterations, and the Morton cube of the input.
This test writes a stand-alone program around the header, builds it with g++ twice (plain, -fsanitize=address,undefined) and runs each
build as a child process.  The program reads a list of questions, one per line, and prints one answer line each; the expected answers come
from tests/remesh_device_ref.py (the rules it shares with the driver) or are worked out here (capacities, retry schedule).

The rule that ends a pass is asked the way the driver asks it: before round r the host has waited for the report of round r - 2 and sees
of the later ones what happens to be in.  A question gives the bidders of every round and, per round j, the decision at which its report
is in: j + 1 (in when first asked for) or j + 2 (the latest the wait allows).
"""
import os
import re
import subprocess

import numpy as np
import pytest

import remesh_device_ref as ref
from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')
HEADER = os.path.join(CSRC, 'nw_remesh_plan.h')
CXX = os.environ.get('CXX', 'g++')
BUILDS = {'plain': [], 'address_undefined': ['-fsanitize=address,undefined']}
ROUNDS_CAP = 4096

PROGRAM = r'''
#include "nw_remesh_plan.h"
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace rm_plan;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    for (int idx = 0; std::getline(in, line); ++idx) {
        std::istringstream ls(line);
        std::string what;
        ls >> what;
        printf("answer %d", idx);
        if (what == "pass") {
            // the driver's loop: wait for the report of the round before last, ask, launch
            int kind; unsigned first;
            ls >> kind >> first;
            std::vector<int> bids(R_MAX[kind]), seen_at(R_MAX[kind]), reports(R_MAX[kind]);
            for (int &b : bids) ls >> b;
            for (int &a : seen_at) ls >> a;
            int launched = 0;
            for (int r = 0; r < R_MAX[kind]; ++r) {
                for (int j = 0; j < r; ++j) reports[j] = seen_at[j] <= r ? bids[j] : -1;
                if (r >= RUN_AHEAD && reports[r - RUN_AHEAD] < 0) { fprintf(stderr, "line %d: the report the host waits for is not in\n", idx); return 2; }
                if (!launches_round(reports.data(), r, first)) break;
                ++launched;
            }
            printf(" %d", launched);
        } else if (what == "cap") {
            std::string pieces_s, room_s; long long nv, nf;                 // (strtod reads inf and nan; operator>> need not)
            ls >> pieces_s >> nv >> nf >> room_s;
            const double pieces = strtod(pieces_s.c_str(), nullptr), room = strtod(room_s.c_str(), nullptr);
            Capacity c = {0, 0, 0, 0};
            const Fit fit = capacities(pieces, nv, nf, room, &c);
            printf(" %d %llu %llu %llu %llu", (int)fit, (unsigned long long)c.Fcap, (unsigned long long)c.Vcap, (unsigned long long)c.Hcap, (unsigned long long)c.list);
        } else if (what == "sweep") {
            int n_list, first_list;
            ls >> n_list >> first_list;
            printf(" %d", (int)sweeps_end(n_list, first_list));
        } else if (what == "iter") {
            int n_relax, before[3], now[3];
            ls >> n_relax >> before[0] >> before[1] >> before[2] >> now[0] >> now[1] >> now[2];
            printf(" %d", (int)iterations_end(n_relax, before, now));
        } else if (what == "retry") {
            std::string env;
            ls >> env;
            double room = first_room(env == "-" ? nullptr : env.c_str());
            for (int t = 0; t < TRIES; ++t, room = next_room(room)) printf(" %.17g", room);
        } else if (what == "cube") {
            std::string path; long long nv;
            ls >> path >> nv;
            std::vector<float> v(3 * nv);
            FILE *fh = fopen(path.c_str(), "rb");
            if (!fh || fread(v.data(), 4, v.size(), fh) != v.size()) return 2;
            fclose(fh);
            const Cube c = morton_cube(v.data(), nv);
            printf(" %.17g %.17g %.17g %.17g", c.lo[0], c.lo[1], c.lo[2], c.per_unit);
        } else if (what == "constants") {
            printf(" %d %d %d %d %d %d %d %u", R_MAX[0], R_MAX[1], R_MAX[2], (int)ROUNDS_CAP, (int)SPLIT_SWEEPS, (int)TRIES, (int)RUN_AHEAD, round_seed(7u, 5));
        } else if (what == "lengths") {
            double L;
            ls >> L;
            printf(" %.17g %.17g", edge_high(L), edge_low(L));
        } else if (what == "valence") {
            int v;
            ls >> v;
            printf(" %d", effective_max_valence(v));
        } else {
            return 2;
        }
        if (!ls) { fprintf(stderr, "bad line %d\n", idx); return 2; }
        printf("\n");
    }
    return 0;
}
'''


# ---- the questions -------------------------------------------------------------------------------------------------------------------------
def ref_rounds(kind, bids):
    """the rounds the restatement runs in a pass whose round j has bids[j] bidders"""
    n = 0
    for r in range(ref.R_MAX[kind]):
        if not ref.pass_goes_on(list(bids[:r]), r):
            break
        n += 1
    return n


def _padded(kind, head, tail):
    return (list(head) + [tail] * 64)[:ref.R_MAX[kind]]


def _random_bids(rng, kind):
    """a pass that thins out: counts that fall by a random factor from a random start, so that the `< 8` and `500 x` rules, an empty round
    and a tail that lasts to R_MAX all occur"""
    b = [int(rng.choice([1, 3, 9, 40, 3400, 3500, 3600, 4000, 4100, 100000]))]
    floor = int(rng.choice([0, 0, 1, 5, 6, 7, 8, 9]))
    while len(b) < ref.R_MAX[kind]:
        b.append(max(floor if rng.random() < 0.9 else 0, int(b[-1] * rng.choice([0.02, 0.2, 0.5, 0.9]))))
    return b


def _on_time(kind):
    """every report of a pass of this kind is in when it is first asked for: that of round j at the decision about round j + 1"""
    return [j + 1 for j in range(ref.R_MAX[kind])]


PASSES = []           # (kind, first, bids, seen_at)
for kind in range(3):
    hand = [_padded(kind, [0], 0),                            # a first round of 0
            _padded(kind, [5, 0], 0),
            _padded(kind, [4000, 100, 8], 8),                 # 8 is not `< 8`: never dries up, ends at R_MAX
            _padded(kind, [4000, 100, 7], 7),                 # 7 * 500 < 4000: so few
            _padded(kind, [3500, 100, 7], 7),                 # 7 * 500 = 3500: not fewer
            _padded(kind, [3501, 100, 7], 7),
            _padded(kind, [3500, 100, 7, 6], 6),              # 6 * 500 < 3500
            _padded(kind, [3000, 6, 6], 6),                   # ... at 3000 it is not
            _padded(kind, [7, 7, 7], 7),                      # (a small pass: nothing is a five-hundredth of its first round)
            _padded(kind, [100000, 1], 100),                  # a round of so few with fuller ones behind it
            _padded(kind, [100], 100)]                        # a tail that never dries up
    for bids in hand:
        PASSES.append((kind, 1, bids, _on_time(kind)))
    for first in (ROUNDS_CAP - 3, ROUNDS_CAP - 2, ROUNDS_CAP - 1, ROUNDS_CAP):
        PASSES.append((kind, first, _padded(kind, [100], 100), _on_time(kind)))          # a pass that starts close to ROUNDS_CAP
        PASSES.append((kind, first, _padded(kind, [100, 0], 0), _on_time(kind)))
    rng = np.random.default_rng(20 + kind)
    for _ in range(500):
        bids = _random_bids(rng, kind)
        PASSES.append((kind, int(rng.integers(1, 3000)), bids, _on_time(kind)))
N_ON_TIME = len(PASSES)
# late reports.  By hand: an empty round whose report comes as late as the wait allows costs one more round
PASSES.append((0, 1, _padded(0, [100, 0], 0), [1, 3] + [j + 1 for j in range(2, 24)]))
LATE_EMPTY = len(PASSES) - 1
for kind in range(3):
    rng = np.random.default_rng(40 + kind)
    for _ in range(1500):
        bids = _random_bids(rng, kind)
        PASSES.append((kind, int(rng.integers(1, 3000)), bids, [j + 1 + int(rng.integers(0, 2)) for j in range(len(bids))]))

ROOMS = (0.05, 0.3, 1.5, 3.0, 192.0)
NAN = float('nan')
AT_NOMEM = (5.0e8 - 8192.0) / 192.0           # pieces that make `want` 5e8 exactly at room 192
assert AT_NOMEM * 192.0 + 8192.0 == 5.0e8
SIZES = [(5000.25, 700, 1300), (1000.5, 700, 1300),                                   # pieces above and below nf_in
         (250000.75, 9000, 17000), (12.0, 3, 1),
         (67108864.0, 700, 1300), (float(np.nextafter(67108864.0, 0.0)), 700, 1300),        # the runaway threshold from both sides
         (float('inf'), 700, 1300), (NAN, 700, 1300),
         (AT_NOMEM, 700, 1300), (float(np.nextafter(AT_NOMEM, np.inf)), 700, 1300), (AT_NOMEM + 1.0, 700, 1300)]      # out of memory, from both sides
CAPS = [(p, nv, nf, room) for p, nv, nf in SIZES for room in ROOMS]
CAPS += [(100.0, 1500000, int(AT_NOMEM), 192.0), (100.0, 1500000, int(AT_NOMEM) + 1, 192.0)]        # ... and through nf_in
SWEEPS = [(n, first) for n in (0, 1, 5, 6, 31, 32, 33) for first in (0, 1, 199, 200, 201, 1000, 1001, 1200, 1201, 6200, 6201, 100000)]
ITERS = [(n_relax, before, now) for n_relax in (0, 1, 3) for before in ((0, 0, 0), (5, 7, 9))
         for now in (before, (before[0] + 1, before[1], before[2]), (before[0], before[1] + 1, before[2]), (before[0], before[1], before[2] + 1))]
RETRIES = ['-', '0.3', '0.05', '0.01', '0', '-2', 'x', '3', '192']
VALENCES = [-5, 0, 1, 6, 16, 59, 60, 61, 1000]
LENGTHS = [1.0, 0.7, float(np.float32(0.3)), 12.5]


def _meshes():
    """inputs of the Morton cube, each a valid mesh for the restatement: a flat one, one whose vertices are one point, an ordinary one"""
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    flat = np.array([[0.25, -1, 3], [4.5, -1, 3], [4.5, 2, 3], [0.25, 2, 3]], np.float32)
    point = np.tile(np.array([[1.5, -2.25, 1e-3]], np.float32), (4, 1))
    rng = np.random.default_rng(7)
    ordinary = (rng.normal(size=(50, 3)) * [3.0, 1.0, 0.1] + [10.0, -20.0, 0.5]).astype(np.float32)
    tris = np.array([[i, i + 1, i + 2] for i in range(0, 48, 3)], np.int32)
    return {'flat': (flat, quad), 'point': (point, quad), 'ordinary': (ordinary, tris)}


MESHES = _meshes()


def _questions(d):
    q = []
    for kind, first, bids, seen_at in PASSES:
        q.append('pass %d %d %s %s' % (kind, first, ' '.join(map(str, bids)), ' '.join(map(str, seen_at))))
    for p, nv, nf, room in CAPS:
        q.append('cap %r %d %d %r' % (p, nv, nf, room))
    q += ['sweep %d %d' % s for s in SWEEPS]
    q += ['iter %d %d %d %d %d %d %d' % ((n,) + tuple(b) + tuple(c)) for n, b, c in ITERS]
    q += ['retry %s' % e for e in RETRIES]
    for name, (v, _) in MESHES.items():
        path = os.path.join(d, name + '.f32')
        v.tofile(path)
        q.append('cube %s %d' % (path, v.shape[0]))
    q.append('constants')
    q += ['lengths %r' % L for L in LENGTHS]
    q += ['valence %d' % v for v in VALENCES]
    return q


# ---- build and run -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=list(BUILDS))
def answers(request, tmp_path_factory):
    """{kind of question: [the fields of each answer line, in the order of the questions]} of one build's run"""
    build, flags = request.param, BUILDS[request.param]
    d = str(tmp_path_factory.mktemp('remesh_plan_' + build))
    src, exe, lst = (os.path.join(d, n) for n in ('remesh_plan.cpp', 'remesh_plan', 'questions.txt'))
    with open(src, 'w') as fh:
        fh.write(PROGRAM)
    questions = _questions(d)
    with open(lst, 'w') as fh:
        fh.write('\n'.join(questions) + '\n')
    # (plain g++, no HIP header on the include path: the header must not need one.  A compiler that cannot build with the sanitizers fails
    # the test: a skip would leave that half of it unchecked without anybody noticing)
    subprocess.check_call([CXX, '-O1', '-g', '-std=c++14', '-Wall', '-Werror'] + flags + ['-I', CSRC, '-o', exe, src])
    r = subprocess.run([exe, lst], capture_output=True, text=True, timeout=120)
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    for report in ('AddressSanitizer', 'LeakSanitizer', 'runtime error'):
        assert report not in r.stderr, r.stderr[-4000:]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith('answer ')]
    assert len(lines) == len(questions)
    got = {}
    for i, (q, l) in enumerate(zip(questions, lines)):
        assert int(l[1]) == i
        got.setdefault(q.split()[0], []).append(l[2:])
    return got


def test_the_header_includes_no_hip_header():
    txt = open(HEADER).read()
    assert 'hip_runtime' not in txt and '#include <hip' not in txt and '#include "' not in txt
    assert not re.search(r'\bhip[A-Z]\w*\s*\(', txt)                  # ... and calls no HIP function


def test_constants_thresholds_and_valence(answers):
    assert [int(x) for x in answers['constants'][0]] == list(ref.R_MAX) + [ROUNDS_CAP, 4, 8, 2, 7 * 64 + 5]
    for L, a in zip(LENGTHS, answers['lengths']):
        assert (float(a[0]), float(a[1])) == (4.0 / 3.0 * L, 4.0 / 5.0 * L)
    for v, a in zip(VALENCES, answers['valence']):
        assert int(a[0]) == (16 if v <= 0 else min(v, 60))


def test_pass_stop_rule_with_every_report_in(answers):
    """with every report in when it is first asked for, the rule launches exactly the rounds the restatement runs -- or, in a call that has
    used up its round numbers (which the restatement does not know of), the rounds that are left.  The restatement's counts cover what the
    cases are for: an empty first round, both sides of `< 8` and of `500 x`, a full R_MAX."""
    got = [int(a[0]) for a in answers['pass'][:N_ON_TIME]]
    seen = set()
    for (kind, first, bids, _), g in zip(PASSES[:N_ON_TIME], got):
        want = ref_rounds(kind, bids)
        seen.add((kind, want))
        assert g == min(want, max(ROUNDS_CAP - first, 0)), (kind, first, bids, g, want)
    for kind in range(3):
        by_hand = [ref_rounds(kind, b) for k, _, b, _ in PASSES[:N_ON_TIME] if k == kind][:11]
        R = ref.R_MAX[kind]
        assert by_hand == [1, 2, R, 4, R, 4, 5, R, R, 3, R], (kind, by_hand)
        assert {w for k, w in seen if k == kind} >= set(range(1, 12)) | {R}
    # close to ROUNDS_CAP: what is left of the call's 4095 rounds, 0 included
    cap_cases = [(first, g) for (kind, first, bids, _), g in zip(PASSES[:N_ON_TIME], got) if first >= ROUNDS_CAP - 3 and bids[1] == 100]
    assert sorted(set(cap_cases)) == [(ROUNDS_CAP - 3, 3), (ROUNDS_CAP - 2, 2), (ROUNDS_CAP - 1, 1), (ROUNDS_CAP, 0)]


def test_pass_stop_rule_with_late_reports(answers):
    """Each report may come in as late as the decision about the round after next.  The rule then launches the restatement's rounds or
    ONE more, never two: +1 is what the code shows, and it is tight.
      * Never fewer: the host sees a subset of what the restatement knows, and either half of the rule only ever stops on a report seen.
      * Let the restatement stop before round T.  If it stops for a round of so few, that round is T - 2 or earlier, the host has waited
        for its report before it decides about round T, and stops there as well.  If it stops for an empty round, that round is T - 1, whose
        report is in at the decision about round T + 1 at the latest: one round more.
    (The GPU test, tests/test_hip_remesh_edges.py, allows two more per pass; its window is wider than need be and stays as it is.)"""
    late = list(zip(PASSES[N_ON_TIME:], answers['pass'][N_ON_TIME:]))
    extra = {}
    for (kind, first, bids, _), a in late:
        want = ref_rounds(kind, bids)
        assert want <= int(a[0]) <= want + 1, (kind, first, bids, a, want)
        extra[int(a[0]) - want] = extra.get(int(a[0]) - want, 0) + 1
    print('rounds beyond the restatement\'s: %r' % (extra,))
    kind, first, bids, _ = PASSES[LATE_EMPTY]
    assert int(answers['pass'][LATE_EMPTY][0]) == ref_rounds(kind, bids) + 1 == 3
    assert extra.get(0, 0) > 300 and extra.get(1, 0) > 300          # (the random passes reach both)


def capacities_ref(pieces, nv_in, nf_in, room):
    """-> (0, Fcap, Vcap, Hcap, list), (1, ...) for a runaway input or (2, ...) for one that is too large; in float64 and uint64 as the header"""
    if not np.float64(pieces) < np.float64(67108864.0):
        return (1, 0, 0, 0, 0)
    want = np.maximum(np.float64(pieces), np.float64(nf_in)) * np.float64(room) + np.float64(8192.0)
    if want > np.float64(5.0e8):
        return (2, 0, 0, 0, 0)
    Fcap = np.array([np.floor(want)]).astype(np.uint64)
    Vcap = np.array([nv_in], np.uint64) + (Fcap - np.array([nf_in], np.uint64)) // np.uint64(2) + np.uint64(1024)
    Hcap = np.uint64(3) * Fcap
    return (0, int(Fcap[0]), int(Vcap[0]), int(Hcap[0]), int(Hcap[0] // np.uint64(2) + np.uint64(64)))


def test_capacities(answers):
    got = {c: tuple(int(x) for x in a) for c, a in zip(CAPS, answers['cap'])}
    for c in CAPS:
        assert got[c] == capacities_ref(*c), (c, got[c])
        if got[c][0] == 0:
            assert got[c][1] >= c[2], 'a case of this test with fewer face slots than input faces: Vcap would wrap'
    # the thresholds, from both sides
    assert got[(67108864.0, 700, 1300, 1.5)][0] == 1 and got[(float(np.nextafter(67108864.0, 0.0)), 700, 1300, 1.5)][0] == 0
    assert got[(NAN, 700, 1300, 1.5)][0] == 1
    assert got[(AT_NOMEM, 700, 1300, 192.0)] == (0, 500000000, 700 + (500000000 - 1300) // 2 + 1024, 1500000000, 750000064)
    assert got[(float(np.nextafter(AT_NOMEM, np.inf)), 700, 1300, 192.0)][0] == 2 and got[(AT_NOMEM + 1.0, 700, 1300, 192.0)][0] == 2
    assert got[(100.0, 1500000, int(AT_NOMEM), 192.0)][0] == 0 and got[(100.0, 1500000, int(AT_NOMEM) + 1, 192.0)][0] == 2
    # pieces below nf_in: the input's faces decide
    assert got[(1000.5, 700, 1300, 1.5)][1] == int(1300 * 1.5 + 8192) and got[(5000.25, 700, 1300, 1.5)][1] == int(5000.25 * 1.5 + 8192.0)


def test_sweep_and_iteration_rules(answers):
    for (n, first), a in zip(SWEEPS, answers['sweep']):
        assert bool(int(a[0])) == ref.sweeps_end(n, first), (n, first)
    assert {ref.sweeps_end(*s) for s in SWEEPS} == {True, False}
    for (n_relax, before, now), a in zip(ITERS, answers['iter']):
        assert bool(int(a[0])) == ref.iterations_end(n_relax, before, now), (n_relax, before, now)
    assert sum(ref.iterations_end(*i) for i in ITERS) == 2


def test_retry_schedule(answers):
    """1.5, or NW_REMESH_ROOM as atof reads it with a floor of 0.05; doubled each time; eight tries"""
    first = {'-': 1.5, '0.3': 0.3, '0.05': 0.05, '0.01': 0.05, '0': 0.05, '-2': 0.05, 'x': 0.05, '3': 3.0, '192': 192.0}
    for env, a in zip(RETRIES, answers['retry']):
        assert [float(x) for x in a] == [first[env] * 2.0 ** t for t in range(8)], env


@pytest.mark.parametrize('name', list(MESHES))
def test_morton_cube(answers, name):
    v, f = MESHES[name]
    m = ref._Mesh(v, f, 1.0, 16, False)
    a = [float(x) for x in answers['cube'][list(MESHES).index(name)]]
    assert a[:3] == [float(x) for x in m.lo]
    assert a[3] == 1024.0 / m.ext
    assert (m.ext == 1e-30) == (name == 'point')
