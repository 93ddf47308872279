"""
The host half of handing a block's result back, without a GPU: ch_shrinkwrap_amd/csrc/nw_host_copy.h holds the copy threads (NwHostPool),
the row copier and the chunked copy-out that follows the flag word.  This test writes a stand-alone program around the header, builds it
with g++ three times (plain, -fsanitize=thread, -fsanitize=address,undefined) and runs each build as a child process.  The program reads
a list of cases, one per line, writes what each case left in the contiguous result and in the strided records to files, and prints one
line per case; the expected bytes are computed here with numpy.  A thread stands in for the device where the staging buffer is filled
slice by slice: it writes a slice into the poisoned source and then release-stores the flag word.
"""
import os
import platform
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'ch_shrinkwrap_amd', 'csrc')
HEADER = os.path.join(CSRC, 'nw_host_copy.h')
CXX = os.environ.get('CXX', 'g++')
BUILDS = {'plain': [], 'thread': ['-fsanitize=thread'], 'address_undefined': ['-fsanitize=address,undefined']}
SENTINEL_ROWS, SENTINEL_CONTIGUOUS = 0xA5, 0x5A

PROGRAM = r'''
#include "nw_host_copy.h"
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

static void dump(const std::string &dir, int idx, const char *ext, const void *p, size_t bytes)
{
    const std::string path = dir + "/" + std::to_string(idx) + "." + ext;
    FILE *fh = fopen(path.c_str(), "wb");
    if (!fh || fwrite(p, 1, bytes, fh) != bytes) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(fh);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    const std::string dir = argv[2];
    std::string line;
    for (int idx = 0; std::getline(in, line); ++idx) {
        std::istringstream ls(line);
        std::string kind, targets, valid_mode, writer;
        long long M, stride, slice_rows, v0, v1;
        int threads, flag_base, defer, give_up_ms;
        ls >> kind >> M >> stride >> targets >> valid_mode >> threads >> slice_rows >> flag_base >> writer >> defer >> give_up_ms >> v0 >> v1;
        if (!ls) { fprintf(stderr, "bad case line %d\n", idx); return 2; }
        // source rows: the floats whose bit patterns count up from 1.0f (the same array in numpy)
        std::vector<float> truth(3 * M), src(3 * M), contiguous(3 * M), snap_contiguous(3 * M);
        for (long long i = 0; i < 3 * M; ++i) { const uint32_t b = 0x3f800000u + (uint32_t)i; memcpy(&truth[i], &b, 4); }
        const bool written_late = writer != "none";
        if (written_late) memset(src.data(), 0xFF, src.size() * 4);         // poison: a chunk copied before its slice shows
        else src = truth;
        memset(contiguous.data(), 0x5A, contiguous.size() * 4);
        std::vector<unsigned char> rows((size_t)(M * stride), 0xA5), snap_rows(rows.size(), 0), valid(M);
        for (long long v = 0; v < M; ++v) valid[v] = valid_mode == "ones" ? 1 : valid_mode == "zeros" ? 0 : (unsigned char)(v & 1);
        float *cp = targets.find('c') != std::string::npos ? contiguous.data() : nullptr;
        void *rp = targets.find('r') != std::string::npos ? (void *)rows.data() : nullptr;
        const unsigned char *vp = valid_mode == "none" ? nullptr : valid.data();
        std::atomic<int> started(0);
        std::unique_ptr<NwHostPool> pool;
        if (threads > 0) { pool.reset(new NwHostPool()); pool->start(threads, [&started] { started.fetch_add(1); }); }
        int ret = 1;
        const auto t0 = std::chrono::steady_clock::now();
        if (kind == "rows") {
            nw_copy_rows(src.data(), v0, v1, cp, rp, stride, vp);
        } else if (kind == "arm") {
            // armed with nothing following: the threads spin out their 1.5 ms and sleep again; then a job straight behind arm(); then
            // shutdown() while they spin
            std::atomic<int> count(0);
            pool->arm();
            std::this_thread::sleep_for(std::chrono::milliseconds(3));
            pool->arm();
            pool->run_chunks(16, [&count](int) { count.fetch_add(1); });
            ret = count.load() == 16;
            pool->arm();
        } else {
            const int S = slice_rows > 0 ? (int)((M + slice_rows - 1) / slice_rows) : 0;
            alignas(64) int flag = flag_base + 1;                           // (the block's kernels have run: no slice yet)
            if (!written_late && S > 0) flag = flag_base + 1 + S + 3;       // every slice long there
            std::thread device;
            if (written_late)
                device = std::thread([&] {
                    for (int k = 0; k < S; ++k) {
                        std::this_thread::sleep_for(std::chrono::microseconds(200));      // (the copy threads are waiting by now)
                        const long long r0 = k * slice_rows, r1 = std::min<long long>(M, r0 + slice_rows);
                        memcpy(src.data() + 3 * r0, truth.data() + 3 * r0, (size_t)(r1 - r0) * 12);
                        __atomic_store_n(&flag, flag_base + 1 + (k + 1), __ATOMIC_RELEASE);
                        if (writer == "first") break;                       // the device falls silent after its first slice
                    }
                });
            ret = nw_copy_out_chunks(src.data(), M, cp, rp, stride, vp, pool.get(), slice_rows, flag_base, &flag, defer != 0,
                                     std::chrono::milliseconds(give_up_ms)) ? 1 : 0;
            snap_contiguous = contiguous;                                   // what the call left, before anybody waits for the records
            if (kind == "defer_run") {
                // a job straight behind the posted one: it starts only when the records are complete
                pool->run_chunks(4, [&](int c) { if (c == 0) snap_rows = rows; });
                rows = snap_rows;
            } else if (kind == "defer_shutdown") {
                pool->shutdown();                                           // (the posted job outstanding: must return)
            } else if (pool) {
                pool->wait_posted();
            }
            contiguous = snap_contiguous;
            if (device.joinable()) device.join();
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (pool) pool->shutdown();
        dump(dir, idx, "contiguous", contiguous.data(), contiguous.size() * 4);
        dump(dir, idx, "rows", rows.data(), rows.size());
        printf("case %d ret=%d started=%d ms=%.3f\n", idx, ret, started.load(), ms);
    }
    return 0;
}
'''


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def case(kind, M, stride=40, targets='cr', valid='alt', threads=0, slice_rows=0, flag_base=0, writer='none', defer=0, give_up_ms=10000,
         v0=0, v1=None):
    return dict(kind=kind, M=M, stride=stride, targets=targets, valid=valid, threads=threads, slice_rows=slice_rows, flag_base=flag_base,
                writer=writer, defer=defer, give_up_ms=give_up_ms, v0=v0, v1=M if v1 is None else v1)


CASES = {}
for M in (1, 8191, 8192, 8193):
    for stride in (12, 40):
        for targets in ('c', 'r', 'cr'):
            for valid in ('none', 'ones', 'zeros', 'alt'):
                CASES['rows-%d-%d-%s-%s' % (M, stride, targets, valid)] = case('rows', M, stride, targets, valid)
CASES['rows-inner-range'] = case('rows', 8193, 40, 'cr', 'alt', v0=1, v1=8192)
# no slices: two chunks of 8192, the last holding one row
for T in (0, 1, 2, 8):
    CASES['chunks-8193-pool%d' % T] = case('chunks', 8193, threads=T)
# slices through the flag word: three slices, the last partial, chunk = 4096; and chunk = 8192, two chunks per slice
for T in (0, 1, 2, 8):
    CASES['sliced-4096-pool%d' % T] = case('chunks', 10242, threads=T, slice_rows=4096, flag_base=1000, writer='all')
for T in (2, 8):
    CASES['sliced-16384-pool%d' % T] = case('chunks', 20000, threads=T, slice_rows=16384, flag_base=1000, writer='all')
CASES['sliced-4096-flag-past-need'] = case('chunks', 10242, threads=8, slice_rows=4096, flag_base=1000)
# the device falls silent after its first slice: false after the give-up time
for T in (0, 8):
    CASES['silent-pool%d' % T] = case('chunks', 10242, threads=T, slice_rows=4096, flag_base=1000, writer='first', give_up_ms=50)
# the strided records behind the caller's back
for T in (1, 2, 8):
    CASES['deferred-20000-pool%d' % T] = case('chunks', 20000, threads=T, defer=1)
CASES['deferred-rows-only'] = case('chunks', 20000, targets='r', threads=8, defer=1)
CASES['deferred-sliced'] = case('chunks', 10242, threads=8, slice_rows=4096, flag_base=1000, writer='all', defer=1)
CASES['deferred-then-a-job'] = case('defer_run', 20000, threads=8, defer=1)
CASES['deferred-then-shutdown'] = case('defer_shutdown', 20000, threads=8, defer=1)
CASES['arm'] = case('arm', 1, threads=8)
NAMES = list(CASES)
FIELDS = ['kind', 'M', 'stride', 'targets', 'valid', 'threads', 'slice_rows', 'flag_base', 'writer', 'defer', 'give_up_ms', 'v0', 'v1']


def source(M):
    return (np.arange(3 * M, dtype=np.uint32) + np.uint32(0x3f800000)).view(np.float32).reshape(M, 3)


def valid_mask(c):
    M = c['M']
    return {'none': np.ones(M, bool), 'ones': np.ones(M, bool), 'zeros': np.zeros(M, bool), 'alt': (np.arange(M) & 1).astype(bool)}[c['valid']]


def expected(c, v0=None, v1=None):
    """-> (contiguous bytes, record bytes) after rows [v0, v1) have been copied"""
    M, stride = c['M'], c['stride']
    v0, v1 = c['v0'] if v0 is None else v0, c['v1'] if v1 is None else v1
    src = source(M)
    contiguous = np.full(12 * M, SENTINEL_CONTIGUOUS, np.uint8)
    if 'c' in c['targets']:
        contiguous[12 * v0:12 * v1] = src[v0:v1].view(np.uint8).ravel()
    rows = np.full((M, stride), SENTINEL_ROWS, np.uint8)
    if 'r' in c['targets']:
        sel = valid_mask(c) & (np.arange(M) >= v0) & (np.arange(M) < v1)
        rows[sel, :12] = src.view(np.uint8).reshape(M, 12)[sel]
    return contiguous, rows.ravel()


# ---- build and run -------------------------------------------------------------------------------------------------------------------------
def _links(tmp, flags):
    one = os.path.join(tmp, 'one.cpp')
    with open(one, 'w') as fh:
        fh.write('int main() { return 0; }\n')
    return subprocess.run([CXX] + flags + ['-pthread', '-o', os.path.join(tmp, 'one'), one], capture_output=True).returncode == 0


@pytest.fixture(scope='module', params=list(BUILDS))
def run(request, tmp_path_factory):
    """{case name: (fields of its result line, contiguous bytes, record bytes)} of one build's run"""
    build, flags = request.param, BUILDS[request.param]
    d = str(tmp_path_factory.mktemp('host_copy_' + build))
    if flags and not _links(d, flags):
        pytest.skip('%s cannot link a program with %s' % (CXX, ' '.join(flags)))
    src, exe, lst, out = (os.path.join(d, n) for n in ('host_copy.cpp', 'host_copy', 'cases.txt', 'out'))
    with open(src, 'w') as fh:
        fh.write(PROGRAM)
    with open(lst, 'w') as fh:
        for name in NAMES:
            fh.write(' '.join(str(CASES[name][k]) for k in FIELDS) + '\n')
    os.mkdir(out)
    # (plain g++, no HIP header on the include path: the header must not need one)
    subprocess.check_call([CXX, '-O1', '-g', '-std=c++14', '-pthread', '-Wall', '-Werror'] + flags + ['-I', CSRC, '-o', exe, src])
    r = subprocess.run([exe, lst, out], capture_output=True, text=True, timeout=120)
    if 'unexpected memory mapping' in r.stderr and shutil.which('setarch'):
        # g++ 11.4's ThreadSanitizer runtime can fail to start any program, a one-line one included, under a recent kernel (seen on Linux
        # 6.18 where mmap addresses are randomised more widely than that runtime expects): "FATAL: ThreadSanitizer: unexpected memory
        # mapping", before main.  That says nothing about the program, so it is run once more with randomisation off, and said aloud.
        print('the ThreadSanitizer runtime could not map its shadow (%s): running the program again under setarch -R' % r.stderr.strip()[-120:])
        r = subprocess.run(['setarch', platform.machine(), '-R', exe, lst, out], capture_output=True, text=True, timeout=120)
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    for report in ('ThreadSanitizer', 'AddressSanitizer', 'LeakSanitizer', 'runtime error'):
        assert report not in r.stderr, r.stderr[-4000:]
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith('case ')]
    assert len(lines) == len(NAMES)
    got = {}
    for i, (name, l) in enumerate(zip(NAMES, lines)):
        assert int(l[1]) == i
        fields = dict(kv.split('=') for kv in l[2:])
        got[name] = (fields, np.fromfile(os.path.join(out, '%d.contiguous' % i), np.uint8), np.fromfile(os.path.join(out, '%d.rows' % i), np.uint8))
    shutil.rmtree(out)
    print('%s: %d cases, %.1f ms in them' % (build, len(NAMES), sum(float(g[0]['ms']) for g in got.values())))
    return got


def check(run, name, returned=1):
    c = CASES[name]
    fields, contiguous, rows = run[name]
    assert int(fields['ret']) == returned, (name, fields)
    assert int(fields['started']) == max(c['threads'] - 1, 0), (name, fields)          # the start callback, once per thread of the pool
    want_c, want_r = expected(c)
    assert contiguous.tobytes() == want_c.tobytes(), name
    assert rows.tobytes() == want_r.tobytes(), name


def test_the_header_includes_no_hip_header():
    txt = open(HEADER).read()
    assert 'hip_runtime' not in txt and '#include <hip' not in txt
    assert not re.search(r'\bhip[A-Z]\w*\s*\(', txt)                  # ... and calls no HIP function


@pytest.mark.parametrize('M', [1, 8191, 8192, 8193])
def test_row_copier(run, M):
    """every stride, pair of targets and mask at this size; bytes the copier does not own keep their sentinel"""
    names = [n for n in NAMES if n.startswith('rows-%d-' % M)]
    assert len(names) == 24
    for n in names:
        check(run, n)
    if M == 8193:
        check(run, 'rows-inner-range')


@pytest.mark.parametrize('pool', [0, 1, 2, 8])
def test_chunked_copy_out_without_slices(run, pool):
    check(run, 'chunks-8193-pool%d' % pool)


@pytest.mark.parametrize('name', [n for n in NAMES if n.startswith('sliced-')])
def test_chunked_copy_out_follows_the_flag_word(run, name):
    """no chunk is copied before the slice it ends in has been announced: none of the source's poison in the result"""
    check(run, name)


@pytest.mark.parametrize('pool', [0, 8])
def test_a_silent_device_is_given_up_on(run, pool):
    """only the first slice arrives: the call says so after its give-up time and every thread comes back (the program ended).  The first
    chunk (= the first slice) has been copied; nothing of the others."""
    name = 'silent-pool%d' % pool
    c = CASES[name]
    fields, contiguous, rows = run[name]
    assert int(fields['ret']) == 0
    assert 50.0 <= float(fields['ms']) < 5000.0, fields
    want_c, want_r = expected(c, 0, 4096)
    assert contiguous.tobytes() == want_c.tobytes()
    assert rows.tobytes() == want_r.tobytes()


@pytest.mark.parametrize('name', [n for n in NAMES if n.startswith('deferred-') and CASES[n]['kind'] == 'chunks'])
def test_deferred_rows(run, name):
    """the contiguous result as the call left it; the records after wait_posted()"""
    check(run, name)


def test_a_job_behind_a_posted_one_finds_it_finished(run):
    """(the records as the second job's first chunk saw them)"""
    check(run, 'deferred-then-a-job')


def test_shutdown_with_a_posted_job_outstanding_returns(run):
    """the program ended; the contiguous result is complete and every record is either written or untouched"""
    name = 'deferred-then-shutdown'
    c = CASES[name]
    fields, contiguous, rows = run[name]
    assert int(fields['ret']) == 1
    want_c, want_r = expected(c)
    assert contiguous.tobytes() == want_c.tobytes()
    rows, want_r = rows.reshape(c['M'], c['stride']), want_r.reshape(c['M'], c['stride'])
    assert ((rows == want_r).all(1) | (rows == SENTINEL_ROWS).all(1)).all()


def test_armed_threads_go_back_to_sleep_take_a_job_and_are_joined(run):
    fields = run['arm'][0]
    assert int(fields['ret']) == 1 and int(fields['started']) == 7
