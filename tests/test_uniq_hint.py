"""The run-length code in colex_at's spare bits (encode_core.h uniq_code; derived.cpp
build_paths writes it, EntryView::run_from reads it instead of puniq), on the CPU: the
emulator's records with the code on must equal the oracle's and the emulator's with
NTC_UNIQ_HINT=0, on reads that put the first clear puniq bit on each side of the code's
three thresholds, on the benchmark's shapes, on reads longer than the largest threshold, on
ragged lengths, at path breaks, on a strain collection and with the suffix table as deep as k.
The stand-alone program tests/uniq_hint_cpu (address and undefined-behaviour sanitizers) holds
the words build_paths writes against the code's definition from puniq."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ntcomp_amd as nt
import uniq_hint_lib as ul
from emu_lib import _p, make_view
from oracle_lib import REPO, pack_reads
from subst_lib import Env

KINDS = 14   # encode_core.h kTrKinds
PUNIQ = 12   # kTrPuniq


_trace = None


def trace_lib():
    """the emulator's trace build (scripts/trace_lines.py's): line counts and NTC_STAT counters"""
    global _trace
    if _trace is None:
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "tests", "emu"), "libntc_emu_trace.so"])
        L = ctypes.CDLL(os.path.join(REPO, "tests", "emu", "libntc_emu_trace.so"))
        P, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.emu_encode.restype = ctypes.c_int
        L.emu_encode.argtypes = [P, P, P, u64, P, u64, P, P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.emu_trace_report.argtypes = [P]
        L.emu_stats.argtypes = [P]
        _trace = L
    return _trace


def _traced(ix, k, bases, offs, tab_u, env):
    """-> (records, offsets, puniq lines per read in the parse, checksum of every left-extension
    test's result: parse_read's NTC_STAT 15)"""
    L = trace_lib()
    v, keep = make_view(ix.n, k, ix.rows, ix.C, ix.lcs)
    total = int(offs[-1])
    recs = np.zeros(total + 1, dtype=np.uint64)
    roff = np.zeros(len(offs), dtype=np.uint64)
    bad = ctypes.c_int64(-1)
    out = np.zeros(1 + 4 * KINDS, dtype=np.uint64)
    st = np.zeros(16, dtype=np.uint64)
    with Env(NTC_TRACE_GROUP=1, **env):
        L.emu_trace_report(_p(out))  # (both calls clear their counters)
        L.emu_stats(_p(st))
        rc = L.emu_encode(ctypes.byref(v), _p(bases), _p(offs), len(offs) - 1, _p(recs), len(recs), _p(roff),
                          ctypes.byref(bad), None, None, 4, 1, tab_u)
        L.emu_trace_report(_p(out))
        L.emu_stats(_p(st))
    assert rc == 0, (rc, bad.value)
    lines = out[1 + 2 * KINDS:].reshape(2, KINDS)
    return recs[: int(roff[-1])], roff, float(lines[1][PUNIQ]) / float(out[0]), int(st[15])


def _both(ix, k, reads, tab_u=0, **env):
    """emulator records with the code on and off: both must be the oracle's, and every
    left-extension test must have returned the same count (the records alone would hide most
    differences: the parse's jump loop folds the count)"""
    bases, offs, exp, eoff = ul.oracle_records(ix, k, reads)
    sums = {}
    for hint in (1, 0):
        got, goff, _, sums[hint] = _traced(ix, k, bases, offs, tab_u, dict(env, NTC_UNIQ_HINT=hint))
        assert np.array_equal(goff, eoff), hint
        assert np.array_equal(got, exp), hint
    assert sums[1] == sums[0] and sums[0] > 0


@pytest.mark.parametrize("k", [15, 31])
def test_repeats_reach_every_threshold_edge(k):
    seqs, ix, reads, probes = ul.repeat_case(k)
    # what repeat_case built holds: the read's end is a d = k position, t - 1 steps of the
    # left-extension test succeed below it and the t-th fails on a non-singleton at d = k
    from oracle_lib import OracleIndex
    orc = OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs)
    uniq = ul.singleton_bits(ix, k)
    seen = set()
    for i, t in probes:
        r = reads[i]
        d, s = orc.ms(r.encode())
        d, s = np.asarray(d, dtype=np.int64), np.asarray(s, dtype=np.int64)
        x = len(r) - 1
        below = (d[x - t:x] == k) & uniq[s[x - t:x]]
        assert d[x] == k and below[1:].all() and d[x - t] == k and not below[0], (i, t)
        seen.add(t)
    assert seen == set(ul.EDGES), sorted(set(ul.EDGES) - seen)
    _both(ix, k, reads)
    _both(ix, k, reads, NTC_EMU_JOINT=0)


@pytest.mark.parametrize("k", [31, 91])
def test_benchmark_shapes(k):
    seqs, ix, reads = ul.random_case(k)
    _both(ix, k, reads, NTC_EMU_JOINT=0)  # the build the upload picks for one genome
    _both(ix, k, reads[:500])


def test_long_reads_mix_code_and_fallback():
    seqs, ix, reads = ul.long_case()
    _both(ix, 31, reads, NTC_EMU_JOINT=0)


@pytest.mark.parametrize("k", [31, 91])
def test_ragged_read_lengths(k):
    seqs, ix, reads = ul.ragged_case(k)
    assert {len(r) for r in reads} == set(range(k + 2, k + 141))
    _both(ix, k, reads, NTC_EMU_JOINT=0)


@pytest.mark.parametrize("k", [15, 31])
def test_record_ends_at_the_start_of_a_run_entry(k):
    seqs, ix, reads = ul.read_start_case(k)
    _both(ix, k, reads)
    _both(ix, k, reads, NTC_EMU_JOINT=0)


def test_strain_collection_joint_runs():
    seqs, ix, reads = ul.strain_case()
    _both(ix, 23, reads)


def test_suffix_table_as_deep_as_k():
    k = 11
    g = nt.synth_genome(111, 60_000)
    ix = nt.Index.build([g.tobytes()], k)
    reads = ul.chop(nt.synth_reads(g, 5, 0, 600, 150, 10_000), 150)
    _both(ix, k, reads, tab_u=k)
    _both(ix, k, reads, tab_u=k, NTC_EMU_JOINT=0)


def test_code_removes_the_puniq_lines():
    """distinct puniq lines per read in the parse, 60 kb genome at k = 91, fall below a tenth
    with the code on"""
    seqs, ix, reads = ul.random_case(91)
    bases, offs = pack_reads(reads)
    r0, _, off, _ = _traced(ix, 91, bases, offs, 0, dict(NTC_UNIQ_HINT=0, NTC_EMU_JOINT=0))
    r1, _, on, _ = _traced(ix, 91, bases, offs, 0, dict(NTC_UNIQ_HINT=1, NTC_EMU_JOINT=0))
    print(f"puniq lines per read: {off:.4f} without the code, {on:.4f} with it")
    assert np.array_equal(r0, r1)
    assert off > 0.3   # the reference point is the parse as it was
    assert on < off / 10


def test_words_match_the_definition_under_sanitizers(tmp_path):
    """tests/uniq_hint_cpu: run_from with the code against run_from without it on made-up entries,
    then build_paths' words against the code's definition from puniq"""
    src = os.path.join(REPO, "tests", "uniq_hint_cpu", "uniq_hint_cpu.cpp")
    exe = str(tmp_path / "uniq_hint_cpu")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-g", "-std=c++17",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(REPO, "include"), src,
                    os.path.join(REPO, "ntcomp_amd", "csrc", "derived.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)   # run_from on made-up entries
    assert r.returncode == 0 and r.stdout.startswith("sweep:"), r.stdout + r.stderr
    calls, coded = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    assert calls > 100_000 and 0 < coded < calls
    cases = [ul.repeat_index(15), ul.repeat_index(31), ul.random_case(31)[:2], ul.random_case(91)[:2],
             ul.strain_case()[:2]]
    ks = [15, 31, 31, 91, 23]
    codes_seen = set()
    for (seqs, ix), k in zip(cases, ks):
        path = str(tmp_path / f"ix_{k}_{ix.n}.bin")
        with open(path, "wb") as f:
            f.write(np.array([ix.n, k] + [int(c) for c in ix.C[:4]], dtype=np.uint64).tobytes())
            for c in range(4):
                f.write(np.ascontiguousarray(ix.rows[c], dtype=np.uint64)[: (ix.n + 63) // 64].tobytes())
            f.write(np.ascontiguousarray(ix.lcs, dtype=np.uint8)[: ix.n].tobytes())
        env = dict(os.environ)
        env.pop("NTC_UNIQ_HINT", None)
        r = subprocess.run([exe, path], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        counts = [int(x) for x in r.stdout.split("codes:")[1].split()[:4]]
        codes_seen |= {c for c in range(4) if counts[c]}
    assert codes_seen == {0, 1, 2, 3}
