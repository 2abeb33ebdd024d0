"""Quality smoothing inside long reference matches, the parts that need no GPU: the per-read
logic of k_q_smooth compiled for the CPU under ASan + UBSan (tests/qsmooth_cpu) against the
checker, the Python surface, the refusals of both command lines, and the checker's own
self-test.

The checker is qsmooth_lib.py (numpy): the rule by its definition, over the CPU oracle's records
or over records made by hand."""
import inspect
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ntcomp_amd as nt
import qsmooth_lib as qs
import qual_lib as ql
from oracle_lib import OracleIndex

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")


# ---- records by hand ----------------------------------------------------------------------------
def long_rec(L, first=0):
    assert 11 < L < 1 << 24
    return (first << 56) | (L << 32) | 0x1234


def short_rec(L, first=0):
    assert 0 < L <= 11
    return ((first + 2) | (L << 2)) << 56 | 0x2B


def recs_of(lens, longs):
    """record lengths in archive order (rightmost first) -> uint64 records"""
    return np.array([long_rec(L, j == len(lens) - 1) if lg else short_rec(L, j == len(lens) - 1)
                     for j, (L, lg) in enumerate(zip(lens, longs))], dtype=np.uint64)


# ---- the checker itself ---------------------------------------------------------------------------
def test_checker_on_a_hand_made_read():
    # 40 bases: archive order = a short record of 3 (positions 37..39), a long one of 20 (17..36), a short
    # one of 5 (12..16), a long one of 12 (0..11)
    recs = recs_of([3, 20, 5, 12], [False, True, False, True])
    lens, is_long = qs.rec_lengths(recs)
    assert lens.tolist() == [3, 20, 5, 12] and is_long.tolist() == [False, True, False, True]
    t12 = qs.trusted_of_read(40, recs, 12)
    assert np.flatnonzero(t12).tolist() == list(range(0, 12)) + list(range(17, 37))
    t13 = qs.trusted_of_read(40, recs, 13)
    assert np.flatnonzero(t13).tolist() == list(range(17, 37))
    assert not qs.trusted_of_read(40, recs, 21).any()
    q = np.frombuffer(b"#5F!" * 10, dtype=np.uint8)
    out, count = qs.smooth(q, t13, "keep", b"I")
    exp = bytearray(b"#5F!" * 10)
    for i in range(17, 37):
        if exp[i] > ord("#"):
            exp[i] = ord("I")
    assert out.tobytes() == bytes(exp) and count == 10  # '#' and '!' stay: at or below the floor
    # bin8: the floor is the level of '#' (q 2 -> 6, the byte '\''), the target the level of 'I' (q 40)
    assert qs.floor_target("bin8", b"I") == (39, 73) and qs.floor_target("keep", b"5") == (35, 53)
    outb, countb = qs.smooth(ql.mode_table("bin8")[q], t13, "bin8", b"I")
    assert countb == 10 and set(outb[17:37].tolist()) == {39, 33, 73}  # '#' -> 39 stays, '!' stays, the rest 73
    # a short record never counts, whatever M; two reads in a batch keep their own ends
    offs, roff = np.array([0, 40, 52]), np.array([0, 4, 5])
    both = np.concatenate([recs, recs_of([12], [True])])
    assert np.flatnonzero(qs.trusted(offs, both, roff, 12)).tolist() == \
        list(range(0, 12)) + list(range(17, 37)) + list(range(40, 52))


# ---- the lane logic on the CPU, under ASan + UBSan ----------------------------------------------
@pytest.fixture(scope="module")
def lane_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qsmooth_cpu") / "qsmooth_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "qsmooth_cpu", "qsmooth_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _lanes(exe, tmp_path, M, mode, to, lead, block_reads, lens, recs, roff, q):
    """q: the bytes after the mode's table -> (bytes replaced, presence maps as sets per block, q')"""
    offs = np.zeros(len(lens) + 1, dtype="<u8")
    offs[1:] = np.cumsum(lens)
    blob = struct.pack("<IIIIIIQQ", M, ql.MODES[mode], to[0], lead, block_reads, 0, len(lens), len(recs)) + \
        offs.tobytes() + np.asarray(roff, dtype="<u8").tobytes() + np.asarray(recs, dtype="<u8").tobytes() + bytes(q)
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:] + r.stderr[-2000:])
    out = (tmp_path / "out.bin").read_bytes()
    count, nb = struct.unpack_from("<QQ", out, 0)
    pres = []
    for b in range(nb):
        p0, p1 = struct.unpack_from("<QQ", out, 16 + 16 * b)
        pres.append({c for c in range(128) if ((p0 if c < 64 else p1) >> (c & 63)) & 1})
    got = np.frombuffer(out, dtype=np.uint8, offset=16 + 16 * nb)
    assert len(got) == int(offs[-1])
    return count, pres, got, offs


def _check(exe, tmp_path, M, mode, to, lead, block_reads, lens, recs, roff, q):
    count, pres, got, offs = _lanes(exe, tmp_path, M, mode, to, lead, block_reads, lens, recs, roff, q)
    mask = qs.trusted(offs, np.asarray(recs, dtype=np.uint64), roff, M)
    exp, exp_count = qs.smooth(np.frombuffer(bytes(q), dtype=np.uint8), mask, mode, to)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
    assert count == exp_count
    for b, p in enumerate(pres):  # the presence map of each block is that of its smoothed bytes
        r0, r1 = b * block_reads, min((b + 1) * block_reads, len(lens))
        assert p == set(exp[int(offs[r0]):int(offs[r1])].tolist()), b
    return exp_count, mask


def _hand_batch(M):
    """reads of 1, 11, 12, M - 1, M and M + 1 bases, a read that is one long record, a read of
    short records only, and a read of more than 64 records (130: long ones of M, M - 1 and 12
    bases among short ones, so that chunks start and end inside trusted and untrusted ground)"""
    reads = [([1], [False]), ([11], [False]), ([12], [True]), ([M - 1], [M - 1 > 11]), ([M], [True]), ([M + 1], [True]),
             ([700], [True]), ([11, 3, 7, 1, 11], [False] * 5)]
    big_l, big_g = [], []
    for j in range(130):
        if j % 3 == 0:
            big_l.append([M, max(M - 1, 12), 12, M + 5][(j // 3) % 4])
            big_g.append(True)
        else:
            big_l.append(1 + (5 * j) % 11)
            big_g.append(False)
    reads.append((big_l, big_g))
    # a read whose long records abut, and one with a long record of M between two of M - 1
    reads.append(([M, M, 3, M], [True, True, False, True]))
    reads.append(([max(M - 1, 12), M, max(M - 1, 12)], [True] * 3))
    lens = [sum(l) for l, _ in reads]
    recs = np.concatenate([recs_of(l, g) for l, g in reads])
    roff = np.zeros(len(reads) + 1, dtype=np.uint64)
    roff[1:] = np.cumsum([len(l) for l, _ in reads])
    return lens, recs, roff


@pytest.mark.parametrize("M", [12, 13, 32, 70])
@pytest.mark.parametrize("lead", range(8))
def test_lane_logic_hand_made_records_at_every_alignment(lane_exe, tmp_path, M, lead):
    """The array starts `lead` bytes into a word, so over the eight leads every read starts and
    ends at each of the word offsets 0..7."""
    lens, recs, roff = _hand_batch(M)
    rng = np.random.default_rng(100 * M + lead)
    q = rng.choice(np.frombuffer(b"!#$5FI", dtype=np.uint8), sum(lens))
    count, mask = _check(lane_exe, tmp_path, M, "keep", b"I", lead, 4, lens, recs, roff, q)
    assert 0 < count < mask.sum() < len(q)  # '!' and '#' on trusted ground stayed
    offs = np.concatenate([[0], np.cumsum(lens)])
    per_read = [mask[offs[r]:offs[r + 1]] for r in range(len(lens))]
    assert [bool(m.all()) for m in per_read[:8]] == [False, False, M == 12, False, True, True, True, False]
    assert not per_read[3].any() and not per_read[7].any() and per_read[8].any() and not per_read[8].all()


def test_lane_logic_word_edges_at_both_ends(lane_exe, tmp_path):
    """A trusted record that starts at word offset a and ends at word offset b, for every a and
    b: short records of a and 8 - b bases (or none) on its sides."""
    M, lens, recs = 12, [], []
    for a in range(8):
        for b in range(8):
            L = 24 + b - a  # every read is whole words long, so each starts on a word boundary
            rl = ([8 - b] if b else []) + [L] + ([a] if a else [])  # (archive order: rightmost first)
            rg = ([False] if b else []) + [True] + ([False] if a else [])
            lens.append(sum(rl))
            recs.append(recs_of(rl, rg))
    roff = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    assert all(n % 8 == 0 for n in lens)
    q = np.full(sum(lens), ord("5"), dtype=np.uint8)
    count, mask = _check(lane_exe, tmp_path, M, "keep", b"~", 0, 64, lens, np.concatenate(recs), roff, q)
    assert count == sum(24 + b - a for a in range(8) for b in range(8))


@pytest.mark.parametrize("mode,to", [("keep", b"I"), ("bin8", b"I"), ("bin8", b"+"), ("keep", b"$")])
def test_lane_logic_on_the_oracles_records(lane_exe, tmp_path, mode, to):
    """Reads with 1 % errors, random reads and one read of 5,000 bases through the CPU oracle."""
    k, M = 31, 32
    genome = nt.synth_genome(7, 20_000)
    ix = nt.Index.build([genome.tobytes()], k)
    orc = OracleIndex(ix.n, k, ix.rows, ix.C, ix.lcs)
    rng = np.random.default_rng(5)
    flat = nt.synth_reads(genome, 2, 0, 300, 150, 10_000).tobytes()
    reads = [flat[150 * i:150 * i + int(rng.integers(1, 151))] for i in range(300)]
    reads += [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 90)) for _ in range(5)]
    long_read = bytearray(genome.tobytes()[3000:8000])
    for p in rng.integers(0, 5000, 120):
        long_read[p] = b"ACGT"[(b"ACGT".index(long_read[p]) + 1) % 4]
    reads.append(bytes(long_read))
    recs, roff, offs = qs.oracle_records(orc, reads)
    assert int(roff[-1] - roff[-2]) > 64  # the long read loops over chunks
    q = ql.mode_table(mode)[rng.integers(33, 75, int(offs[-1])).astype(np.uint8)]
    count, mask = _check(lane_exe, tmp_path, M, mode, to, 3, 64, [len(r) for r in reads], recs, roff, q)
    assert 0.3 < mask.mean() < 0.95 and count > 0


# ---- the Python surface -------------------------------------------------------------------------
def test_python_surface():
    for fn in (nt.GpuContext.encode_pack_fastq, nt.GpuContext.encode_pack_fastq_paired):
        p = inspect.signature(fn).parameters
        assert p["quality_smooth"].default is None and p["quality_smooth_to"].default is None
    for prop in ("quality_smooth", "quality_smooth_to", "quality_smoothed"):
        assert isinstance(getattr(nt.GpuContext, prop), property), prop
    assert nt.GpuContext.quality_smoothed.fset is None  # read-only
    assert (nt.QUALITY_SMOOTH_MIN, nt.QUALITY_SMOOTH_MAX, nt.QUALITY_SMOOTH_DEFAULT) == (12, 16777215, 32)
    assert nt.QUALITY_SMOOTH_TO == b"I"
    assert [nt._smooth_code(m) for m in (0, 12, 32, 16777215, np.int64(40))] == [0, 12, 32, 16777215, 40]
    for bad in (1, 11, -1, 16777216, 2 ** 40, "32", 32.0, None, True):
        with pytest.raises(ValueError, match="quality_smooth"):
            nt._smooth_code(bad)
    assert [nt._smooth_to_code(t) for t in (b"I", "I", 73, b"$", b"~")] == [73, 73, 73, 36, 126]
    for bad in (b"#", b"\x7f", b" ", b"", b"II", "II", 35, 127, None, 1.5, "éé"):
        with pytest.raises(ValueError, match="quality_smooth_to"):
            nt._smooth_to_code(bad)


# ---- both command lines: refused with status 2 before any GPU is opened -------------------------
def _cli(which, *args, cwd):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), cwd=cwd, capture_output=True, env=env, timeout=120)


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_refusals(tmp_path, which):
    (tmp_path / "r.fq").write_text("@r\nACGT\n+\nIIII\n")
    # (no index exists under that prefix: a call that got past its arguments would fail otherwise, status 1)
    common = ["encode", "-i", str(tmp_path / "noindex"), str(tmp_path / "r.fq")]
    keep = ["--qualities", "keep", "--quality-file", str(tmp_path / "q.ntcq")]
    bin8 = ["--qualities", "bin8", "--quality-file", str(tmp_path / "q.ntcq")]

    def refused(args, msg):
        r = _cli(which, *common, *args, cwd=tmp_path)
        assert r.returncode == 2 and r.stdout == b"", (args, r.returncode, r.stderr)
        assert b"ntcomp: encode: " + msg in r.stderr, (args, r.stderr)
        assert not (tmp_path / "q.ntcq").exists()  # nothing is written

    for q in ([], ["--qualities", "drop"]):
        refused(q + ["--quality-smooth"], b"--quality-smooth needs --qualities keep or bin8")
        refused(q + ["--quality-smooth", "40"], b"--quality-smooth needs --qualities keep or bin8")
        refused(q + ["--quality-smooth-to", "5"], b"--quality-smooth-to needs --qualities keep or bin8")
    for m in ("0", "1", "11", "16777216", "99999999999"):
        refused(keep + ["--quality-smooth", m], b"--quality-smooth: M must be 12..16777215")
    refused(keep + ["--quality-smooth=x"], b"--quality-smooth: M must be 12..16777215")
    for c in ("#", "!", "II", "", " ", "\x7f"):
        refused(keep + ["--quality-smooth", "--quality-smooth-to=" + c], b"--quality-smooth-to: one printable byte in '$'..'~'")
    for c in ("$", "(", "*"):
        refused(bin8 + ["--quality-smooth", "32", "--quality-smooth-to", c], b"--quality-smooth-to: under bin8")
    # accepted arguments get as far as the index, which is not there: not status 2
    for ok in (keep + ["--quality-smooth"], keep + ["--quality-smooth", "12", "--quality-smooth-to", "$"],
               bin8 + ["--quality-smooth=16777215", "--quality-smooth-to", "+"], ["--quality-smooth"] + keep):
        r = _cli(which, *common, *ok, cwd=tmp_path)
        assert r.returncode not in (0, 2), (ok, r.returncode, r.stderr)


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_help_lists_the_flags(tmp_path, which):
    r = _cli(which, "encode", "--help", cwd=tmp_path)
    assert r.returncode == 0 and b"--quality-smooth" in r.stdout and b"--quality-smooth-to" in r.stdout
