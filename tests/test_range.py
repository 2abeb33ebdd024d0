"""Decoding a range of reads, the parts that need no GPU: ntc_archive_info on archives built with
the host codec, the window's rule (window_core.h) compiled for the CPU under ASan + UBSan
(tests/window_cpu) against the checker, the shard arithmetic, both command lines' parsing and
refusals, and the C and Python surface.

The checker is range_lib.py (plain Python); it tests itself on import."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import ntcomp_amd as nt
import ntcomp_amd.cli as cli
import range_lib as rl
from test_unpack import random_records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")


# ---- ntc_archive_info ---------------------------------------------------------------------------
def _block(rng, n_recs, n_reads):
    recs = random_records(rng, n_recs)
    recs[0] = np.uint64(5 | (12 << 32))  # one long record
    recs[-1] = np.uint64(1 | ((2 | (1 << 2)) << 56))  # and one short one: the block is written
    return nt.write_block(recs, n_reads), n_recs


def _archive(rng, shape):
    """file header + one block per (records, reads) of shape -> (bytes, [(offset, bytes, reads, records)])"""
    data, want = nt.file_header(), []
    for n_recs, n_reads in shape:
        blob, _ = _block(rng, n_recs, n_reads)
        want.append(dict(offset=len(data), bytes=len(blob), reads=n_reads, records=n_recs, bad=0))
        data += blob
    return data, want


def _info(tmp_path, data):
    (tmp_path / "a.dat").write_bytes(data)
    return nt.archive_info(str(tmp_path / "a.dat"))


def test_info_of_an_empty_archive(tmp_path):
    for data in (nt.file_header(), b""):
        assert _info(tmp_path, data) == dict(blocks=[], n_blocks=0, n_reads=0, n_records=0, tail_bytes=0)


def test_info_of_one_partial_block(tmp_path):
    data, want = _archive(np.random.default_rng(1), [(700, 300)])
    assert _info(tmp_path, data) == dict(blocks=want, n_blocks=1, n_reads=300, n_records=700, tail_bytes=0)


def test_info_of_three_blocks_and_a_part(tmp_path):
    shape = [(70_000, 65_536), (66_000, 65_536), (65_536, 65_536), (40, 17)]
    data, want = _archive(np.random.default_rng(2), shape)
    got = _info(tmp_path, data)
    assert got["blocks"] == want and got["n_blocks"] == 4 and got["tail_bytes"] == 0
    assert got["n_reads"] == 3 * 65_536 + 17 and got["n_records"] == sum(s[0] for s in shape)
    assert want[-1]["offset"] + want[-1]["bytes"] == len(data)


def test_info_flags_a_bad_middle_block_and_lists_the_rest(tmp_path):
    data, want = _archive(np.random.default_rng(3), [(500, 200), (600, 200), (300, 90)])
    bad = bytearray(data)
    at = want[1]["offset"] + 12  # stream 0's encoded_size: it no longer matches its gzip trailer
    bad[at:at + 4] = struct.pack("<I", struct.unpack_from("<I", data, at)[0] + 1)
    got = _info(tmp_path, bytes(bad))
    want[1] = dict(want[1], reads=0, records=0, bad=1)
    assert got["blocks"] == want and got["n_blocks"] == 3 and got["n_reads"] == 290 and got["n_records"] == 800
    # damage in a gzip payload, not a header, is not seen here: nothing is inflated
    pay = bytearray(data)
    mid = want[1]["offset"] + 32 + 40
    pay[mid:mid + 8] = bytes(8)
    assert _info(tmp_path, bytes(pay))["blocks"][1]["bad"] == 0


def test_info_reports_a_truncated_tail(tmp_path):
    data, want = _archive(np.random.default_rng(4), [(500, 200), (600, 200)])
    for cut_at in (want[1]["offset"] + 10, want[1]["offset"] + 32 + 5, len(data) - 1):
        got = _info(tmp_path, data[:cut_at])
        assert got["blocks"] == want[:1] and got["n_reads"] == 200 and got["tail_bytes"] == cut_at - want[1]["offset"]
    assert _info(tmp_path, data + b"xyz")["tail_bytes"] == 3
    with pytest.raises(nt.NtcError) as e:
        nt.archive_info(str(tmp_path / "missing.dat"))
    assert e.value.code == 9  # NTC_ERR_IO


# ---- window_core.h against the checker -------------------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("window_cpu") / "window_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "window_cpu", "window_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _core(exe, tmp_path, text, first, count, paired=False):
    recs = rl.records(text)
    blob = struct.pack("<4Q", len(recs), first, count, int(paired)) + struct.pack(f"<{len(recs)}Q", *map(len, recs)) + text
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    out = (tmp_path / "out.bin").read_bytes()
    if struct.unpack_from("<Q", out)[0] == 0:
        assert len(out) == 8
        return None
    total = struct.unpack_from("<Q", out, 8)[0]
    assert total == len(out) - 16
    return out[16:]


def _text(rng, n, fastq):
    """n records with ids crossing 99 -> 100, reads of 0..300 bases"""
    out = []
    for r in range(n):
        ln = int(rng.integers(0, 301))
        read = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), ln))
        if fastq:
            out.append(b"@n%d x\n" % r + read + b"\n+\n" + b"I" * ln + b"\n")
        else:
            out.append(b">seq.%d\n" % (95 + r) + read + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("fastq", [False, True])
def test_core_windows_equal_the_cut(core_exe, tmp_path, fastq):
    n = 150  # a 64-read name-chain restart inside, and a last partial group
    text = _text(np.random.default_rng(5 + fastq), n, fastq)
    windows = [(0, n), (0, 1), (n - 1, 1), (63, 2), (62, 4), (127, 2), (1, n - 2), (64, 64)]
    for first, count in windows:
        assert rl.window_ok(first, count, n)
        assert _core(core_exe, tmp_path, text, first, count) == rl.cut(text, first, first + count), (first, count)
        sizes = [len(x) for x in rl.records(text)]
        assert sum(rl.window_sizes(sizes, first, count)) == len(rl.cut(text, first, first + count))


def test_core_refuses_what_the_checker_refuses(core_exe, tmp_path):
    text = _text(np.random.default_rng(7), 10, False)
    for first, count, paired in [(0, 0, False), (5, 0, False), (10, 1, False), (9, 2, False), (0, 11, False), (11, 0, False),
                                 (2**63, 2**63, False), (1, 2**64 - 1, False), (1, 2, True), (2, 3, True), (0, 1, True)]:
        assert not rl.window_ok(first, count, 10, paired)
        assert _core(core_exe, tmp_path, text, first, count, paired) is None, (first, count, paired)
    for first, count in [(0, 10), (2, 4), (8, 2)]:  # whole pairs pass
        assert rl.window_ok(first, count, 10, True)
        assert _core(core_exe, tmp_path, text, first, count, True) == rl.cut(text, first, first + count)
    assert _core(core_exe, tmp_path, b"", 0, 1) is None  # an empty batch has no window


# ---- shard arithmetic --------------------------------------------------------------------------------
def test_shards_partition_the_blocks():
    for n in range(1, 8):
        for nb in range(0, 10):
            slices = [nt.shard_blocks(i, n, nb) for i in range(1, n + 1)]
            assert slices == [rl.shard(i, n, nb) for i in range(1, n + 1)]
            assert slices[0][0] == 0 and slices[-1][1] == nb
            assert all(a[1] == b[0] for a, b in zip(slices, slices[1:])) and all(lo <= hi for lo, hi in slices)
            assert max(hi - lo for lo, hi in slices) - min(hi - lo for lo, hi in slices) <= 1
    for i, n in ((0, 3), (4, 3), (1, 0)):
        with pytest.raises(ValueError):
            nt.shard_blocks(i, n, 5)


def test_block_range_of_the_checker_by_hand():
    reads = [65_536, 65_536, 65_536, 3_392]
    assert rl.block_range(reads, 0, 1) == (0, 0, 0, 0, 65_535)
    assert rl.block_range(reads, 65_535, 2) == (0, 1, 0, 65_535, 65_535)
    assert rl.block_range(reads, 65_536, 65_536) == (1, 1, 65_536, 0, 0)
    assert rl.block_range(reads, 199_999, 1) == (3, 3, 196_608, 3_391, 0)
    assert rl.block_range(reads, 0, 200_000) == (0, 3, 0, 0, 0)


# ---- command lines ------------------------------------------------------------------------------------
SPECS = ["3-9", "7", "7-", "-4", "1-1", "", "-", "0", "0-3", "5-4", "1-2-3", "a-b", "1,2", " 3", "--4", "3 ", "+3", "1e3"]
SHARDS = ["1/1", "2/4", "4/4", "0/4", "5/4", "2", "/4", "2/", "a/b", "1/0", "1/2/3", " 1/2", "-1/2"]


def test_the_python_parsers_agree_with_the_checker():
    for spec in SPECS:
        want = rl.parse_reads(spec)
        if want is None:
            with pytest.raises(ValueError):
                cli.parse_reads(spec)
        else:
            assert cli.parse_reads(spec) == want, spec
    for spec in SHARDS:
        want = rl.parse_shard(spec)
        if want is None:
            with pytest.raises(ValueError):
                cli.parse_shard(spec)
        else:
            assert cli.parse_shard(spec) == want, spec


@pytest.fixture(scope="module")
def small_archive(tmp_path_factory):
    """four blocks of 10, 10, 10 and 3 reads (an odd block would make a pair slice start inside a pair)"""
    d = tmp_path_factory.mktemp("arch")
    data, want = _archive(np.random.default_rng(8), [(40, 10), (40, 10), (30, 10), (20, 3)])
    (d / "enc.dat").write_bytes(data)
    data, _ = _archive(np.random.default_rng(9), [(40, 9), (40, 10)])
    (d / "odd.dat").write_bytes(data)
    return d, want


def _run(cli_name, args, cwd):
    head = [sys.executable, "-m", "ntcomp_amd"] if cli_name == "python" else [NATIVE]
    return subprocess.run(head + args, capture_output=True, cwd=cwd, env=dict(os.environ, PYTHONPATH=REPO), timeout=120)


@pytest.mark.parametrize("cli_name", ["python", "native"])
def test_both_command_lines_refuse_with_status_2(small_archive, tmp_path, cli_name):
    """before any GPU is opened: no index is there to be loaded"""
    d, _ = small_archive
    enc, odd = str(d / "enc.dat"), str(d / "odd.dat")
    refused = [["decode", "-i", "idx", "--reads", s, enc] for s in SPECS if rl.parse_reads(s) is None and s not in ("--4", "-")]
    refused += [["decode", "-i", "idx", "--reads=" + s, enc] for s in ("--4", "-")]
    refused += [["decode", "-i", "idx", "--shard", s, enc] for s in SHARDS if rl.parse_shard(s) is None and not s.startswith("-")]
    refused += [
        ["decode", "-i", "idx", "--reads", "1-4", "--shard", "1/2", enc],
        ["verify", "-i", "idx", "--digest-file", "d.ntcd", "--reads", "1-4", "--shard", "1/2", enc],
        ["verify", "-i", "idx", "--digest-file", "d.ntcd", "--reads", "9-3", enc],
        ["decode", "-i", "idx", "--reads", "2-5", "--mate-out", "r2.out", enc],  # A must be odd
        ["decode", "-i", "idx", "--reads", "3-5", "--mate-out", "r2.out", enc],  # B must be even
        ["decode", "-i", "idx", "--reads", "4", "--mate-out", "r2.out", enc],
        ["decode", "-i", "idx", "--reads", "33-", "--mate-out", "r2.out", enc],  # ... to the archive's last read, the 33rd
        ["decode", "-i", "idx", "--reads", "34", enc],  # the archive holds 33 reads
        ["decode", "-i", "idx", "--reads", "30-34", enc],
        ["decode", "-i", "idx", "--shard", "2/2", "--mate-out", "r2.out", odd],  # the slice starts at read 10 (from 1): inside a pair
    ]
    for args in refused:
        r = _run(cli_name, args, tmp_path)
        assert r.returncode == 2, (args, r.stdout[-300:], r.stderr[-300:])
        assert r.stdout == b"" and not os.listdir(tmp_path)


@pytest.mark.parametrize("cli_name", ["python", "native"])
def test_an_empty_shard_writes_nothing_and_exits_0(small_archive, tmp_path, cli_name):
    d, _ = small_archive
    (tmp_path / "none.dat").write_bytes(nt.file_header())
    r = _run(cli_name, ["decode", "-i", "idx", "--shard", "1/5", str(d / "enc.dat")], tmp_path)  # blocks [0, 0)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-300:]
    r = _run(cli_name, ["decode", "-i", "idx", "--shard", "2/3", str(tmp_path / "none.dat")], tmp_path)
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-300:]


@pytest.mark.parametrize("cli_name", ["python", "native"])
def test_info_on_both_command_lines(small_archive, tmp_path, cli_name):
    d, want = small_archive
    size = sum(b["bytes"] for b in want)
    r = _run(cli_name, ["info", str(d / "enc.dat")], tmp_path)
    assert r.returncode == 0 and r.stdout == b"blocks 4 reads 33 records 130 bytes %d trailing_bytes 0\n" % size, r.stderr
    r = _run(cli_name, ["info", "--blocks", str(d / "enc.dat")], tmp_path)
    lines = r.stdout.decode().splitlines()
    assert r.returncode == 0 and len(lines) == 5 and lines[0].startswith("blocks 4 reads 33 ")
    first = 1
    for i, (ln, b) in enumerate(zip(lines[1:], want)):
        assert ln == f"block {i} offset {b['offset']} bytes {b['bytes']} reads {b['reads']} records {b['records']} first_read {first}"
        first += b["reads"]
    # a damaged header: listed, and a non-zero status; trailing bytes are reported
    bad = bytearray((d / "enc.dat").read_bytes())
    bad[want[2]["offset"] + 12] ^= 0x10
    (tmp_path / "bad.dat").write_bytes(bytes(bad[:-7]))
    r = _run(cli_name, ["info", "--blocks", str(tmp_path / "bad.dat")], tmp_path)
    lines = r.stdout.decode().splitlines()
    assert r.returncode not in (0, 2) and lines[0].endswith(f"trailing_bytes {want[3]['bytes'] - 7} damaged_blocks 1")
    assert lines[0].startswith("blocks 3 reads 20 ") and lines[3].endswith(" reads 0 records 0 damaged") and len(lines) == 4
    assert _run(cli_name, ["info", str(tmp_path / "missing.dat")], tmp_path).returncode == 1


# ---- the C and Python surface ---------------------------------------------------------------------------
def test_c99_consumer_pins_the_new_structs(small_archive, tmp_path):
    exe = str(tmp_path / "abi_range")
    libdir = os.path.join(REPO, "ntcomp_amd")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "abi_range.c"), "-o", exe, "-L", libdir, "-lntcomp_gpu", "-Wl,-rpath," + libdir]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe, str(small_archive[0] / "enc.dat")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert '"ntc_file_opts5": 112' in r.stdout and '"ntc_r_stats": 56' in r.stdout and '"ntc_archive_block": 40' in r.stdout
    assert "info rc 0 blocks 4 reads 33 records 130 tail 0" in r.stdout
    assert ctypes.sizeof(nt.FileOpts5) == 112 and ctypes.sizeof(nt.RStats) == 56 and ctypes.sizeof(nt.ArchiveBlock) == 40
    assert [f[0] for f in nt.FileOpts5._fields_[:-2]] == [f[0] for f in nt.FileOpts4._fields_]
    assert nt.FileOpts5.read_first.offset == 96 and nt.FileOpts5.read_count.offset == 104


def test_the_new_symbols_are_declared_and_exported():
    heads = "".join(open(os.path.join(REPO, "include", h)).read() for h in ("ntcomp_codec.h", "ntcomp_pipeline.h"))
    L = nt.lib()
    for sym in ("ntc_decode_set_window", "ntc_decode_file_ex5", "ntc_archive_info"):
        assert sym + "(" in heads and sym in nt.EXPORTED and hasattr(L, sym)
    assert callable(nt.GpuContext.set_window) and callable(nt.archive_info) and callable(nt.shard_blocks)
    import inspect
    assert "reads" in inspect.signature(nt.decode_file).parameters
    assert [n for n, _ in nt.RStats._fields_] == ["blocks_total", "reads_total", "first_block", "blocks_read", "reads_written",
                                                  "head_skipped", "tail_skipped"]


def test_ex5_checks_its_struct_before_anything_else():
    """no context is needed to be refused: a null or short struct is NTC_ERR_INVALID_ARG"""
    L = nt.lib()
    o, st = nt.PipelineOpts(), nt.PipelineStats()
    assert L.ntc_decode_file_ex5(None, 0, b"x", 1, None, ctypes.byref(o), ctypes.byref(st), None, None, None) == 1
    fo = nt.FileOpts5(ctypes.sizeof(nt.FileOpts4), 0, -1, 0, -1, None, None, 0, -1, None, 0, -1, None, 0, None, -1, 0, 0)
    assert L.ntc_decode_file_ex5(None, 0, b"x", 1, ctypes.byref(fo), ctypes.byref(o), ctypes.byref(st), None, None, None) == 1
    assert L.ntc_decode_set_window(None, 0, 1) == 1
