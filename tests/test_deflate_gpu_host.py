"""NTC_DEFLATE_GPU without a GPU: the host restatement of the device's deflate coder
(deflate_core.h) through ntc_deflate_stream / ntc_deflate_block, and the same header compiled
alone under ASan + UBSan (tests/deflate_cpu).  The checkers are Python's zlib (which verifies CRC-32
and ISIZE) and the library's own reader (libdeflate when present).

A stream of the container is whole 64-bit words, so the C ABI carries multiples of 8 bytes only:
through it go the listed sizes that are such multiples and, for every other one, the multiples of 8
on both sides of it (deflate_lib.WORD_SIZES); the byte-exact list 0, 1, 2, 3, 4, C - 1, ... runs
through the stand-alone program, which is the same coder and takes any size."""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import ntcomp_amd as nt
import deflate_lib as dl
from test_codec_golden import CASES, recs_of, parse_container

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
INVALID_ARG = 1
WORD = dict(dl.word_cases())


def test_constants_match_the_header():
    src = open(os.path.join(REPO, "ntcomp_amd", "csrc", "deflate_core.h")).read()
    assert "#define NTC_DF_CHUNK %d " % dl.C in src and "kDfB = %d;" % dl.B in src
    hdr = open(os.path.join(REPO, "include", "ntcomp_codec.h")).read()
    assert "#define NTC_DEFLATE_GPU %d" % dl.ENGINE_GPU in hdr and nt.DEFLATE_ENGINES["gpu"] == dl.ENGINE_GPU


@pytest.mark.parametrize("name", sorted(WORD))
def test_sizes_and_contents(name):
    """every member inflates to its input, is one member, keeps the bound; two calls agree"""
    data = WORD[name]
    m = dl.member_of(data)
    dl.check_member(m, data)
    assert dl.member_of(data) == m
    if name.startswith(("random", "all256", "one3")) or (name.startswith("size") and (len(data) // 8) % 2):
        assert dl.all_stored(m, len(data)), name  # nothing to gain: every chunk is stored
    if name.startswith(("zero", "period")):
        assert len(m) < len(data) // 8 + 64  # the matches are used
    if name.startswith("far") and len(data) == dl.C:
        # the 300 random bytes once (about 8.2 bits each with their code's header) and their copy as two
        # matches of the last distance code; as literals the copy alone would be 300 bytes more
        assert len(m) < 18 + 300 + 250
    if name.startswith("fib"):
        assert len(m) < 0.5 * len(data)  # (about 2.6 bits of entropy per byte: Huffman is chosen)


def test_word_sizes_cover_the_list():
    assert all(s % 8 == 0 for s in dl.WORD_SIZES)
    for x in dl.SIZES:
        assert (x // 8) * 8 in dl.WORD_SIZES and -(-x // 8) * 8 in dl.WORD_SIZES
    for n in dl.WORD_SIZES:
        assert "size%d" % n in WORD and len(WORD["size%d" % n]) == n


def test_a_match_stops_at_the_chunk_boundary():
    """a repeat that runs over the boundary: each chunk inflates alone, from its own bytes"""
    data = dl.content("straddle", dl.MULTI)
    m = dl.member_of(data)
    dl.check_member(m, data)
    d = zlib.decompressobj(-15)
    first = d.decompress(m[10:], dl.C)  # the first chunk's blocks end on a byte boundary...
    assert first == data[:dl.C]
    # ... and what follows is a deflate stream of its own: nothing in it points before the boundary
    used = len(m) - 10 - len(d.unconsumed_tail) - len(d.unused_data)
    assert used > 0


def _fib_bytes(k, seed):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    data = b"".join(bytes([40 + i]) * c for i, c in enumerate(f))
    return bytes(np.random.default_rng(seed).permutation(np.frombuffer(data, np.uint8))), f


def test_limiter_acts_on_fibonacci_frequencies():
    """Exact Fibonacci counts.  One chunk holds 21 symbols of them (28,656 bytes): with the end-of-block
    symbol the unlimited Huffman code is 21 bits deep, and the format has no way to say more than 15, so
    a member that is not stored and inflates was cut to 15 bits and kept complete.  Then 28 symbols over
    many chunks.  The size: a Huffman code spends less than p_max + 0.086 bits per symbol over the
    entropy (Gallager), p_max = 0.382 here, and the cut to 15 bits moves a few symbols of frequency
    below 2^-15 -- together under 0.5 bits; a chunk's code description is under 100 bytes."""
    for k, seed in ((21, 1), (28, 2)):
        data, f = _fib_bytes(k, seed)
        data = data[:len(data) // 8 * 8]
        assert (k == 21 and len(data) == 28656 < dl.C) or len(data) > 20 * dl.C
        m = dl.member_of(data)
        dl.check_member(m, data)
        p = np.array(f, np.float64) / sum(f)
        h = float(-(p * np.log2(p)).sum())
        assert not dl.all_stored(m, len(data))
        assert len(m) < len(data) * (h + 0.5) / 8 + 100 * -(-len(data) // dl.C) + 18, (k, len(m), h)


@pytest.mark.parametrize("name", sorted(n for n in CASES if not CASES[n]["dropped"]))
def test_fixture_blocks(name):
    """the four streams of every codec fixture: ntc_deflate_block with engine 3 equals the four
    ntc_deflate_stream parts, holds the fixture's streams, and reads back through nt.read_block"""
    c = CASES[name]
    recs = recs_of(c)
    meta, payload = nt.pack_block(recs, c["num_records"])
    whole = nt.deflate_block(meta, payload, "gpu")
    assert b"".join(nt.deflate_stream(meta, s, payload, "gpu") for s in range(4)) == whole
    assert nt.deflate_block(meta, payload, "gpu") == whole
    for s, (h, member) in enumerate(parse_container(whole)):
        exp = c["streams"][s]
        assert h == {"num_records": c["num_records"], "num_u64": exp["num_u64"], "encoded_size": exp["encoded_size"],
                     "param": exp["param"]}
        dl.check_member(member, bytes.fromhex(exp["payload"]))
    got, used, nrec = nt.read_block(whole)
    assert used == len(whole) and nrec == c["num_records"] and np.array_equal(got, recs)


def test_dropped_fixture_keeps_its_status():
    for name in sorted(n for n in CASES if CASES[n]["dropped"]):
        meta, payload = nt.pack_block(recs_of(CASES[name]), CASES[name]["num_records"])
        with pytest.raises(nt.NtcError) as e:
            nt.deflate_block(meta, payload, "gpu")
        assert e.value.code == 3


def test_golden_blocks():
    """the goldens' reads through the oracle and the host packer: engine 3 round-trips"""
    from oracle_lib import OracleIndex, golden_names, load_golden, pack_reads
    seen = 0
    for name in golden_names():
        g = load_golden(name)
        if "reads" not in g:
            continue
        ix = OracleIndex(g["n"], g["k"], g["rows_u64"], g["C"], g["lcs_u8"])
        bases, offs = pack_reads(g["reads"])
        try:
            recs, _ = ix.encode(bases, offs)
        except RuntimeError:
            continue
        meta, payload = nt.pack_block(recs, len(offs) - 1)
        if meta.status:
            continue
        got, used, nrec = nt.read_block(nt.deflate_block(meta, payload, "gpu"))
        assert np.array_equal(got, recs) and nrec == len(offs) - 1
        seen += 1
    assert seen


@pytest.fixture(scope="module")
def c91():
    return dl.c91_block()


def test_the_coder_uses_what_it_finds(c91):
    """the small C91-shaped block: s3's member beats Huffman-only deflate, s2's is no larger than
    its own, s1 and s4 come out stored"""
    meta, payload = c91
    raw = nt.stream_payloads(meta, payload)
    size = []
    for s in range(4):
        m = nt.deflate_stream(meta, s, payload, "gpu")[32:]
        dl.check_member(m, raw[s])
        h = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        size.append((len(raw[s]), len(m) - 18, len(h.compress(raw[s]) + h.flush())))
        print("s%d raw %d gpu %d huffman-only %d" % ((s + 1,) + size[-1]))
        if s in (0, 3):
            assert dl.all_stored(m, len(raw[s])), s
    assert size[2][1] < size[2][2]
    assert size[1][1] <= size[1][2]
    got, _, _ = nt.read_block(nt.deflate_block(meta, payload, "gpu"))
    assert len(got) == meta.n_recs


def test_refusals(c91):
    meta, payload = c91
    for engine in (4, -1, 99):
        for s in range(4):
            assert dl.deflate_stream_rc(meta, s, payload, engine)[0] == INVALID_ARG
    buf = np.frombuffer(payload, dtype=np.uint8)
    out, n = ctypes.c_void_p(), ctypes.c_uint64()
    assert nt.lib().ntc_deflate_block(ctypes.byref(meta), buf.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(out),
                                      ctypes.byref(n)) == INVALID_ARG
    # the side sections are out of scope: a sound (empty) section deflates under the host engines, and
    # engine 3 is refused there, engine 4 everywhere
    words = np.zeros(64, np.uint8)
    for cls, fn in ((nt.QualMeta, nt.lib().ntc_q_deflate_section), (nt.NameMeta, nt.lib().ntc_n_deflate_section)):
        m = cls()
        for engine, want in ((0, 0), (3, INVALID_ARG), (4, INVALID_ARG), (-1, INVALID_ARG)):
            rc = fn(ctypes.byref(m), words.ctypes.data_as(ctypes.c_void_p), engine, ctypes.byref(out), ctypes.byref(n))
            assert rc == want, (cls.__name__, engine)
            if out:
                nt.lib().ntc_buffer_free(out)
                out = ctypes.c_void_p()


@pytest.mark.parametrize("which", ["native", "python"])
def test_misspelt_engine_exits_with_2(which, tmp_path):
    """before an index is read or a GPU opened: the index prefix does not exist"""
    head = [sys.executable, "-m", "ntcomp_amd"] if which == "python" else [NATIVE]
    r = subprocess.run(head + ["encode", "-i", str(tmp_path / "none"), "--deflate", "gpx", str(tmp_path / "none.fq")],
                       capture_output=True, env=dict(os.environ, PYTHONPATH=REPO, HIP_VISIBLE_DEVICES="-1"), timeout=120)
    assert r.returncode == 2 and b"--deflate" in r.stderr and b"gpu" in r.stderr


# ---- the header alone, under ASan + UBSan -------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate_cpu") / "deflate_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "deflate_cpu", "deflate_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_stand_alone_program_over_the_byte_exact_list(cpu_exe, tmp_path):
    cs = dl.cases()
    assert [len(d) for n, d in cs if n.startswith("size")] == dl.SIZES
    (tmp_path / "in.bin").write_bytes(b"".join(struct.pack("<Q", len(d)) + d for _, d in cs))
    r = subprocess.run([cpu_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-3000:]
    out, at = (tmp_path / "out.bin").read_bytes(), 0
    for name, data in cs:
        size, nc = struct.unpack_from("<QQ", out, at)
        choices = out[at + 16:at + 16 + nc]
        member = out[at + 16 + nc:at + 16 + nc + size]
        at += 16 + nc + size
        assert nc == max(1, -(-len(data) // dl.C)) and set(choices) <= {1, 2, 3}, name
        dl.check_member(member, data)
        if len(data) % 8 == 0:  # the same bytes as the library's
            assert member == dl.member_of(data), name
        if name.startswith(("random", "all256")):
            assert set(choices) == {1}, name
        if name.startswith(("zero", "period", "far")):
            assert 3 in choices, name
        if name.startswith("straddle") and len(data) > dl.C:
            assert choices[0] == 3  # the copy's part inside the first chunk is a match there
    assert at == len(out)
