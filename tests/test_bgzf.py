"""BGZF members without a GPU: the host restatement behind ntc_bgzf_compress(NULL, ...) -- the member
plan of bgzf_core.h and the coder of deflate_core.h run by one lane -- against a plan model in Python
integers (bgzf_lib.plan), a member parser, zlib, gzip and the library's own inflater; and the same
headers compiled alone under ASan + UBSan (tests/bgzf_cpu)."""
import ctypes
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bgzf_lib as bl
import ntcomp_amd as nt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, CAPACITY, UNSUPPORTED = 1, 5, 9
SHAPES = bl.shapes()


def test_constants_match_the_headers():
    src = open(os.path.join(REPO, "ntcomp_amd", "csrc", "bgzf_core.h")).read()
    assert "kBgzfMember = %d;" % bl.M in src and "kBgzfGrid = %d;" % bl.G in src
    hdr = open(os.path.join(REPO, "include", "ntcomp_codec.h")).read()
    assert "#define NTC_BGZF_MEMBER %d" % bl.M in hdr and "#define NTC_BGZF_GRID %d" % bl.G in hdr
    assert nt.BGZF_EOF == bl.EOF and len(bl.EOF) == 28 and gzip.decompress(bl.EOF) == b""
    assert (nt.BGZF_MEMBER_BYTES, nt.BGZF_GRID) == (bl.M, bl.G)
    for n in (0, 1, bl.G, bl.G + 1, bl.M, bl.M + 1, 10 ** 7):
        assert nt.bgzf_bound(n) == bl.bound(n)


def test_the_model_on_the_shapes_it_was_built_for():
    """what the issue says of the shapes, said of the model: the library is held to the model below"""
    p = lambda name: bl.plan(len(SHAPES[name][0]), SHAPES[name][1])
    assert [len(p("plain%d" % n)) for n in (0, 1, 32768, 32769, 65280, 65281, 130560)] == [0, 1, 1, 1, 1, 2, 2]
    assert p("R0") == [] and p("R1") == [(0, 100)]
    assert p("ends_on_grid") == [(0, bl.G)]
    assert p("starts_on_grid") == [(0, bl.G), (bl.G, bl.G), (2 * bl.G, 500)]
    assert p("over3841") == [(0, bl.G - 3840), (bl.G - 3840, bl.M), (2 * bl.G, 1000)]  # the cell is exactly M
    assert p("over3842") == [(0, bl.G - 3841), (bl.G - 3841, bl.M), (2 * bl.G - 1, 1), (2 * bl.G, 1000)]  # and one more
    assert p("one140000") == [(0, bl.M), (bl.M, bl.M), (2 * bl.M, 140000 - 2 * bl.M)]  # two empty cells, plain cuts
    assert p("largest") == [(0, 0xFF00)]
    for name in ("fasta", "fastq", "zero_runs", "zero_on_grid", "long_between"):
        text, off = SHAPES[name]
        starts = {int(o) for o in off}
        inside_long = [a for a, _ in p(name) if a not in starts]
        assert bool(inside_long) == (name == "long_between"), name  # only a record past 3,841 bytes is cut inside


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(name):
    text, off = SHAPES[name]
    blob, table = nt.bgzf_compress(text, off)
    members = bl.check(blob, table, text, off)
    assert nt.bgzf_compress(text, off)[0] == blob
    # the library's own reader of BGZF input takes every member
    found = nt.bgzf_members(blob)
    assert [(a, b, c) for a, b, c in found] == [(p, b, isize) for p, b, _, isize in members]
    out, res = nt.inflate_members(None, blob, found)
    assert (res["status"] == 0).all() and out.tobytes() == text
    if name in ("random", "largest"):  # nothing to gain: every chunk is stored, 5 bytes each
        assert len(blob) == len(text) + sum(26 + 5 * len(bl.chunks(n)) for _, n in bl.plan(len(text), off))
    if name == "largest":
        assert len(blob) == bl.MAX_MEMBER and struct.unpack_from("<H", blob, 16)[0] == 0xFFFF - 220
    if name in ("one_byte", "fasta", "fastq"):
        assert len(blob) < len(text) // 2


def test_offsets_only_matter_through_the_cuts():
    """equal offsets are interchangeable: dropping the empty records changes no byte"""
    text, off = SHAPES["zero_runs"]
    dense = np.unique(off)
    assert len(dense) < len(off)
    assert nt.bgzf_compress(text, dense)[0] == nt.bgzf_compress(text, off)[0]


def test_refusals():
    text, off = SHAPES["fasta"]
    for o in (None, off):
        with pytest.raises(nt.NtcError) as e:
            nt.bgzf_compress(text, o, cap=bl.bound(len(text)) - 1)
        assert e.value.code == CAPACITY and e.value.needed == bl.bound(len(text))
        assert nt.bgzf_compress(text, o, cap=bl.bound(len(text)))[0] == nt.bgzf_compress(text, o)[0]
    bad = []
    o = off.copy()
    o[0] = 1
    bad.append(o)
    o = off.copy()
    o[-1] -= 1
    bad.append(o)
    bad.append(np.append(off, off[-1] + 1))
    o = off.copy()
    o[7], o[8] = o[8], o[7]
    bad.append(o)
    for o in bad:
        with pytest.raises(nt.NtcError) as e:
            nt.bgzf_compress(text, o)
        assert e.value.code == INVALID_ARG
    # a member table too small for the members
    src = np.frombuffer(text, np.uint8)
    out = np.zeros(bl.bound(len(text)), np.uint8)
    tab = np.zeros(2, nt.BGZF_MEMBER)
    nm, used = ctypes.c_uint64(), ctypes.c_uint64()
    rc = nt.lib().ntc_bgzf_compress(None, src.ctypes.data, len(text), off.ctypes.data, len(off) - 1, out.ctypes.data, len(out),
                                    tab.ctypes.data, 2, ctypes.byref(nm), ctypes.byref(used))
    assert rc == CAPACITY and nm.value == len(bl.plan(len(text), off)) > 2


def test_decode_file_ex7_checks_its_struct(tmp_path):
    """a short struct_bytes, a non-zero reserved2 and an unknown format are refused before anything is opened"""
    assert ctypes.sizeof(nt.FileOpts7) == ctypes.sizeof(nt.FileOpts6) + 8
    o, ps = nt.PipelineOpts(0, 2, 0, 0, 0), nt.PipelineStats()

    def call(fo):
        return nt.lib().ntc_decode_file_ex7(None, 0, os.fsencode(str(tmp_path / "none.dat")), 1, ctypes.byref(fo), ctypes.byref(o),
                                            ctypes.byref(ps), None, None, None, None)

    values = (0, -1, 0, -1, None, None, 0, -1, None, 0, -1, None, 0, None, -1, 0, 0, 0, 0)
    for size in (0, ctypes.sizeof(nt.FileOpts6), ctypes.sizeof(nt.FileOpts7) - 1):
        assert call(nt.FileOpts7(size, *values, 1, 0)) == INVALID_ARG
    assert call(nt.FileOpts7(ctypes.sizeof(nt.FileOpts7), *values, 1, 1)) == INVALID_ARG
    assert call(nt.FileOpts7(ctypes.sizeof(nt.FileOpts7), *values, 2, 0)) == INVALID_ARG
    assert nt.OUT_FORMATS == {"text": 0, "bgzf": 1}
    hdr = open(os.path.join(REPO, "include", "ntcomp_pipeline.h")).read()
    assert "#define NTC_OUT_TEXT 0" in hdr and "#define NTC_OUT_BGZF 1" in hdr


# ---- the headers alone, under ASan + UBSan --------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgzf_cpu") / "bgzf_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "bgzf_cpu", "bgzf_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_stand_alone_program_over_the_shapes(cpu_exe, tmp_path):
    names = sorted(SHAPES)
    with open(tmp_path / "in.bin", "wb") as f:
        for name in names:
            text, off = SHAPES[name]
            f.write(struct.pack("<QQ", len(text), 0 if off is None else len(off)))
            f.write(text)
            if off is not None:
                f.write(np.asarray(off, "<u8").tobytes())
    r = subprocess.run([cpu_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-3000:]
    out, at = (tmp_path / "out.bin").read_bytes(), 0
    for name in names:
        text, off = SHAPES[name]
        nm, size = struct.unpack_from("<QQ", out, at)
        table = np.frombuffer(out, nt.BGZF_MEMBER, nm, at + 16)
        blob = out[at + 16 + 32 * nm:at + 16 + 32 * nm + size]
        at += 16 + 32 * nm + size
        bl.check(blob, table, text, off)
        assert blob == nt.bgzf_compress(text, off)[0], name  # the library's bytes
    assert at == len(out)
