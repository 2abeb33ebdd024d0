"""Paired-end reads, the parts that need no GPU: the mate rule by hand, the kernels' shared
logic (pair_core.h) compiled for the CPU under ASan + UBSan (tests/pair_cpu) against the
checker, and the C, Python and command-line surface.

The checker is pair_lib.py (plain Python); it tests itself on import."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import names_lib as nl
import ntcomp_amd as nt
import pair_lib as pl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
INVALID_ARG, FORMAT, UNSUPPORTED = 1, 8, 10
OK = (1 << 64) - 1
X = b"x" * 70

# (name 1, name 2, the mates agree)
RULE = [
    (b"x/1", b"x/2", True),
    (b"x 1:N:0:A", b"x 2:N:0:A", True),
    (b"same", b"same", True),
    (b"", b"", True),
    (b"/1", b"/2", True),
    (b"x/1", b"x", False),
    (b"x/2", b"x/1", False),
    (b"abc", b"abcd", False),  # one id a proper prefix of the other
    (b"abcd", b"abc", False),
    (b"abc/1", b"abcd/2", False),
    (X[:63] + b"a" + X[:5], X[:63] + b"b" + X[:5], False),  # the first difference at byte 63, 64, 65
    (X[:64] + b"a", X[:64] + b"b", False),
    (X[:65] + b"a", X[:65] + b"b", False),
    (X[:63] + b"a", X[:63] + b"a", True),
    (X[:64] + b"/1", X[:64] + b"/2", True),
    (X[:63] + b"/1", X[:63] + b"/2", True),  # the strip across a 64-byte step
    (X[:62] + b"/1", X[:62] + b"/2", True),
    (b"x\t1", b"x\t2", True),  # a tab as the cut
    (b"x\tq", b"x y", True),
    (b"x/1\tq", b"x/2 y", True),
    (b"x/1", b"x/1", True),  # identical names agree whatever they end in
    (b"x/2", b"x/2", True),
    (b"x /1", b"x /2", True),
    (b" a", b" b", True),  # two empty ids
    (b"a/1", b"b/2", False),
    (b"1", b"2", False),
]


def test_the_rule_by_hand():
    for a, b, agree in RULE:
        assert pl.mates_agree(a, b) is agree, (a, b)
    assert pl.first_bad_pair([r[0] for r in RULE], [r[1] for r in RULE]) == 5
    assert pl.first_bad_pair([b"a", b"b"], [b"a", b"b"]) is None


def test_the_checker_weaves_and_splits():
    t1 = nl.make_fastq([b"a/1", b"b/1"], [b"AC", b"G"], last_newline=False)
    t2 = nl.make_fastq([b"a/2", b"b/2"], [b"T", b"TTT"], eol=b"\r\n")
    w = pl.weave(t1, t2)
    assert w == b"@a/1\nAC\n+\nII\n@a/2\r\nT\r\n+\r\nI\r\n@b/1\nG\n+\nI\n@b/2\r\nTTT\r\n+\r\nIII\r\n"
    assert pl.split(w, 4) == (t1 + b"\n", t2)
    with pytest.raises(AssertionError):
        pl.weave(t1, t2 + t2)
    with pytest.raises(AssertionError):
        pl.split(t2 + t2[:t2.index(b"@b")], 4)


# ---- pair_core.h on the CPU -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_cpu") / "pair_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "pair_cpu", "pair_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _core(exe, tmp_path, t1, t2, n_pairs):
    """-> (weave status, check status, woven text, part 1, part 2)"""
    (tmp_path / "in.bin").write_bytes(struct.pack("<QQ", n_pairs, len(t1)) + t1 + struct.pack("<Q", len(t2)) + t2)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    out = (tmp_path / "out.bin").read_bytes()
    weave = struct.unpack_from("<Q", out, 0)[0]
    if weave != OK:
        assert len(out) == 8
        return weave, None, None, None, None
    check, n = struct.unpack_from("<QQ", out, 8)
    woven = out[24:24 + n]
    first = struct.unpack_from("<Q", out, 24 + n)[0]
    text = out[32 + n:]
    assert len(text) == n
    return weave, check, woven, text[:first], text[first:]


def _sides(rng, n):
    ids = [b"r%d" % p + bytes(rng.integers(65, 91, int(rng.integers(0, 140)), dtype=np.uint8)) for p in range(n)]
    out = []
    for k in (b"1", b"2"):
        reads = [bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 200))).astype(np.uint8)) for _ in range(n)]
        names = [i + (b"/" + k if p % 2 else b" " + k + b":N:0") for p, i in enumerate(ids)]
        out.append((names, reads))
    return out


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"])
@pytest.mark.parametrize("last1", [True, False])
@pytest.mark.parametrize("last2", [True, False])
def test_core_weaves_checks_and_splits(core_exe, tmp_path, eol, last1, last2):
    rng = np.random.default_rng(1)
    s1, s2 = _sides(rng, 131)
    t1 = nl.make_fastq(*s1, eol=eol, last_newline=last1)
    t2 = nl.make_fastq(*s2, eol=eol, last_newline=last2)
    weave, check, woven, p1, p2 = _core(core_exe, tmp_path, t1, t2, 131)
    assert (weave, check) == (OK, OK)
    assert woven == pl.weave(t1, t2)
    assert (p1, p2) == pl.split(woven, 4)
    assert nl.names_of(woven) == [n for pair in zip(s1[0], s2[0]) for n in pair]


def test_core_on_the_rule_cases(core_exe, tmp_path):
    reads = [b"ACGT"] * len(RULE)
    for eol in (b"\n", b"\r\n"):
        t1 = nl.make_fastq([r[0] for r in RULE], reads, eol=eol)
        t2 = nl.make_fastq([r[1] for r in RULE], reads, eol=eol)
        _, check, woven, _, _ = _core(core_exe, tmp_path, t1, t2, len(RULE))
        assert check == (2 * 5) << 8 | FORMAT and woven == pl.weave(t1, t2)
    for i, (a, b, agree) in enumerate(RULE):  # each case alone, behind good pairs
        n1, n2 = [b"ok/1"] * 3 + [a], [b"ok/2"] * 3 + [b]
        t1, t2 = nl.make_fastq(n1, reads[:4]), nl.make_fastq(n2, reads[:4], last_newline=False)
        _, check, _, _, _ = _core(core_exe, tmp_path, t1, t2, 4)
        assert check == (OK if agree else (2 * 3) << 8 | FORMAT), (a, b)
        assert (pl.first_bad_pair(n1, n2) is None) is agree


def test_core_small_counts(core_exe, tmp_path):
    assert _core(core_exe, tmp_path, b"", b"", 0) == (OK, OK, b"", b"", b"")
    t1, t2 = b"@\nA\n+\nI\n", b"@\nC\n+\nJ"
    assert _core(core_exe, tmp_path, t1, t2, 1) == (OK, OK, t1 + t2 + b"\n", t1, t2 + b"\n")


@pytest.mark.parametrize("case", ["one_fewer", "one_more", "three_lines", "three_lines_no_newline", "text_1", "zero_pairs",
                                  "one_empty", "newlines_only"])
def test_core_refuses_other_record_counts(core_exe, tmp_path, case):
    rng = np.random.default_rng(2)
    s1, s2 = _sides(rng, 9)
    t1, t2 = nl.make_fastq(*s1), nl.make_fastq(*s2)
    recs, n = pl._records(t2, 4), 9
    if case == "one_fewer":
        t2, bad = b"".join(recs[:-1]), 2 * 8 + 1
    elif case == "one_more":
        t2, bad = t2 + recs[0], 2 * 8 + 1
    elif case == "three_lines":
        t2, bad = t2[:t2.rindex(b"\n", 0, len(t2) - 1) + 1], 2 * 8 + 1
    elif case == "three_lines_no_newline":
        t2, bad = t2[:t2.rindex(b"\n", 0, len(t2) - 1)], 2 * 8 + 1
    elif case == "text_1":
        t1, bad = b"".join(pl._records(t1, 4)[:4]), 2 * 4
    elif case == "zero_pairs":
        n, bad = 0, 0
    elif case == "one_empty":
        t2, bad = b"", 1
    else:
        t1, bad = b"\n" * 100, 2 * 8
    weave = _core(core_exe, tmp_path, t1, t2, n)[0]
    assert weave == bad << 8 | FORMAT


# ---- the C, Python and command-line surface ---------------------------------------------------------
def test_c99_consumer_pins_the_new_structs(tmp_path):
    exe = str(tmp_path / "abi_pairs")
    libdir = os.path.join(REPO, "ntcomp_amd")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "abi_pairs.c"), "-o", exe, "-L", libdir, "-lntcomp_gpu", "-Wl,-rpath," + libdir]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert '"ntc_file_opts4": 96' in r.stdout and '"ntc_p_stats": 32' in r.stdout
    import ctypes
    assert ctypes.sizeof(nt.FileOpts4) == 96 and ctypes.sizeof(nt.PStats) == 32


def test_the_new_symbols_are_declared_and_exported():
    heads = "".join(open(os.path.join(REPO, "include", h)).read() for h in ("ntcomp_codec.h", "ntcomp_pipeline.h"))
    L = nt.lib()
    for sym in ("ntc_encode_pack_fastq_paired", "ntc_decode_pair_split", "ntc_encode_file_ex4", "ntc_decode_file_ex4"):
        assert sym + "(" in heads and sym in nt.EXPORTED and hasattr(L, sym)
    assert nt.PAIR_MODES == {"off": 0, "ids": 1, "nocheck": 2}
    assert isinstance(nt.GpuContext.paired, property) and callable(nt.GpuContext.encode_pack_fastq_paired)


def test_without_the_gpu_stage_pairs_are_unsupported(tmp_path):
    """pipeline.cpp linked over the GPU stub (no capi.cpp): the hook table is null"""
    san, csrc = os.path.join(REPO, "tests", "san"), os.path.join(REPO, "ntcomp_amd", "csrc")
    subprocess.run(["gcc", "-O1", "-c", os.path.join(REPO, "oracle", "ntcomp_oracle.c"), "-o", str(tmp_path / "orc.o")],
                   check=True, capture_output=True, text=True)
    exe = str(tmp_path / "pair_hooks")
    srcs = [os.path.join(csrc, f + ".cpp") for f in ("fastx", "pgzip", "block_codec", "index_io", "sbwt_build", "pipeline")]
    cmd = ["g++", "-O0", "-std=c++17", "-I" + os.path.join(san, "stub_include"), "-I" + os.path.join(REPO, "include"), "-pthread",
           *srcs, os.path.join(san, "gpu_stub.cpp"), os.path.join(REPO, "tests", "pair_cpu", "pair_hooks.cpp"),
           str(tmp_path / "orc.o"), "-o", exe, "-lz", "-ldl"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe, str(tmp_path / "none.fq")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mode 1: encode 10 decode 10" in r.stdout and "short struct: 1" in r.stdout


REFUSED = [
    ["encode", "-i", "idx", "--mate-file", "r2.fq", "--interleaved", "r1.fq"],
    ["encode", "-i", "idx", "--mate-check", "ids", "r1.fq"],
    ["encode", "-i", "idx", "--mate-check", "off", "r1.fq"],
    ["encode", "-i", "idx", "--mate-file", "r2.fq", "--host-parse", "r1.fq"],
    ["encode", "-i", "idx", "--interleaved", "--host-parse", "r1.fq"],
    ["encode", "-i", "idx", "--interleaved", "--mate-check", "names", "r1.fq"],
    ["verify", "-i", "idx", "--digest-file", "d.ntcd", "--mate-out", "r2.out", "enc.dat"],
]


@pytest.mark.parametrize("cli", ["python", "native"])
def test_both_command_lines_refuse_with_status_2(tmp_path, cli):
    """before anything is loaded or written: no index, input or GPU is there to be touched"""
    head = [sys.executable, "-m", "ntcomp_amd"] if cli == "python" else [NATIVE]
    env = dict(os.environ, PYTHONPATH=REPO)
    for args in REFUSED:
        r = subprocess.run(head + args, capture_output=True, cwd=tmp_path, env=env, timeout=120)
        assert r.returncode == 2, (args, r.stderr[-300:])
        assert not os.listdir(tmp_path)
