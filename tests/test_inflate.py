"""`--inflate gpu` without a GPU: the host restatement of the device's inflate decoder
(inflate_core.h) through ntc_inflate_members with no context, and the same header compiled alone
under ASan + UBSan (tests/inflate_cpu).  The checker is Python's zlib, which verifies the gzip
header, CRC-32 and ISIZE."""
import ctypes
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import ntcomp_amd as nt
import inflate_lib as il

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
INVALID_ARG = 1


run_all = il.run_all


def test_constants_match_the_headers():
    src = open(os.path.join(REPO, "ntcomp_amd", "csrc", "inflate_core.h")).read()
    assert "kInfMaxOut = %d;" % il.MAX_OUT in src
    for v, name in enumerate(il.STATUS_NAMES):
        assert "%s = %d," % (name, v) in src, name
    hdr = open(os.path.join(REPO, "include", "ntcomp_codec.h")).read()
    assert "#define NTC_INFLATE_MAX_OUT %du" % il.MAX_OUT in hdr
    assert nt.INFLATE_MAX_OUT == il.MAX_OUT and sorted(nt.INFLATE_STATUS) == list(range(10))
    assert nt.INFLATE_MEMBER.itemsize == 24 and nt.INFLATE_RESULT.itemsize == 16
    for sym in ("ntc_inflate_members", "ntc_inflate_members_device"):
        assert sym + "(" in hdr and sym in nt.EXPORTED and hasattr(nt.lib(), sym)


def test_the_corpus_is_what_the_issue_lists():
    names = [n for n, _, _ in il.sound()]
    sizes = {len(d) for _, _, d in il.sound()}
    assert {0, 1, 2, 3, 257, 258, 259, 65279, 65280, 65535, 65536} <= sizes
    for k in il.KINDS:
        for suffix in ["l0", "l1", "l6", "l9", "fixed", "huffman", "rle", "filtered"]:
            assert "%s-%s" % (k, suffix) in names
    for n, m, d in il.all_sound():
        ok, data = il.zlib_accepts(m)
        assert ok and data == d, n
    assert il.EOF_MEMBER in [m for _, m, _ in il.sound()]
    for n, m, c, st in il.damaged():
        assert st != 0
        ok, data = il.zlib_accepts(m)
        assert not ok or len(data) != c or c > il.MAX_OUT, n  # zlib refuses it, or the caller's size is what is wrong


def test_sound_members_give_zlibs_bytes():
    cs = il.all_sound()
    outs, res = run_all(None, [m for _, m, _ in cs], [len(d) for _, _, d in cs])
    for (name, m, d), o, r in zip(cs, outs, res):
        assert r["status"] == 0, (name, nt.INFLATE_STATUS[int(r["status"])])
        assert o == d and r["crc"] == zlib.crc32(d) and r["out_bytes"] == len(d), name


def test_each_member_alone_and_packed_tightly():
    """calls of one member; and bgzf_members' triples, the outputs back to back"""
    cs = il.all_sound()
    for name, m, d in cs[::7]:
        out, res = nt.inflate_members(None, m, [(0, len(m), len(d), 0)])
        assert res[0]["status"] == 0 and out.tobytes() == d, name
    bg = [(n, m, d) for n, m, d in cs if nt.bgzf_members(m) == [(0, len(m), len(d))]]
    assert len(bg) > 60
    blob = b"".join(m for _, m, _ in bg)
    listed = nt.bgzf_members(blob + b"\x1f\x8b\x08\x00 not bgzf")
    assert [(s, z) for _, s, z in listed] == [(len(m), len(d)) for _, m, d in bg]
    out, res = nt.inflate_members(None, blob, listed)
    assert (res["status"] == 0).all() and out.tobytes() == b"".join(d for _, _, d in bg)


def test_bgzf_members_stops_at_what_is_no_member():
    text = il.fastq_text(3000)
    a = il.bgzf(il.raw_deflate(text), text)
    assert nt.bgzf_members(b"") == [] and nt.bgzf_members(a[:17]) == []
    assert nt.bgzf_members(a + a[:-1]) == [(0, len(a), 3000)]  # the second one is cut short
    assert nt.bgzf_members(a + il.EOF_MEMBER) == [(0, len(a), 3000), (len(a), 28, 0)]
    assert nt.bgzf_members(il.gzip_member(il.raw_deflate(text), text)) == []
    assert nt.bgzf_members(il.gzip_member(il.raw_deflate(text), text, extra=b"AB\x01\0z")) == []
    two = il.gzip_member(il.raw_deflate(text), text, extra=b"AB\x01\0z" + b"BC\x02\0" + struct.pack("<H", 12 + 11 + len(il.raw_deflate(text)) + 8 - 1))
    assert nt.bgzf_members(two) == [(0, len(two), 3000)]  # the BC subfield need not come first


def test_damaged_members_get_their_status():
    cs = il.damaged()
    outs, res = run_all(None, [m for _, m, _, _ in cs], [c for _, _, c, _ in cs])
    for (name, m, c, st), o, r in zip(cs, outs, res):
        assert r["status"] == st, (name, nt.INFLATE_STATUS[int(r["status"])], "expected", nt.INFLATE_STATUS[st])
        assert o is None


def test_a_call_that_mixes_sound_and_damaged_members():
    """every sound neighbour is exact, nothing else of the output is touched (run_all checks the
    bytes between and inside the failed slots), and the order of the members does not matter"""
    good, bad = il.all_sound(), il.damaged()
    members, claimed, want = [], [], []
    for i in range(max(len(good), len(bad))):
        g, b = good[i % len(good)], bad[i % len(bad)]
        members += [g[1], b[1]]
        claimed += [len(g[2]), b[2]]
        want += [(0, g[2]), (b[3], None)]
    outs, res = run_all(None, members, claimed)
    for i, ((st, d), o, r) in enumerate(zip(want, outs, res)):
        assert r["status"] == st and o == d, i
    outs2, res2 = run_all(None, members[::-1], claimed[::-1])
    assert outs2[::-1] == outs and (res2[::-1] == res).all()


def test_argument_refusals():
    L = nt.lib()
    text = il.fastq_text(1000)
    mem = il.bgzf(il.raw_deflate(text), text)
    blob = np.frombuffer(mem + mem, dtype=np.uint8)
    out = np.zeros(4096, dtype=np.uint8)
    res = np.zeros(4, dtype=nt.INFLATE_RESULT)
    bad = ctypes.c_uint64(77)

    def call(descs, comp_bytes=len(blob), cap=len(out)):
        m = np.array(descs, dtype=nt.INFLATE_MEMBER)
        return L.ntc_inflate_members(None, blob.ctypes.data_as(ctypes.c_void_p), comp_bytes, m.ctypes.data_as(ctypes.c_void_p),
                                     len(m), out.ctypes.data_as(ctypes.c_void_p), cap, res.ctypes.data_as(ctypes.c_void_p),
                                     ctypes.byref(bad))

    n = len(mem)
    assert call([(0, n, 1000, 0), (n, n, 1000, 1000)]) == 0 and bad.value == 0 and out[:2000].tobytes() == text + text
    out[:] = 0
    for descs, kw in [
        ([(0, n, 1000, 0), (n, n, 1000, 999)], {}),           # the outputs overlap by a byte
        ([(0, n, 1000, 500), (n, n, 1000, 0)], {}),           # the same, in the other order
        ([(0, n, 1000, 0), (n, n, 1000, 0)], {}),             # the same place
        ([(0, n, 1000, 0), (n, n + 1, 1000, 1000)], {}),      # past the compressed bytes
        ([(2 * n + 1, 0, 0, 0)], {}),
        ([(1 << 63, n, 1000, 0)], {}),
        ([(0, n, 1000, 4096 - 999)], {}),                     # past the output
        ([(0, n, 1000, 1 << 63)], {}),
        ([(0, n, 70000, 0)], {}),                             # too large, but its place must exist all the same
        ([(0, n, 1000, 0)], {"cap": 999}),
        ([(0, n, 1000, 0)], {"comp_bytes": n - 1}),
    ]:
        assert call(descs, **kw) == INVALID_ARG, descs
    assert not out.any()  # nothing ran
    assert L.ntc_inflate_members(None, None, 0, None, 1, None, 0, None, ctypes.byref(bad)) == INVALID_ARG
    assert L.ntc_inflate_members(None, None, 0, None, 0, None, 0, None, None) == INVALID_ARG
    assert L.ntc_inflate_members(None, None, 0, None, 0, None, 0, None, ctypes.byref(bad)) == 0 and bad.value == 0
    assert L.ntc_inflate_members_device(None, None, 0, None, 0, None, 0, None, ctypes.byref(bad)) == INVALID_ARG
    # empty outputs overlap nothing, and a too-large member with room is a status, not a refusal
    big = np.zeros(80000, dtype=np.uint8)
    o, r = nt.inflate_members(None, il.EOF_MEMBER + mem, [(0, 28, 0, 500), (28, n, 1000, 0), (0, 28, 0, 500), (28, n, 70000, 2000)], out=big)
    assert list(r["status"]) == [0, 0, 0, il.TOO_LARGE] and o[:1000].tobytes() == text and not o[1000:].any()


def test_mutation_sweep():
    """about 2,000 seeded single-bit and single-byte changes: status 0 exactly where zlib takes the
    member whole, and then with zlib's bytes"""
    ms = il.mutants()
    assert 1900 <= len(ms) <= 2100 and len({m for _, m in ms}) > 1800
    claimed = [il.claimed_of(m) for _, m in ms]
    outs, res = run_all(None, [m for _, m in ms], claimed)
    accepted = 0
    for (name, m), c, o, r in zip(ms, claimed, outs, res):
        ok, data = il.zlib_accepts(m)
        if r["status"] == 0:
            assert ok and o == data, name
        if ok and len(data) <= il.MAX_OUT:
            assert r["status"] == 0, (name, nt.INFLATE_STATUS[int(r["status"])])
            accepted += 1
    kinds = {int(s) for s in res["status"]}
    print("mutants %d, accepted %d, statuses %s" % (len(ms), accepted, sorted(kinds)))
    assert accepted >= 20 and {il.BAD_HEADER, il.BAD_CODE, il.CRC, il.INPUT} <= kinds


# ---- the header alone, under ASan + UBSan -------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate_cpu") / "inflate_cpu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "inflate_cpu", "inflate_cpu.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_stand_alone_program_over_the_corpus_and_the_mutants(cpu_exe, tmp_path):
    """where the bounds are proven: every member is decoded from a buffer of exactly its bytes into
    one of exactly the claimed size, and the results are the library's"""
    cases = [(n, m, len(d)) for n, m, d in il.all_sound()] + [(n, m, c) for n, m, c, _ in il.damaged()] \
        + [(n, m, il.claimed_of(m)) for n, m in il.mutants()]
    (tmp_path / "in.bin").write_bytes(b"".join(struct.pack("<II", len(m), c) + m for _, m, c in cases))
    r = subprocess.run([cpu_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-3000:]
    assert r.stdout.split()[0] == b"%d" % len(cases)
    outs, res = run_all(None, [m for _, m, _ in cases], [c for _, _, c in cases])
    data, at = (tmp_path / "out.bin").read_bytes(), 0
    for (name, m, c), o, rr in zip(cases, outs, res):
        st, nb, crc = struct.unpack_from("<III", data, at)
        at += 12
        assert (st, nb, crc) == (rr["status"], rr["out_bytes"], rr["crc"]), name
        if st == 0:
            assert data[at:at + nb] == o, name
            at += nb
    assert at == len(data)


# ---- the command lines' refusals: before an index is read or a GPU opened ---------------------------
@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_refusals_exit_with_2(which, tmp_path):
    text = il.fastq_text(4000)
    (tmp_path / "r.fq.gz").write_bytes(il.bgzf(il.raw_deflate(text), text) + il.EOF_MEMBER)
    (tmp_path / "plain.fq.gz").write_bytes(il.gzip_member(il.raw_deflate(text), text))
    (tmp_path / "r.fq").write_bytes(text)
    head = [sys.executable, "-m", "ntcomp_amd"] if which == "python" else [NATIVE]
    env = dict(os.environ, PYTHONPATH=REPO, HIP_VISIBLE_DEVICES="-1")

    def run(*args):
        r = subprocess.run(head + ["encode", "-i", str(tmp_path / "none")] + [str(a) for a in args], capture_output=True, env=env,
                           timeout=120)
        return r.returncode, r.stderr

    bg = tmp_path / "r.fq.gz"
    for args, word in (
        (["--inflate", "gpx", bg], b"--inflate"),                                   # a misspelt engine
        (["--inflate", "gpu", "--host-parse", bg], b"--host-parse"),
        (["--inflate", "gpu", tmp_path / "plain.fq.gz"], b"plain.fq.gz does not start with a BGZF member"),
        (["--inflate", "gpu", tmp_path / "r.fq"], b"r.fq does not start with a BGZF member"),
        (["--inflate", "gpu", "--mate-file", tmp_path / "plain.fq.gz", bg], b"plain.fq.gz does not start with a BGZF member"),
        (["--inflate", "gpu", "--mate-file", bg, tmp_path / "r.fq"], b"r.fq does not start with a BGZF member"),
    ):
        rc, err = run(*args)
        assert rc == 2 and word in err, (args, rc, err[-300:])
    # a sound request gets past the checks and fails on the index that is not there: not with 2
    rc, err = run("--inflate", "gpu", bg)
    assert rc not in (0, 2) and b"BGZF" not in err, err[-300:]


def test_the_pipeline_surface():
    hdr = open(os.path.join(REPO, "include", "ntcomp_pipeline.h")).read()
    assert "ntc_encode_file_ex6(" in hdr and "ntc_encode_file_ex6" in nt.EXPORTED and hasattr(nt.lib(), "ntc_encode_file_ex6")
    assert nt.INFLATE_ENGINES == {"host": 0, "gpu": 1} and "#define NTC_INFLATE_GPU 1" in hdr
    assert ctypes.sizeof(nt.FileOpts6) == ctypes.sizeof(nt.FileOpts5) + 8 and ctypes.sizeof(nt.IStats) == 48
    assert [n for n, _ in nt.FileOpts6._fields_][:-2] == [n for n, _ in nt.FileOpts5._fields_]
    import inspect
    assert "inflate" in inspect.signature(nt.encode_file).parameters
    L = nt.lib()
    assert L.ntc_encode_file_ex6(None, 0, b"x", 1, None, None, None, None, None, None, None, None, None) == INVALID_ARG
    fo = nt.FileOpts6(ctypes.sizeof(nt.FileOpts5), 0, -1, 0, -1, None, None, 0, -1, None, 0, -1, None, 0, None, -1, 0, 0, 1, 0)
    assert L.ntc_encode_file_ex6(None, 0, b"x", 1, ctypes.byref(fo), None, None, None, None, None, None, None, None) == INVALID_ARG
