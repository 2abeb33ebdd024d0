"""`decode --bgzf` through the file pipeline (ntc_decode_file_ex7) and both command lines: the output
is a BGZF file whose members inflate to the bytes of plain `decode`, ends with the EOF member only
when the decode succeeded, and goes back through `encode --inflate gpu` to the archive it came from."""
import ctypes
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bgzf_lib as bl
import ntcomp_amd as nt

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
K = 31
SIDE = (("--exceptions", ".ntcx"), ("--quality-file", ".ntcq"), ("--name-file", ".ntcn"), ("--digest-file", ".ntcd"))
N_READS = 2 * 65536 + 1000


def _cli(which, args, stdout=None):
    head = [sys.executable, "-m", "ntcomp_amd"] if which == "python" else [NATIVE]
    return subprocess.run(head + [str(a) for a in args], stdout=stdout or subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, PYTHONPATH=REPO), timeout=300)


def _encode(idx, src, out, *extra):
    """-> [the archive, the four side files]"""
    args = ["encode", "-i", idx, "--non-acgt", "keep", "--qualities", "keep", "--names", "keep", *extra]
    for flag, ext in SIDE:
        args += [flag, str(out) + ext]
    with open(out, "wb") as f:
        r = _cli("native", args + [src], stdout=f)
    assert r.returncode == 0, r.stderr[-2000:]
    return [open(out, "rb").read()] + [open(str(out) + ext, "rb").read() for _, ext in SIDE]


def _sides(arch, digest=True):
    return [x for flag, ext in SIDE if digest or ext != ".ntcd" for x in (flag, str(arch) + ext)]


def _decode(which, pipe, out, *extra, sides=True, ok=True):
    """decode the fixture's archive into `out` -> (its bytes, the --stats line, the exit status)"""
    args = ["decode", "-i", pipe["idx"], "--stats", *extra] + (_sides(pipe["arch"]) if sides else [])
    with open(out, "wb") as f:
        r = _cli(which, args + [pipe["arch"]], stdout=f)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stderr.decode().strip().splitlines()
    return open(out, "rb").read(), (json.loads(lines[-1]) if ok else lines), r.returncode


def check_bgzf(blob, plain, st=None):
    """a BGZF file: members, the EOF member last, the plain text inside; -> the members before the EOF"""
    assert blob.endswith(bl.EOF)
    members = bl.parse(blob)
    assert members[-1][3] == 0 and all(isize > 0 for _, _, _, isize in members[:-1])
    assert gzip.decompress(blob) == plain
    at = 0
    for _, _, _, isize in members[:-1]:  # every member starts on a record's header line
        assert (at == 0 or plain[at - 1:at] == b"\n") and plain[at:at + 1] in (b">", b"@")
        at += isize
    if st is not None:
        assert st["bgzf"] is True and st["bgzf_members"] == len(members) - 1
        assert st["bgzf_text_bytes"] == len(plain) and st["bgzf_bytes"] == len(blob) - len(bl.EOF)
        n_chunks = sum(len(bl.chunks(isize)) for _, _, _, isize in members[:-1])
        assert st["bgzf_chunks_stored"] + st["bgzf_chunks_huffman"] + st["bgzf_chunks_matches"] == n_chunks
        assert st["bgzf_s"] >= 0
    return members[:-1]


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """an index at k = 31; a FASTQ of two full blocks and 1,000 reads of 40-60 bases, some with an
    N; its archive with all side files; and the plain decodes the tests compare against"""
    d = tmp_path_factory.mktemp("bgzfpipe")
    genome = nt.synth_genome(12, 300_000)
    nt.Index.build([genome.tobytes()], K).save(str(d / "idx"))
    n = N_READS
    flat = bytearray(nt.synth_reads(genome, 21, 0, n, 60, 10_000).tobytes())
    rng = np.random.default_rng(5)
    for p in rng.integers(0, len(flat), 300):
        flat[p] = ord("N")
    lens = rng.integers(40, 61, n)
    quals = rng.choice(np.frombuffer(b"FFFF:,#", np.uint8), 60 * n).tobytes()
    recs = [b"@r%d/%d x\n%s\n+\n%s\n" % (i, 1 + i % 2, bytes(flat[60 * i:60 * i + int(lens[i])]), quals[60 * i:60 * i + int(lens[i])])
            for i in range(n)]
    text = b"".join(recs)
    (d / "r.fq").write_bytes(text)
    p = {"d": d, "idx": str(d / "idx"), "text": text, "recs": recs, "arch": str(d / "a.dat")}
    p["files"] = _encode(p["idx"], d / "r.fq", d / "a.dat")
    p["fastq"], st, _ = _decode("native", p, d / "plain.fq")
    assert p["fastq"] == text and st["bgzf"] is False and st["bgzf_members"] == 0
    p["fasta"], _, _ = _decode("native", p, d / "plain.fa", sides=False)
    assert p["fasta"].count(b">seq.") == n
    return p


@pytest.mark.parametrize("which", ["native", "python"])
def test_both_command_lines(pipe, which):
    d = pipe["d"]
    blob, st, _ = _decode(which, pipe, d / (which + ".fq.gz"), "--bgzf")
    members = check_bgzf(blob, pipe["fastq"], st)
    assert len(members) >= len(pipe["text"]) // bl.M and len(blob) < len(pipe["text"]) // 2
    fa, st, _ = _decode(which, pipe, d / (which + ".fa.gz"), "--bgzf", sides=False)
    check_bgzf(fa, pipe["fasta"], st)
    if which == "python":  # the same bytes from both
        assert blob == open(d / "native.fq.gz", "rb").read() and fa == open(d / "native.fa.gz", "rb").read()


def test_batches_contexts_and_threads(pipe):
    """members never span a batch: one block per batch gives other members and the same text; for a
    given batch size the bytes do not depend on the contexts or threads"""
    d = pipe["d"]
    ref = open(d / "native.fq.gz", "rb").read() if os.path.exists(d / "native.fq.gz") else _decode("native", pipe, d / "ref.fq.gz", "--bgzf")[0]
    one, st, _ = _decode("native", pipe, d / "bpb1.fq.gz", "--bgzf", "--blocks-per-batch", "1")
    members = check_bgzf(one, pipe["fastq"], st)
    ends, at = set(), 0
    for _, _, _, isize in members:
        at += isize
        ends.add(at)
    for k in (65536, 2 * 65536):  # a member ends where a block's text ends
        assert len(b"".join(pipe["recs"][:k])) in ends
    two, st, _ = _decode("native", pipe, d / "two.fq.gz", "--bgzf", "--devices", "0,0", "--threads", "3")
    assert two == ref and st["gpus"] == 2
    two1, _, _ = _decode("native", pipe, d / "two1.fq.gz", "--bgzf", "--devices", "0,0", "--blocks-per-batch", "1")
    assert two1 == one


def test_mate_out(pipe):
    d = pipe["d"]
    p1, _, _ = _decode("native", pipe, d / "m1.fq", "--mate-out", d / "m2.fq")
    p2 = open(d / "m2.fq", "rb").read()
    assert p1 == b"".join(pipe["recs"][0::2]) and p2 == b"".join(pipe["recs"][1::2])
    for which in ("native", "python"):
        z1, st, _ = _decode(which, pipe, d / "m1.fq.gz", "--bgzf", "--mate-out", d / "m2.fq.gz")
        z2 = open(d / "m2.fq.gz", "rb").read()
        m1, m2 = check_bgzf(z1, p1), check_bgzf(z2, p2)
        assert st["bgzf_members"] == len(m1) + len(m2) and st["bgzf_text_bytes"] == len(p1) + len(p2)
        assert st["mate1_bytes"] == len(z1) and st["mate2_bytes"] == len(z2) and st["pairs"] == N_READS // 2


def test_reads_inside_one_block(pipe):
    d = pipe["d"]
    for spec, a, b in (("70001-70900", 70000, 70900), ("131073-", 131072, N_READS)):
        plain, _, _ = _decode("native", pipe, d / "range.fq", "--reads", spec)
        assert plain == b"".join(pipe["recs"][a:b])
        for which in ("native", "python"):
            blob, st, _ = _decode(which, pipe, d / "range.fq.gz", "--bgzf", "--reads", spec)
            check_bgzf(blob, plain, st)
            assert st["r_reads_written"] == b - a


def test_three_shards_concatenate(pipe):
    d = pipe["d"]
    parts = [_decode("native" if i != 2 else "python", pipe, d / ("shard%d.fq.gz" % i), "--bgzf", "--shard", "%d/3" % i)[0]
             for i in (1, 2, 3)]
    assert all(p.endswith(bl.EOF) for p in parts)
    whole = b"".join(parts)
    assert gzip.decompress(whole) == pipe["fastq"]
    members = bl.parse(whole)
    assert sum(1 for _, _, _, isize in members if isize == 0) == 3  # the EOF members in the middle are empty members
    found = nt.bgzf_members(whole)
    assert len(found) == len(members)
    # more shards than blocks (slice 1 of 4 holds none of the 3): the empty slice is an EOF member alone
    for which in ("native", "python"):
        r = _cli(which, ["decode", "-i", pipe["idx"], "--bgzf", "--shard", "1/4", *_sides(pipe["arch"]), pipe["arch"]])
        assert r.returncode == 0 and r.stdout == bl.EOF


def test_round_trip_through_inflate_gpu(pipe):
    """the lossless decode --bgzf output is an input `encode --inflate gpu` takes: back come the archive
    and every side file, byte for byte"""
    d = pipe["d"]
    src = d / "native.fq.gz"
    if not os.path.exists(src):
        _decode("native", pipe, src, "--bgzf")
    again = _encode(pipe["idx"], src, d / "again.dat", "--inflate", "gpu")
    assert again == pipe["files"]


def test_a_failed_decode_leaves_no_eof_member(pipe):
    """the digest file of another run (its last read differs): the decode fails, and the output
    holds the batches before the mismatch but not the EOF member -- a truncated BGZF file"""
    d = pipe["d"]
    last = bytearray(pipe["recs"][-1])
    seq_at = last.index(b"\n") + 1
    last[seq_at] = ord("A") if last[seq_at] != ord("A") else ord("C")
    (d / "other.fq").write_bytes(b"".join(pipe["recs"][:-1]) + bytes(last))
    _encode(pipe["idx"], d / "other.fq", d / "other.dat")
    sides = _sides(pipe["arch"], digest=False) + ["--digest-file", str(d / "other.dat") + ".ntcd"]
    for which in ("native", "python"):
        out = d / ("failed-%s.fq.gz" % which)
        with open(out, "wb") as f:
            r = _cli(which, ["decode", "-i", pipe["idx"], "--bgzf", "--blocks-per-batch", "1", *sides, pipe["arch"]], stdout=f)
        blob = open(out, "rb").read()
        assert r.returncode != 0 and b"digest" in r.stderr.lower(), r.stderr[-500:]
        assert not blob.endswith(bl.EOF)
        members = bl.parse(blob)  # whole members all the same
        assert all(isize > 0 for _, _, _, isize in members)
        assert pipe["fastq"].startswith(gzip.decompress(blob + bl.EOF))


def test_verify_refuses_bgzf(pipe):
    for which in ("native", "python"):
        r = _cli(which, ["verify", "-i", pipe["idx"], "--bgzf", *_sides(pipe["arch"]), pipe["arch"]],
                 stdout=subprocess.PIPE)
        assert r.returncode == 2 and b"--bgzf" in r.stderr and r.stdout == b""


def test_library_surface(pipe):
    """nt.decode_file(out_format="bgzf"): the "z" stats; out_fd -1 wins; refusals"""
    d = pipe["d"]
    ix = nt.Index.load(pipe["idx"])
    ctx = nt.GpuContext(0)
    try:
        ctx.upload(ix)
        side = dict(nx_path=pipe["arch"] + ".ntcx", q_path=pipe["arch"] + ".ntcq", n_path=pipe["arch"] + ".ntcn")
        with open(d / "lib.fq.gz", "wb") as f:
            st = nt.decode_file([ctx], pipe["arch"], f.fileno(), out_format="bgzf", **side)
        blob = open(d / "lib.fq.gz", "rb").read()
        members = check_bgzf(blob, pipe["fastq"])
        z = st["z"]
        assert z["out_format"] == 1 and z["members"] == len(members) and z["text_bytes"] == len(pipe["fastq"])
        assert z["bytes"] == len(blob) - 28 == st["bytes_out"] - 28 and z["seconds"] > 0
        assert not ctx.bgzf_text  # the option is the call's
        st = nt.decode_file([ctx], pipe["arch"], -1, out_format="bgzf", d_path=pipe["arch"] + ".ntcd", **side)
        assert st["z"]["members"] == 0 and st["reads"] == N_READS  # nothing is compressed under out_fd -1
        fo = nt.FileOpts7(ctypes.sizeof(nt.FileOpts7), 0, -1, 0, -1, None, None, 0, -1, None, 0, -1, None, 0, None, -1, 0, 0, 0, 0, 2, 0)
        arr = (ctypes.c_void_p * 1)(ctx.h.value)
        o, ps = nt.PipelineOpts(0, 2, 0, 0, 0), nt.PipelineStats()
        call = lambda: nt.lib().ntc_decode_file_ex7(arr, 1, os.fsencode(pipe["arch"]), 1, ctypes.byref(fo), ctypes.byref(o),
                                                    ctypes.byref(ps), None, None, None, None)
        assert call() == 1  # out_format 2
        fo.out_format, fo.reserved2 = 1, 1
        assert call() == 1
    finally:
        ctx.close()
