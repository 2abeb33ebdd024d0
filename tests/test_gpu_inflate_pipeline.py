"""`encode --inflate gpu` through the file pipeline and both command lines: a BGZF input whose
runs of members are inflated on the GPU gives byte for byte the archive and the side files of
`--inflate host`, and of the plain text."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ntcomp_amd as nt
import inflate_lib as il

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
K = 31
SIDE = (("--exceptions", ".ntcx"), ("--quality-file", ".ntcq"), ("--name-file", ".ntcn"), ("--digest-file", ".ntcd"))


def _cli(which, args, stdout=None):
    head = [sys.executable, "-m", "ntcomp_amd"] if which == "python" else [NATIVE]
    return subprocess.run(head + [str(a) for a in args], stdout=stdout or subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, PYTHONPATH=REPO), timeout=300)


def _encode(which, idx, src, out, *extra, sides=False, ok=True):
    """-> (the archive and, with sides, the four side files; stderr; exit status)"""
    args = ["encode", "-i", idx, *extra]
    if sides:
        args += ["--non-acgt", "keep", "--qualities", "keep", "--names", "keep"]
        for flag, ext in SIDE:
            args += [flag, str(out) + ext]
    with open(out, "wb") as f:
        r = _cli(which, args + [src], stdout=f)
    if ok:
        assert r.returncode == 0, r.stderr[-2000:]
    files = [open(out, "rb").read()] + ([open(str(out) + ext, "rb").read() for _, ext in SIDE] if sides else [])
    return files, r.stderr, r.returncode


def bgzf_file(text, sizes):
    """text as BGZF: members of the given sizes in turn, then bgzip's empty last member"""
    out, at, i = [], 0, 0
    while at < len(text):
        n = sizes[i % len(sizes)]
        out.append(il.bgzf(il.raw_deflate(text[at:at + n], 1), text[at:at + n]))
        at += n
        i += 1
    return b"".join(out) + il.EOF_MEMBER


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """an index at k = 31; a FASTQ of two full blocks and 1,000 reads of 40-60 bases, some with an
    N, as plain text, as BGZF with members of 65,280 bytes, and as BGZF with odd member sizes so
    that the reader's cuts fall inside members"""
    d = tmp_path_factory.mktemp("infpipe")
    genome = nt.synth_genome(12, 300_000)
    nt.Index.build([genome.tobytes()], K).save(str(d / "idx"))
    n = 2 * 65536 + 1000
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
    (d / "r.fq.gz").write_bytes(bgzf_file(text, [65280]))
    (d / "odd.fq.gz").write_bytes(bgzf_file(text, [65280, 1, 40001, 12345, 65536 - 300, 77]))
    return {"d": d, "idx": str(d / "idx"), "text": text, "recs": recs}


@pytest.fixture(scope="module")
def host(pipe):
    """the plain text's archive and side files, and `--inflate host`'s over the BGZF file"""
    d = pipe["d"]
    plain, _, _ = _encode("native", pipe["idx"], d / "r.fq", d / "plain.dat", sides=True)
    files, err, _ = _encode("native", pipe["idx"], d / "r.fq.gz", d / "host.dat", "--inflate", "host", "--stats", sides=True)
    st = json.loads(err.decode().strip().splitlines()[-1])
    assert st["inflate"] == "host" and st["inflate_members"] == 0 and st["inflate_runs"] == 0
    assert files == plain
    return files


def _stats(err):
    return json.loads(err.decode().strip().splitlines()[-1])


def test_native_gpu_equals_host_and_plain(pipe, host):
    d = pipe["d"]
    files, err, _ = _encode("native", pipe["idx"], d / "r.fq.gz", d / "gpu.dat", "--inflate", "gpu", "--stats", sides=True)
    assert files == host
    st = _stats(err)
    members = len(nt.bgzf_members(open(d / "r.fq.gz", "rb").read()))
    assert st["inflate"] == "gpu" and st["inflate_members"] == members and st["inflate_bytes"] == len(pipe["text"])
    assert st["inflate_runs"] >= 1 and st["inflate_fallback_runs"] == 0 and st["inflate_s"] > 0
    assert st["reads"] == len(pipe["recs"]) and st["gpu_parsed_batches"] >= 1


def test_odd_member_sizes_and_small_batches(pipe, host):
    d = pipe["d"]
    files, err, _ = _encode("native", pipe["idx"], d / "odd.fq.gz", d / "odd.dat", "--inflate", "gpu", "--blocks-per-batch", "1",
                            "--stats", sides=True)
    assert files == host
    assert _stats(err)["inflate_bytes"] == len(pipe["text"])


def test_python_cli_and_two_contexts(pipe, host):
    d = pipe["d"]
    files, err, _ = _encode("python", pipe["idx"], d / "r.fq.gz", d / "py.dat", "--inflate", "gpu", "--stats", sides=True)
    assert files == host
    st = _stats(err)
    assert st["inflate"] == "gpu" and st["inflate_bytes"] == len(pipe["text"]) and st["inflate_fallback_runs"] == 0
    files, _, _ = _encode("native", pipe["idx"], d / "odd.fq.gz", d / "two.dat", "--inflate", "gpu", "--devices", "0,0", sides=True)
    assert files == host


def test_paired_with_two_bgzf_mates(pipe):
    d = pipe["d"]
    n = 20000
    m1 = b"".join(b"@p%d/1\n%s" % (i, r.split(b"\n", 1)[1]) for i, r in enumerate(pipe["recs"][:n]))
    m2 = b"".join(b"@p%d/2\n%s" % (i, r.split(b"\n", 1)[1]) for i, r in enumerate(pipe["recs"][n:2 * n]))
    (d / "m1.fq.gz").write_bytes(bgzf_file(m1, [65280]))
    (d / "m2.fq.gz").write_bytes(bgzf_file(m2, [30011, 65280]))
    a, _, _ = _encode("native", pipe["idx"], d / "m1.fq.gz", d / "pair-host.dat", "--mate-file", d / "m2.fq.gz", sides=True)
    b, err, _ = _encode("native", pipe["idx"], d / "m1.fq.gz", d / "pair-gpu.dat", "--mate-file", d / "m2.fq.gz", "--inflate", "gpu",
                        "--stats", sides=True)
    assert a == b
    st = _stats(err)
    assert st["pairs"] == n and st["inflate_bytes"] == len(m1) + len(m2) and st["inflate_fallback_runs"] == 0
    # a mate that is not BGZF is refused before anything is opened
    (d / "m2.plain.gz").write_bytes(gzip.compress(m2[:5000], 1))
    r = _cli("native", ["encode", "-i", pipe["idx"], "--inflate", "gpu", "--mate-file", d / "m2.plain.gz", d / "m1.fq.gz"])
    assert r.returncode == 2 and b"m2.plain.gz does not start with a BGZF member" in r.stderr


def test_a_flipped_crc_fails_alike(pipe):
    """one member's CRC flipped: the run falls back to the host's path, which fails as it does
    under `--inflate host`: same exit status, same message"""
    d = pipe["d"]
    blob = bytearray(open(d / "r.fq.gz", "rb").read())
    off, size, _ = nt.bgzf_members(bytes(blob))[3]
    blob[off + size - 8] ^= 0x10
    (d / "bad.fq.gz").write_bytes(bytes(blob))
    got = {}
    for eng in ("host", "gpu"):
        _, err, rc = _encode("native", pipe["idx"], d / "bad.fq.gz", d / ("bad-%s.dat" % eng), "--inflate", eng, ok=False)
        got[eng] = (rc, err.decode().strip().splitlines()[-1])
    assert got["host"][0] != 0 and got["gpu"] == got["host"], got


def test_a_plain_gzip_tail_goes_the_hosts_way(pipe):
    """a BGZF file followed by a plain gzip member: the tail is no BGZF member and takes the
    existing path; the output is the host engine's"""
    d = pipe["d"]
    k = 30000
    head, tail = b"".join(pipe["recs"][:k]), b"".join(pipe["recs"][k:k + 5000])
    (d / "tail.fq.gz").write_bytes(bgzf_file(head, [65280])[:-len(il.EOF_MEMBER)] + gzip.compress(tail, 6))
    a, _, _ = _encode("native", pipe["idx"], d / "tail.fq.gz", d / "tail-host.dat", "--inflate", "host", sides=True)
    b, err, _ = _encode("native", pipe["idx"], d / "tail.fq.gz", d / "tail-gpu.dat", "--inflate", "gpu", "--stats", sides=True)
    assert a == b
    st = _stats(err)
    assert st["reads"] == k + 5000 and st["inflate_bytes"] == len(head)


def test_library_surface(pipe):
    """nt.encode_file(inflate="gpu"): the "i" stats; host_parse and a plain input are refused"""
    d = pipe["d"]
    ix = nt.Index.load(pipe["idx"])
    ctx = nt.GpuContext(0)
    try:
        ctx.upload(ix)
        with open(d / "lib.dat", "wb") as f:
            st = nt.encode_file([ctx], str(d / "odd.fq.gz"), f.fileno(), inflate="gpu", non_acgt="mask")  # (the reads hold Ns)
        assert st["i"]["engine"] == 1 and st["i"]["bytes"] == len(pipe["text"]) and st["i"]["fallback_runs"] == 0
        assert st["i"]["members"] == len(nt.bgzf_members(open(d / "odd.fq.gz", "rb").read())) and st["i"]["seconds"] > 0
        with open(d / "lib2.dat", "wb") as f:
            nt.encode_file([ctx], str(d / "odd.fq.gz"), f.fileno(), non_acgt="mask")
        assert open(d / "lib.dat", "rb").read() == open(d / "lib2.dat", "rb").read()
        for kw, code in (({"host_parse": True}, 1), ({}, 10)):
            src = str(d / "odd.fq.gz") if kw else str(d / "r.fq")
            with open(d / "lib3.dat", "wb") as f, pytest.raises(nt.NtcError) as e:
                nt.encode_file([ctx], src, f.fileno(), inflate="gpu", **kw)
            assert e.value.code == code
        assert "BGZF" in str(e.value)
    finally:
        ctx.close()
