"""Deflate of the packed block streams on the GPU (deflate.hip, ntc_deflate_blocks_device, option
"gpu_deflate"): every member the device writes is byte for byte the host restatement's
(ntc_deflate_stream with NTC_DEFLATE_GPU, itself checked in test_deflate_gpu_host.py) and inflates
to its input under Python's zlib."""
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import ntcomp_amd as nt
import deflate_lib as dl
from test_codec_golden import CASES, recs_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = nt.GpuContext(0)
    yield c
    c.close()


def lay_out(streams_of_blocks, dropped=()):
    """hand-built blocks: for each block four byte strings (multiples of 8) -> metas and the
    payload that holds them back to back; the blocks listed in dropped get status 3"""
    metas, parts, off = [], [], 0
    for b, streams in enumerate(streams_of_blocks):
        m, size = dl.meta_for([len(s) // 8 for s in streams])
        for s in range(4):
            m.stream[s].offset += off
        if b in dropped:
            m.status = 3
        metas.append(m)
        parts += list(streams)
        off += size
    return metas, b"".join(parts)


def device_members(ctx, metas, payload, d_pay=None, cap=None):
    """ntc_deflate_blocks_device over the payload -> the members, [block][stream] (None where
    the block yields nothing), after checking that they lie back to back"""
    own = d_pay is None
    if own:
        d_pay = ctx.alloc(max(64, len(payload)))
        if len(payload):
            ctx.h2d(d_pay, np.frombuffer(payload, dtype=np.uint8))
    need = sum(dl.bound(8 * m.stream[s].encoded_size) for m in metas if m.status == 0 for s in range(4))
    cap = need if cap is None else cap
    d_out = ctx.alloc(max(64, cap))
    try:
        off_len, used = ctx.deflate_device(d_pay, metas, d_out, cap)
        out = np.zeros(max(used, 8), dtype=np.uint8)
        if used:
            ctx.d2h(out, d_out)
    finally:
        ctx.free(d_out)
        if own:
            ctx.free(d_pay)
    out = out[:used].tobytes()
    members, at = [], 0
    for b, m in enumerate(metas):
        if m.status:
            assert not off_len[b].any()
            members.append(None)
            continue
        row = []
        for s in range(4):
            o, n = int(off_len[b, s, 0]), int(off_len[b, s, 1])
            assert o == at
            row.append(out[o:o + n])
            at += n
        members.append(row)
    assert at == used
    return members


def host_members(metas, payload):
    return [None if m.status else [nt.deflate_stream(m, s, payload, "gpu")[32:] for s in range(4)] for m in metas]


@pytest.fixture(scope="module")
def listed():
    """the whole size x content list as blocks of four streams, an empty stream and a dropped
    block among them; the host restatement's members, computed once"""
    cs = [d for _, d in dl.word_cases()]
    assert any(len(d) == 0 for d in cs)
    while len(cs) % 4:
        cs.append(b"")
    blocks = [cs[i:i + 4] for i in range(0, len(cs), 4)]
    blocks.insert(2, [dl.content("fib", 4096)] * 4)  # the dropped one
    metas, payload = lay_out(blocks, dropped=(2,))
    return blocks, metas, payload, host_members(metas, payload)


def test_device_members_equal_the_host_restatement(ctx, listed):
    blocks, metas, payload, want = listed
    got = device_members(ctx, metas, payload)
    assert got[2] is None and want[2] is None
    for b, streams in enumerate(blocks):
        if b == 2:
            continue
        for s in range(4):
            dl.check_member(got[b][s], streams[s])
            assert got[b][s] == want[b][s], (b, s, len(streams[s]))
    # the same context again, the blocks in reverse order: tables and workspace are reused uncleared
    rmetas, rpayload = lay_out(blocks[::-1], dropped=(len(blocks) - 3,))
    again = device_members(ctx, rmetas, rpayload)
    assert again == got[::-1]


def test_capacity_is_checked_before_anything_runs(ctx, listed):
    _, metas, payload, _ = listed
    need = sum(dl.bound(8 * m.stream[s].encoded_size) for m in metas if m.status == 0 for s in range(4))
    with pytest.raises(nt.NtcError) as e:
        device_members(ctx, metas, payload, cap=need - 1)
    assert e.value.code == 5 and e.value.needed == need


def test_after_the_gpu_packer(ctx):
    """codec fixtures -> ntc_pack_blocks_device -> the device deflate, the payload never leaving
    the device in between: the members inflate to the fixtures' pre-deflate streams"""
    names = sorted(CASES)
    blocks = [recs_of(CASES[n]) for n in names]
    recs = np.concatenate(blocks)
    roffs = np.zeros(len(blocks) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(b) for b in blocks])
    cap = max(1 << 16, 16 * len(recs) + 1024 * len(blocks))
    d_recs, d_roffs, d_pay = ctx.alloc(recs.nbytes), ctx.alloc(roffs.nbytes), ctx.alloc(cap)
    try:
        ctx.h2d(d_recs, recs)
        ctx.h2d(d_roffs, roffs)
        metas, used = ctx.pack_device(d_recs, d_roffs, len(blocks), 1, d_pay, cap)
        members = device_members(ctx, metas, b"", d_pay=d_pay)
    finally:
        for p in (d_recs, d_roffs, d_pay):
            ctx.free(p)
    seen = 0
    for n, m, row in zip(names, metas, members):
        c = CASES[n]
        if c["dropped"]:
            assert m.status == 3 and row is None
            continue
        for s in range(4):
            raw = bytes.fromhex(c["streams"][s]["payload"])
            dl.check_member(row[s], raw)
            seen += 1
    assert seen >= 4 * 10


@pytest.fixture(scope="module")
def c91(ctx):
    genome = nt.synth_genome(1, 1_000_000)
    ix = nt.Index.build_gpu(ctx, [genome.tobytes()], 91)
    ctx.upload(ix)
    return genome


def batch_members(ctx, call, *args):
    """the call with the option off, then on -> (metas, raw payload, members by block)"""
    metas, payload = call(*args)[:2]
    ctx.set_option("gpu_deflate", 1)
    try:
        metas2, blob = call(*args)[:2]
        off_len = ctx.encode_members()
    finally:
        ctx.set_option("gpu_deflate", 0)
    assert len(off_len) == len(metas2) == len(metas)
    for a, b in zip(metas, metas2):
        assert a.status == b.status and a.num_records == b.num_records
        assert [(a.stream[s].num_u64, a.stream[s].encoded_size, a.stream[s].param) for s in range(4)] == \
            [(b.stream[s].num_u64, b.stream[s].encoded_size, b.stream[s].param) for s in range(4)]
    members = [None if m.status else [blob[int(o):int(o) + int(n)] for o, n in off_len[b]] for b, m in enumerate(metas)]
    assert sum(len(x) for row in members if row for x in row) == len(blob)
    return metas, payload, members


def test_gpu_deflate_on_the_batch_calls(ctx, c91):
    """ntc_encode_pack_batch and ntc_encode_pack_fastq under "gpu_deflate": the members equal the
    host restatement of the payload the same call returns with the option off"""
    n, L = 3000, 150
    reads = nt.synth_reads(c91, 2, 0, n, L, 10_000)
    offs = np.arange(0, n * L + 1, L, dtype=np.uint64)
    metas, payload, members = batch_members(ctx, ctx.encode_pack, reads, offs, 1024)
    assert len(metas) == 3 and members == host_members(metas, payload)
    text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, reads[i * L:(i + 1) * L].tobytes(), b"I" * L) for i in range(n))
    metas, payload, members = batch_members(ctx, ctx.encode_pack_fastq, text, n, 1024)
    assert len(metas) == 3 and members == host_members(metas, payload)
    # the option off again: the call leaves no members
    ctx.encode_pack(reads, offs, 1024)
    assert len(ctx.encode_members()) == 0


def test_one_full_block(ctx, c91):
    """65,536 C91-shaped reads, one call: the members equal the host restatement's; the sizes go
    to the log"""
    n, L = 65536, 150
    reads = nt.synth_reads(c91, 2, 0, n, L, 10_000)
    offs = np.arange(0, n * L + 1, L, dtype=np.uint64)
    metas, payload, members = batch_members(ctx, ctx.encode_pack, reads, offs, 65536)
    assert len(metas) == 1 and metas[0].status == 0
    want = host_members(metas, payload)
    raw = nt.stream_payloads(metas[0], payload)
    for s in range(4):
        huff = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
        lvl6 = zlib.compressobj(6, zlib.DEFLATED, -15)
        print("s%d raw %d gpu member %d huffman-only %d zlib-6 %d" % (
            s + 1, len(raw[s]), len(members[0][s]), len(huff.compress(raw[s]) + huff.flush()),
            len(lvl6.compress(raw[s]) + lvl6.flush())))
        assert zlib.decompress(members[0][s], 31) == raw[s]
        assert members[0][s] == want[0][s], s


# ---- the file pipeline and both command lines ---------------------------------------------------
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
K = 31


def _cli(which, args, stdout=None):
    head = [sys.executable, "-m", "ntcomp_amd"] if which == "python" else [NATIVE]
    return subprocess.run(head + [str(a) for a in args], stdout=stdout or subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, PYTHONPATH=REPO), timeout=300)


def _encode(which, idx, src, out, *extra):
    with open(out, "wb") as f:
        r = _cli(which, ["encode", "-i", idx, *extra, src], stdout=f)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out, "rb").read(), r.stderr


def _decode(idx, enc, *extra):
    r = _cli("native", ["decode", "-i", idx, *extra, enc])
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _blocks(data):
    """block for block what nt.read_block_streams gives: header fields and inflated streams"""
    pos, out = 32, []
    while pos < len(data):
        m, payload, used = nt.read_block_streams(data[pos:])
        out.append((m.num_records, [(m.stream[s].num_u64, m.stream[s].encoded_size, m.stream[s].param) for s in range(4)],
                    nt.stream_payloads(m, payload)))
        pos += used
    return out


def _info(enc):
    r = _cli("native", ["info", "--blocks", enc])
    assert r.returncode == 0, r.stderr[-2000:]
    keep = []
    for line in r.stdout.decode().splitlines()[1:]:
        w = line.split()
        keep.append((w[w.index("reads") + 1], w[w.index("records") + 1], w[w.index("first_read") + 1]))
    return keep


def _fastq(reads, names=None, quals=None):
    return [b"@%s\n%s\n+\n%s\n" % (names[i] if names else b"r%d" % i, r, quals[i] if quals else b"I" * len(r))
            for i, r in enumerate(reads)]


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """an index at k = 31 and a FASTQ of two full blocks and a partial one, reads of 40-60 bases"""
    d = tmp_path_factory.mktemp("dfpipe")
    genome = nt.synth_genome(12, 300_000)
    nt.Index.build([genome.tobytes()], K).save(str(d / "idx"))
    n = 2 * 65536 + 5000
    flat = nt.synth_reads(genome, 21, 0, n, 60, 10_000).tobytes()
    rng = np.random.default_rng(3)
    lens = rng.integers(40, 61, n)
    reads = [flat[60 * i:60 * i + int(lens[i])] for i in range(n)]
    (d / "r.fq").write_bytes(b"".join(_fastq(reads)))
    return {"d": d, "idx": str(d / "idx"), "fq": str(d / "r.fq"), "reads": reads, "genome": genome}


@pytest.fixture(scope="module")
def archives(pipe):
    d, out = pipe["d"], {}
    runs = {"gpu-n-1": ("native", ["--deflate", "gpu", "--blocks-per-batch", "1"]),
            "gpu-n-4-00": ("native", ["--deflate", "gpu", "--blocks-per-batch", "4", "--devices", "0,0"]),
            "gpu-n-1-00": ("native", ["--deflate", "gpu", "--blocks-per-batch", "1", "--devices", "0,0", "--stats"]),
            "gpu-p-4": ("python", ["--deflate", "gpu", "--blocks-per-batch", "4", "--stats"]),
            "zlib-n-4": ("native", ["--deflate", "zlib", "--blocks-per-batch", "4"]),
            "zlib-p-1-00": ("python", ["--deflate", "zlib", "--blocks-per-batch", "1", "--devices", "0,0"])}
    for tag, (which, extra) in runs.items():
        out[tag], err = _encode(which, pipe["idx"], pipe["fq"], d / (tag + ".dat"), *extra)
        if "--stats" in extra:
            assert b'"deflate": "gpu"' in err, err[-600:]
    return out


def test_pipeline_archives_agree(pipe, archives):
    """every gpu archive is the same bytes whatever the batch size, the contexts or the command
    line; block for block it holds the zlib archive's headers and streams; both decode alike"""
    gpu = [v for k, v in archives.items() if k.startswith("gpu")]
    assert len(gpu) == 4 and all(g == gpu[0] for g in gpu)
    assert archives["zlib-n-4"] == archives["zlib-p-1-00"] != gpu[0]
    assert _blocks(gpu[0]) == _blocks(archives["zlib-n-4"]) and len(_blocks(gpu[0])) == 3
    d = pipe["d"]
    fa = _decode(pipe["idx"], d / "gpu-n-1.dat")
    assert fa == _decode(pipe["idx"], d / "zlib-n-4.dat")
    assert fa == b"".join(b">seq.%d\n%s\n" % (i + 1, r) for i, r in enumerate(pipe["reads"]))
    assert _info(d / "gpu-n-1.dat") == _info(d / "zlib-n-4.dat")
    # the members of the file are the host restatement's: the file is the block-by-block host codec's
    blob, pos = nt.file_header(), 32
    while pos < len(archives["zlib-n-4"]):
        m, payload, used = nt.read_block_streams(archives["zlib-n-4"][pos:])
        blob += nt.deflate_block(m, payload, "gpu")
        pos += used
    assert blob == gpu[0]


def test_reads_and_shards_of_a_gpu_archive(pipe):
    d, n = pipe["d"], len(pipe["reads"])
    enc = d / "gpu-n-1.dat"
    if not enc.exists():
        _encode("native", pipe["idx"], pipe["fq"], enc, "--deflate", "gpu", "--blocks-per-batch", "1")
    full = [b">seq.%d\n%s\n" % (i + 1, r) for i, r in enumerate(pipe["reads"])]
    assert _decode(pipe["idx"], enc, "--reads", "65530-65540") == b"".join(full[65529:65540])
    parts = [_decode(pipe["idx"], enc, "--shard", "%d/3" % i) for i in (1, 2, 3)]
    assert b"".join(parts) == b"".join(full) and all(parts)


def test_side_files_under_the_gpu_engine(pipe, tmp_path):
    """names, qualities (rANS), non-ACGT runs and digests beside a gpu archive: verify passes, decode
    gives the FASTQ back, and the side files are those of the run whose host engine the sections
    share (--deflate auto)"""
    n = 65536 + 3000
    rng = np.random.default_rng(8)
    reads = [bytearray(r) for r in pipe["reads"][:n]]
    for i in range(0, n, 97):
        reads[i][7] = ord("N")
    reads = [bytes(r) for r in reads]
    names = [b"run7.%d len=%d" % (i, len(r)) for i, r in enumerate(reads)]
    q = rng.integers(35, 75, sum(map(len, reads)), dtype=np.uint8).tobytes()
    quals, at = [], 0
    for r in reads:
        quals.append(q[at:at + len(r)])
        at += len(r)
    text = b"".join(_fastq(reads, names, quals))
    (tmp_path / "s.fq").write_bytes(text)
    side = {}
    for tag in ("gpu", "auto"):
        side[tag] = ["--exceptions", tmp_path / (tag + ".nx"), "--quality-file", tmp_path / (tag + ".q"), "--name-file",
                     tmp_path / (tag + ".n"), "--digest-file", tmp_path / (tag + ".d")]
        _encode("native", pipe["idx"], tmp_path / "s.fq", tmp_path / (tag + ".dat"), "--deflate", tag, "--non-acgt", "keep",
                "--qualities", "keep", "--quality-coder", "rans", "--names", "keep", *side[tag])
    for ext in ("nx", "q", "n", "d"):
        assert (tmp_path / ("gpu." + ext)).read_bytes() == (tmp_path / ("auto." + ext)).read_bytes(), ext
    r = _cli("native", ["verify", "-i", pipe["idx"], *side["gpu"], tmp_path / "gpu.dat"])
    assert r.returncode == 0 and b"verify: OK" in r.stdout, r.stderr[-2000:]
    assert _decode(pipe["idx"], tmp_path / "gpu.dat", *side["gpu"]) == text
    assert _blocks((tmp_path / "gpu.dat").read_bytes()) == _blocks((tmp_path / "auto.dat").read_bytes())


def _both(pipe, tmp_path, src, *extra):
    g, _ = _encode("native", pipe["idx"], src, tmp_path / "g.dat", "--deflate", "gpu", *extra)
    z, _ = _encode("native", pipe["idx"], src, tmp_path / "z.dat", "--deflate", "zlib", *extra)
    assert g != z and _blocks(g) == _blocks(z)
    return g, z


def test_other_inputs_under_the_gpu_engine(pipe, tmp_path):
    """--mate-file, --host-parse, a FASTA input and a gzip'd FASTQ: the gpu archive holds the zlib
    archive's blocks"""
    n = 70_000
    reads = pipe["reads"][:n]
    (tmp_path / "h.fq").write_bytes(b"".join(_fastq(reads)))
    g, _ = _both(pipe, tmp_path, tmp_path / "h.fq", "--host-parse")
    assert len(_blocks(g)) == 2
    (tmp_path / "c.fa").write_bytes(b"".join(b">c%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    assert _blocks(_both(pipe, tmp_path, tmp_path / "c.fa")[0]) == _blocks(g)
    with gzip.open(tmp_path / "z.fq.gz", "wb", compresslevel=1) as f:
        f.write(b"".join(_fastq(reads)))
    assert _blocks(_both(pipe, tmp_path, tmp_path / "z.fq.gz")[0]) == _blocks(g)
    m1 = [b"p%d/1" % i for i in range(n // 2)]
    m2 = [b"p%d/2" % i for i in range(n // 2)]
    (tmp_path / "1.fq").write_bytes(b"".join(_fastq(reads[0::2], m1)))
    (tmp_path / "2.fq").write_bytes(b"".join(_fastq(reads[1::2], m2)))
    gp, _ = _both(pipe, tmp_path, tmp_path / "1.fq", "--mate-file", tmp_path / "2.fq")
    assert _blocks(gp) == _blocks(g)
    (tmp_path / "i.fq").write_bytes(b"".join(a + b for a, b in zip(_fastq(reads[0::2], m1), _fastq(reads[1::2], m2))))
    assert _both(pipe, tmp_path, tmp_path / "i.fq", "--interleaved")[0] == gp


def test_dropped_block_and_bad_read_under_the_gpu_engine(pipe, tmp_path):
    """a middle block without a short record is dropped as under zlib (App. B.3); a base absent
    from the index fails with the same bad read"""
    g = pipe["genome"].tobytes()
    clean = [g[100 * i % 200_000:100 * i % 200_000 + 50] for i in range(65536)]  # error-free: long records only
    reads = pipe["reads"][:65536] + clean + pipe["reads"][65536:70000]
    (tmp_path / "m.fq").write_bytes(b"".join(_fastq(reads)))
    gz, z = _both(pipe, tmp_path, tmp_path / "m.fq")
    assert len(_blocks(gz)) == 2
    assert _decode(pipe["idx"], tmp_path / "g.dat") == _decode(pipe["idx"], tmp_path / "z.dat")
    bad = list(pipe["reads"][:3000])
    bad[2345] = bad[2345][:9] + b"N" + bad[2345][10:]
    (tmp_path / "b.fq").write_bytes(b"".join(_fastq(bad)))
    errs = []
    for engine in ("gpu", "zlib"):
        r = _cli("native", ["encode", "-i", pipe["idx"], "--deflate", engine, tmp_path / "b.fq"])
        assert r.returncode != 0
        errs.append((r.returncode, [ln for ln in r.stderr.decode().splitlines() if "2346" in ln or "2345" in ln]))
    assert errs[0] == errs[1] and errs[0][1]


def test_option_off_changes_nothing(pipe, tmp_path, ctx):
    """the other engines' archives are the block-by-block host codec's bytes, as before"""
    n = 70_000
    reads = pipe["reads"][:n]
    (tmp_path / "o.fq").write_bytes(b"".join(_fastq(reads)))
    ix = nt.Index.load(pipe["idx"])
    ctx.upload(ix)
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8)
    offs = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    recs, roff = ctx.encode(bases, offs)
    engines = ["zlib"] + (["libdeflate", "adaptive"] if nt.libdeflate_available() else [])
    for engine in engines:
        exp = nt.file_header()
        for b0 in range(0, n, 65536):
            b1 = min(n, b0 + 65536)
            m, payload = nt.pack_block(recs[int(roff[b0]):int(roff[b1])], b1 - b0)
            exp += nt.deflate_block(m, payload, engine)
        got, _ = _encode("native", pipe["idx"], tmp_path / "o.fq", tmp_path / "o.dat", "--deflate", engine)
        assert got == exp, engine
