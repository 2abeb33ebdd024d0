"""Decoding a range of reads on the GPU: the window on the text formatters (window.hip) through
ntc_decode_set_window, the block seek of the file pipeline through ntc_decode_file_ex5, and both
command lines.

The existing full decode is the reference for everything: a window's or a range's text must be
the cut of the unwindowed text that range_lib.py (plain Python) makes."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import names_lib as nl
import ntcomp_amd as nt
import pair_lib as pl
import range_lib as rl

pytestmark = pytest.mark.gpu
INVALID_ARG, FORMAT, DIGEST = 1, 8, 12
BR = 128
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
ALL = dict(non_acgt="keep", qualities="keep", names="keep", digests=True)
FORMATS = ["fasta", "named_fasta", "fastq-pack", "fastq-rans", "named_fastq-pack", "named_fastq-rans"]


@pytest.fixture(scope="module")
def env():
    genome = nt.synth_genome(7, 20_000)
    ix = nt.Index.build([genome.tobytes()], 31)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    yield genome, ix, ctx
    ctx.close()


def _reads(rng, genome, n, lo=1, hi=300):
    g = genome.tobytes()
    lens = rng.integers(lo, hi + 1, n)
    lens[0], lens[-1] = lo, hi
    out = [g[s:s + ln] for s, ln in zip(rng.integers(0, len(g) - hi, n).tolist(), lens.tolist())]
    for i in range(0, n, 7):  # N runs for the exceptions
        r = bytearray(out[i])
        r[len(r) // 2:len(r) // 2 + 3] = b"N" * len(r[len(r) // 2:len(r) // 2 + 3])
        out[i] = bytes(r)
    return out


N = 3 * BR + 64  # 3 blocks and a part


@pytest.fixture(scope="module")
def batch(env):
    """448 reads of 1-300 bases with N runs, names of many lengths, encoded under both quality
    coders; and the unwindowed text of every format (first_id 95), decoded once"""
    genome, _, ctx = env
    rng = np.random.default_rng(80)
    reads = _reads(rng, genome, N)
    names = [b"r%d:" % i + bytes(rng.integers(65, 91, int(rng.integers(0, 40)), dtype=np.uint8)) for i in range(N)]
    quals = [bytes(rng.integers(33, 75, len(r), dtype=np.uint8)) for r in reads]
    text = nl.make_fastq(names, reads, quals)
    enc = {c: ctx.encode_pack_fastq(text, N, block_reads=BR, quality_coder=c, **ALL) for c in ("pack", "rans")}
    assert len(enc["pack"][0]) == 4 and len(enc["pack"][3]) > 0
    whole = {fmt: _decode(ctx, enc, fmt) for fmt in FORMATS}
    assert whole["named_fastq-pack"] == whole["named_fastq-rans"] == text
    assert whole["fasta"].startswith(b">seq.95\n") and b">seq.99\n" in whole["fasta"] and b">seq.100\n" in whole["fasta"]
    assert all(len(rl.records(t)) == N for t in whole.values())
    return enc, whole


def _decode(ctx, enc, fmt, window=None, first_id=95, dg=None):
    """one batch through ntc_decode_fasta_unpacked in fmt, every side list pending"""
    kind, _, coder = fmt.partition("-")
    metas, payload, nb, runs, (qm, qp), (nm, npay), digests = enc[coder or "pack"]
    arr = (nt.BlockMeta * len(metas))(*metas)
    assert ctx.unpack(arr, payload, len(metas))[:2] == (len(metas), N)
    if kind.startswith("named"):
        ctx.set_names(nm, npay)
    if kind.endswith("fastq"):
        ctx.set_qualities(qm, qp)
    ctx.set_exceptions(runs, ctx.substitute)
    ctx.decode_set_digests(digests if dg is None else dg)
    if window is not None:
        ctx.set_window(*window)
    return ctx.decode_fasta_unpacked(first_id=first_id)


WINDOWS = [(0, N), (0, 1), (N - 1, 1), (127, 2), (63, 2), (1, N - 2)]


# 1 windows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_a_window_is_the_cut_of_the_unwindowed_text(env, batch, fmt):
    _, _, ctx = env
    enc, whole = batch
    for first, count in WINDOWS:
        got = _decode(ctx, enc, fmt, (first, count))  # (its length is *out_len)
        assert got == rl.cut(whole[fmt], first, first + count), (first, count)
    if fmt == "fasta":  # ids cross 99 -> 100 inside a window, and keep the batch's numbering
        assert _decode(ctx, enc, fmt, (4, 2)).startswith(b">seq.99\n") and b"\n>seq.100\n" in _decode(ctx, enc, fmt, (4, 2))


def test_a_window_through_ntc_decode_fasta(env):
    """the records path (host unpack): the same window, *out_len its bytes; a size query keeps it"""
    genome, _, ctx = env
    rng = np.random.default_rng(81)
    reads = [r.replace(b"N", b"A") for r in _reads(rng, genome, 200, 31, 90)]
    bases, offs = nt.pack_reads(reads)
    recs, _ = ctx.encode(bases, offs)
    out = np.zeros(len(bases) + 20 * 200, dtype=np.uint8)
    n = ctypes.c_uint64()
    call = lambda cap: ctx.L.ntc_decode_fasta(ctx.h, recs.ctypes.data, len(recs), 200, len(bases), 95, out.ctypes.data, cap,
                                              ctypes.byref(n))
    assert call(len(out)) == 0
    whole = out[:n.value].tobytes()
    for first, count in [(0, 200), (0, 1), (199, 1), (127, 2), (3, 5)]:
        ctx.set_window(first, count)
        assert call(0) == 5 and n.value == len(whole)  # NTC_ERR_CAPACITY: the whole batch's bytes, the window waits
        out[:] = 0
        assert call(len(out)) == 0
        assert out[:n.value].tobytes() == rl.cut(whole, first, first + count) and not out[n.value:].any()
    assert call(len(out)) == 0 and out[:n.value].tobytes() == whole  # and it is gone


# 2 pairs -----------------------------------------------------------------------------------------------
def test_an_even_window_splits_its_pairs(env, batch):
    _, _, ctx = env
    enc, whole = batch
    ctx.paired = "nocheck"
    try:
        for fmt in ("fasta", "named_fastq-rans"):
            lines = 4 if "fastq" in fmt else 2
            for first, count in [(0, N), (0, 2), (N - 2, 2), (126, 4), (62, 4), (2, N - 4)]:
                got = _decode(ctx, enc, fmt, (first, count))
                assert got == pl.split(rl.cut(whole[fmt], first, first + count), lines), (fmt, first, count)
                assert ctx.pair_split() == len(got[0])
        for first, count in [(1, 2), (2, 3), (1, 1), (127, 2)]:  # whole pairs only
            with pytest.raises(nt.NtcError) as e:
                _decode(ctx, enc, "fasta", (first, count))
            assert e.value.code == INVALID_ARG, (first, count)
        assert _decode(ctx, enc, "fasta") == pl.split(whole["fasta"], 2)
    finally:
        ctx.paired = "off"


# 3 refusal, 4 consumption ------------------------------------------------------------------------------
def test_refusals_and_consumption(env, batch):
    _, _, ctx = env
    enc, whole = batch
    fresh = nt.GpuContext(0)
    try:
        fresh.share_index(ctx)
        plain = _decode(fresh, enc, "named_fastq-pack")
        arr = (nt.BlockMeta * 4)(*enc["pack"][0])
        fresh.unpack(arr, enc["pack"][1], 4)
        bare = fresh.decode_fasta_unpacked(first_id=95)  # no side list pending: the masked reads as FASTA
    finally:
        fresh.close()
    assert plain == whole["named_fastq-pack"] and bare != whole["fasta"] and len(bare) == len(whole["fasta"])
    for first, count in [(N, 1), (N - 1, 2), (0, N + 1), (N + 5, 3)]:  # first + count > n_reads
        with pytest.raises(nt.NtcError) as e:
            _decode(ctx, enc, "named_fastq-pack", (first, count))
        assert e.value.code == INVALID_ARG, (first, count)
        # the failed call took the window and the side lists with it: a plain call follows
        arr = (nt.BlockMeta * 4)(*enc["pack"][0])
        ctx.unpack(arr, enc["pack"][1], 4)
        assert ctx.decode_fasta_unpacked(first_id=95) == bare
    with pytest.raises(nt.NtcError) as e:
        ctx.set_window(3, 0)
    assert e.value.code == INVALID_ARG
    assert _decode(ctx, enc, "named_fastq-pack", (5, 9)) == rl.cut(plain, 5, 14)
    assert _decode(ctx, enc, "named_fastq-pack") == plain  # a windowed call, then a plain one: a fresh context's
    ctx.set_window(5, 9)  # a window set and dropped again by an empty one
    with pytest.raises(nt.NtcError):
        ctx.set_window(0, 0)
    assert _decode(ctx, enc, "named_fastq-pack") == plain


# 5 digests ----------------------------------------------------------------------------------------------
def test_a_window_still_verifies_the_whole_batch(env, batch):
    _, _, ctx = env
    enc, whole = batch
    dg = enc["rans"][6]
    for block, field in [(3, "d_seq"), (2, "d_qual"), (1, "d_name"), (3, "d_sym")]:
        bad = [nt.DigestMeta.from_buffer_copy(bytes(m)) for m in dg]
        setattr(bad[block], field, getattr(bad[block], field) ^ 1)
        with pytest.raises(nt.NtcError) as e:  # the window is block 0's first read
            _decode(ctx, enc, "named_fastq-rans", (0, 1), dg=bad)
        assert e.value.code == DIGEST and f"block {block}" in str(e.value), (block, field, str(e.value))
    assert _decode(ctx, enc, "named_fastq-rans", (0, 1)) == rl.cut(whole["named_fastq-rans"], 0, 1)
    got = ctx.decode_digests()
    assert [m.d_seq for m in got] == [m.d_seq for m in dg] and len(got) == 4  # every block was digested


# ---- the file pipeline ------------------------------------------------------------------------------------
SIDES = ("dat", "ntcx", "ntcq", "ntcn", "ntcd")
TOTAL = 200_000
BLOCKS = [65_536, 65_536, 65_536, 3_392]


@pytest.fixture(scope="module")
def archive(env, tmp_path_factory):
    """100,000 pairs of 30-60 bp reads (three blocks of 65,536 reads and a part of 3,392), all
    four side files, encoded once by the existing pipeline; the full decodes are the reference"""
    genome, ix, ctx = env
    d = tmp_path_factory.mktemp("range")
    rng = np.random.default_rng(90)
    g = genome.tobytes()
    lens = rng.integers(30, 61, TOTAL).tolist()
    starts = rng.integers(0, len(g) - 60, TOTAL).tolist()
    qual_pool = bytes(rng.integers(40, 75, 1 << 16, dtype=np.uint8))
    recs = []
    for i, (s, ln) in enumerate(zip(starts, lens)):
        read = g[s:s + ln]
        if i % 11 == 0:
            read = read[:ln // 2] + b"N" + read[ln // 2 + 1:]
        q = qual_pool[(i * 37) & 0xFFFF:][:ln]
        q = q + qual_pool[:ln - len(q)]
        recs.append(b"@p%d/%d\n" % (i // 2, 1 + i % 2) + read + b"\n+\n" + q + b"\n")
    text = b"".join(recs)
    (d / "in.fq").write_bytes(text)
    fds = {s: open(d / f"a.{s}", "wb") for s in SIDES}
    try:
        st = nt.encode_file([ctx], str(d / "in.fq"), fds["dat"].fileno(), threads=4, blocks_per_batch=2, deflate="zlib",
                            non_acgt="keep", nx_fd=fds["ntcx"].fileno(), qualities="keep", q_fd=fds["ntcq"].fileno(),
                            names="keep", n_fd=fds["ntcn"].fileno(), d_fd=fds["ntcd"].fileno(), pair_mode="ids")
    finally:
        for f in fds.values():
            f.close()
    assert st["reads"] == TOTAL and st["blocks"] == 4
    side = dict(nx_path=str(d / "a.ntcx"), q_path=str(d / "a.ntcq"), n_path=str(d / "a.ntcn"), d_path=str(d / "a.ntcd"))
    info = nt.archive_info(str(d / "a.dat"))
    assert [b["reads"] for b in info["blocks"]] == BLOCKS and info["n_reads"] == TOTAL and info["tail_bytes"] == 0
    full_fq = _file_decode([ctx], d, "a.dat", side)[0]
    assert full_fq == text
    full_fa = _file_decode([ctx], d, "a.dat", {})[0]
    assert len(rl.records(full_fa)) == TOTAL and full_fa.startswith(b">seq.1\n")
    ix.save(str(d / "idx"))
    return dict(d=d, side=side, fq=rl.records(full_fq), fa=rl.records(full_fa), info=info)


def _file_decode(ctxs, d, name, side, out="o.txt", **kw):
    with open(d / out, "wb") as f:
        st = nt.decode_file(ctxs, str(d / name), f.fileno(), threads=4, **{"blocks_per_batch": 1, **kw}, **side)
    return (d / out).read_bytes(), st


def _span(recs, a, b):
    """reads a..b, 1-based and inclusive, of a text's records"""
    return b"".join(recs[a - 1:b])


RANGES = [(1, 1), (65_536, 65_537), (65_537, 131_072), (200_000, 200_000), (1, 200_000)]


@pytest.mark.parametrize("n_ctx,bpb,host_unpack", [(1, 1, False), (2, 1, False), (1, 2, False), (2, 2, False), (1, 2, True)])
def test_single_ranges(env, archive, tmp_path, monkeypatch, n_ctx, bpb, host_unpack):
    _, _, ctx = env
    if host_unpack:
        monkeypatch.setenv("NTC_HOST_UNPACK", "1")
    ctxs = [ctx]
    if n_ctx == 2:
        ctxs.append(nt.GpuContext(0))
        ctxs[1].share_index(ctx)
    try:
        for a, b in RANGES:
            got, st = _file_decode(ctxs, archive["d"], "a.dat", archive["side"], out=str(tmp_path / "o"), blocks_per_batch=bpb,
                                   reads=(a - 1, b - a + 1))
            assert got == _span(archive["fq"], a, b), (a, b)
            b0, b1, before, head, tail = rl.block_range(BLOCKS, a - 1, b - a + 1)
            assert st["r"] == dict(blocks_total=4, reads_total=TOTAL, first_block=b0, blocks_read=b1 - b0 + 1,
                                   reads_written=b - a + 1, head_skipped=head, tail_skipped=tail)
            assert st["blocks"] == b1 - b0 + 1 and st["reads"] == b - a + 1 and st["bytes_out"] == len(got)
            assert st["d"]["sections"] == b1 - b0 + 1
    finally:
        for c in ctxs[1:]:
            c.close()


PARTS = [(1, 7), (8, 65_536), (65_537, 65_540), (65_541, 196_609), (196_610, 200_000)]


@pytest.mark.parametrize("kind", ["fasta", "fastq"])
def test_a_partition_concatenates_to_the_full_text(env, archive, tmp_path, kind):
    """FASTA without side files: the archive's seq.N numbering is kept; FASTQ with all of them"""
    _, _, ctx = env
    side = archive["side"] if kind == "fastq" else {}
    parts = [_file_decode([ctx], archive["d"], "a.dat", side, out=str(tmp_path / "o"), blocks_per_batch=2,
                          reads=(a - 1, b - a + 1))[0] for a, b in PARTS]
    assert b"".join(parts) == b"".join(archive["fq" if kind == "fastq" else "fa"])
    if kind == "fasta":
        assert parts[3].startswith(b">seq.65541\n") and parts[4].startswith(b">seq.196610\n")


def test_ex5_without_a_range_is_ex4(env, archive, tmp_path):
    _, _, ctx = env
    a, sa = _file_decode([ctx], archive["d"], "a.dat", archive["side"], out=str(tmp_path / "a"))
    b, sb = _file_decode([ctx], archive["d"], "a.dat", archive["side"], out=str(tmp_path / "b"), reads=(0, 0))
    c, _ = _file_decode([ctx], archive["d"], "a.dat", archive["side"], out=str(tmp_path / "c"), reads=(12_345, 0))
    assert a == b == c == b"".join(archive["fq"])
    assert sb["r"] == dict(blocks_total=4, reads_total=TOTAL, first_block=0, blocks_read=4, reads_written=TOTAL,
                           head_skipped=0, tail_skipped=0)
    assert all(sa[k] == sb[k] for k in ("reads", "bases", "blocks", "dropped_blocks", "bytes_out", "error")) and sa["d"] == sb["d"]
    outs = {}
    for tag, kw in (("ex4", {}), ("ex5", dict(reads=(0, 0)))):  # and under pairs, where the level below is ex4 itself
        with open(tmp_path / (tag + ".1"), "wb") as f1, open(tmp_path / (tag + ".2"), "wb") as f2:
            st = nt.decode_file([ctx], str(archive["d"] / "a.dat"), f1.fileno(), threads=4, out_fd2=f2.fileno(), pair_mode="nocheck",
                                **archive["side"], **kw)
        outs[tag] = ((tmp_path / (tag + ".1")).read_bytes(), (tmp_path / (tag + ".2")).read_bytes(), st["p"], st["d"], st["reads"])
    assert outs["ex4"] == outs["ex5"] and outs["ex4"][0] == b"".join(archive["fq"][0::2])


def test_skipped_blocks_are_never_read(env, archive, tmp_path):
    _, _, ctx = env
    blk = archive["info"]["blocks"]
    data = bytearray((archive["d"] / "a.dat").read_bytes())
    bs = struct.unpack_from("<I", data, blk[1]["offset"])[0]  # block 1's first gzip payload, not its header
    mid = blk[1]["offset"] + 32 + bs // 2
    assert bs > 200
    data[mid:mid + 64] = bytes(b ^ 0x5A for b in data[mid:mid + 64])
    (tmp_path / "bad.dat").write_bytes(bytes(data))
    assert [b["bad"] for b in nt.archive_info(str(tmp_path / "bad.dat"))["blocks"]] == [0, 0, 0, 0]  # the headers are whole
    side = {k: v for k, v in archive["side"].items() if k != "d_path"}
    got, st = _file_decode([ctx], tmp_path, "bad.dat", side, reads=(196_700, 100))  # inside block 3
    assert got == _span(archive["fq"], 196_701, 196_800) and st["r"]["blocks_read"] == st["blocks"] == 1
    got, st = _file_decode([ctx], tmp_path, "bad.dat", archive["side"], reads=(131_072, 10))  # block 2, under the digests
    assert got == _span(archive["fq"], 131_073, 131_082) and st["blocks"] == 1 and st["d"]["sections"] == 1
    for first, count in [(65_536, 1), (65_535, 2), (0, TOTAL), (131_071, 2)]:  # touching block 1
        with pytest.raises(nt.NtcError) as e:
            _file_decode([ctx], tmp_path, "bad.dat", side, reads=(first, count))
        assert e.value.code == FORMAT and "block 1" in str(e.value), str(e.value)
    got, st = _file_decode([ctx], tmp_path, "bad.dat", side)  # the unranged decode: as ever, the output ends before block 1
    assert got == _span(archive["fq"], 1, 65_536) and st["dropped_blocks"] == 3 and st["blocks"] == 1


def test_digests_under_a_range(env, archive, tmp_path):
    _, _, ctx = env
    data = bytearray((archive["d"] / "a.ntcq").read_bytes())
    pos = 32
    for _ in range(2):  # to block 2's section: 24 bytes, the alphabet, one gzip member
        pos += 24 + data[pos + 17] + struct.unpack_from("<I", data, pos + 20)[0]
    assert data[pos + 24] == 40  # the lowest quality of the fixture: the section's first alphabet byte
    data[pos + 24] = 39
    (tmp_path / "bad.ntcq").write_bytes(bytes(data))
    side = dict(archive["side"], q_path=str(tmp_path / "bad.ntcq"))
    got, st = _file_decode([ctx], archive["d"], "a.dat", side, out=str(tmp_path / "o"), reads=(196_608, 3_392))  # block 3
    assert got == _span(archive["fq"], 196_609, 200_000) and st["d"]["blocks_qual"] == 1
    with pytest.raises(nt.NtcError) as e:
        _file_decode([ctx], archive["d"], "a.dat", side, out=str(tmp_path / "o"), reads=(131_072 + 50, 10))  # in block 2
    assert e.value.code == DIGEST and "block 2 " in str(e.value) and "component qual" in str(e.value)
    assert e.value.bad_read == 131_072


def test_side_file_checks_and_refusals(env, archive, tmp_path):
    _, _, ctx = env
    mode, metas, payload = nt.read_names(archive["side"]["n_path"])
    with open(tmp_path / "short.ntcn", "wb") as f:  # its last section cut off
        nt.write_names(f.fileno(), mode, metas[:-1], payload)
    side = dict(archive["side"], n_path=str(tmp_path / "short.ntcn"))
    with pytest.raises(nt.NtcError) as e:
        _file_decode([ctx], archive["d"], "a.dat", side, out=str(tmp_path / "o"), reads=(0, 10))
    assert e.value.code == FORMAT and "names: 3 sections for 4 blocks" in str(e.value)
    assert (tmp_path / "o").read_bytes() == b"" and e.value.stats["gpu_s"] == 0 and e.value.stats["wall_s"] == 0  # before any GPU call
    # a section that disagrees with its block's header, far from the range: the digest file's section 1
    dg = bytearray(open(archive["side"]["d_path"], "rb").read())
    assert struct.unpack_from("<Q", dg, 32 + 56)[0] == 65_536
    struct.pack_into("<Q", dg, 32 + 56, 65_535)
    (tmp_path / "off.ntcd").write_bytes(bytes(dg))
    with pytest.raises(nt.NtcError) as e:
        _file_decode([ctx], archive["d"], "a.dat", dict(archive["side"], d_path=str(tmp_path / "off.ntcd")),
                     out=str(tmp_path / "o"), reads=(199_000, 10))
    assert e.value.code == FORMAT and "digests: section 1 holds 65535 reads" in str(e.value)
    assert (tmp_path / "o").read_bytes() == b"" and e.value.stats["gpu_s"] == 0
    for first, count in [(TOTAL, 1), (TOTAL + 5, 1), (TOTAL - 1, 2), (0, TOTAL + 1)]:
        with pytest.raises(nt.NtcError) as e:
            _file_decode([ctx], archive["d"], "a.dat", archive["side"], out=str(tmp_path / "o"), reads=(first, count))
        assert e.value.code == INVALID_ARG and "holds 200000 reads" in str(e.value)


def test_pairs_under_a_range(env, archive, tmp_path):
    _, _, ctx = env
    fq = archive["fq"]
    with open(tmp_path / "o1", "wb") as f1, open(tmp_path / "o2", "wb") as f2:
        st = nt.decode_file([ctx], str(archive["d"] / "a.dat"), f1.fileno(), threads=4, blocks_per_batch=2, out_fd2=f2.fileno(),
                            pair_mode="nocheck", reads=(2, 131_072), **archive["side"])  # reads 3..131074
    assert (tmp_path / "o1").read_bytes() == b"".join(fq[2:131_074:2])
    assert (tmp_path / "o2").read_bytes() == b"".join(fq[3:131_074:2])
    assert st["p"]["pairs"] == 65_536 and st["reads"] == 131_072 and st["r"]["blocks_read"] == 3
    with open(tmp_path / "x1", "wb") as f1, open(tmp_path / "x2", "wb") as f2, pytest.raises(nt.NtcError) as e:
        nt.decode_file([ctx], str(archive["d"] / "a.dat"), f1.fileno(), out_fd2=f2.fileno(), pair_mode="nocheck", reads=(1, 4),
                       **archive["side"])  # reads 2..5
    assert e.value.code == INVALID_ARG


# ---- command lines --------------------------------------------------------------------------------------------
def _cli(which, args, stdout=None):
    head = [sys.executable, "-m", "ntcomp_amd"] if which == "python" else [NATIVE]
    return subprocess.run(head + args, stdout=stdout or subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, PYTHONPATH=REPO), timeout=300)


@pytest.mark.parametrize("which", ["native", "python"])
def test_command_lines(archive, tmp_path, which):
    d, s = archive["d"], archive["side"]
    side = ["--exceptions", s["nx_path"], "--quality-file", s["q_path"], "--name-file", s["n_path"], "--digest-file", s["d_path"]]
    base = ["-i", str(d / "idx"), str(d / "a.dat")]
    r = _cli(which, ["decode", "--reads", "65530-65540", "--stats"] + side + base)
    assert r.returncode == 0 and r.stdout == _span(archive["fq"], 65_530, 65_540), r.stderr[-2000:]
    assert b'"r_blocks_read": 2' in r.stderr and b'"r_reads_written": 11' in r.stderr and b'"r_head_skipped": 65529' in r.stderr
    r = _cli(which, ["decode", "--reads", "199999-"] + base)  # FASTA: the numbering of the archive
    assert r.returncode == 0 and r.stdout == _span(archive["fa"], 199_999, 200_000), r.stderr[-2000:]
    parts = []
    for i in range(1, 5):
        r = _cli(which, ["decode", "--shard", f"{i}/4"] + side + base)
        assert r.returncode == 0, r.stderr[-2000:]
        parts.append(r.stdout)
    assert b"".join(parts) == b"".join(archive["fq"]) and parts[3] == _span(archive["fq"], 196_609, 200_000)
    r = _cli(which, ["verify", "--shard", "2/4"] + side + base)
    assert r.returncode == 0 and b"verify: OK: 1 of 4 blocks, 65536 reads" in r.stdout, r.stderr[-2000:]
    r = _cli(which, ["decode", "--reads", "3-131074", "--mate-out", str(tmp_path / "m2")] + side + base)
    assert r.returncode == 0 and r.stdout == b"".join(archive["fq"][2:131_074:2]), r.stderr[-2000:]
    assert (tmp_path / "m2").read_bytes() == b"".join(archive["fq"][3:131_074:2])
    info = archive["info"]
    r = _cli(which, ["info", "--blocks", str(d / "a.dat")])
    lines = r.stdout.decode().splitlines()
    assert r.returncode == 0 and lines[0] == (f"blocks 4 reads {TOTAL} records {info['n_records']} "
                                              f"bytes {sum(b['bytes'] for b in info['blocks'])} trailing_bytes 0")
    first = 1
    for i, b in enumerate(info["blocks"]):
        assert lines[1 + i] == (f"block {i} offset {b['offset']} bytes {b['bytes']} reads {b['reads']} records {b['records']} "
                                f"first_read {first}")
        first += b["reads"]
    assert _cli(which, ["info", str(d / "a.dat")]).stdout.decode() == lines[0] + "\n"
