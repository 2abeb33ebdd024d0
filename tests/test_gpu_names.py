"""FASTQ read names on the GPU (names.hip): the canonical front- and back-coded sections
ntc_encode_pack_fastq yields under names keep / id, their way back into the text on decode,
the "NTCN" file through the pipelines, and a byte-for-byte lossless FASTQ round trip.

The checker is independent of the code under test: names_lib.py (plain Python / numpy)."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import names_lib as nl
import ntcomp_amd as nt

pytestmark = pytest.mark.gpu
FORMAT, UNSUPPORTED = 8, 10
BR = 128  # block_reads: two groups of 64 per block
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")


@pytest.fixture(scope="module")
def env():
    genome = nt.synth_genome(7, 20_000)
    ix = nt.Index.build([genome.tobytes()], 31)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    yield genome, ix, ctx
    ctx.close()


def _blob(metas):
    return b"".join(ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m)) for m in metas)


def _reads(rng, genome, n, lo=1, hi=300):
    g = genome.tobytes()
    lens = rng.integers(lo, hi + 1, n)
    lens[0], lens[-1] = lo, hi
    return [g[s:s + ln] for s, ln in zip(rng.integers(0, len(g) - hi, n).tolist(), lens.tolist())]


def _encode(ctx, text, n, mode="keep", **kw):
    """-> (block metas, payload, name metas as dicts, name payload)"""
    out = ctx.encode_pack_fastq(text, n, block_reads=BR, names=mode, **kw)
    nm, npay = out[-1]
    return out[0], out[1], [nl.meta_dict(m) for m in nm], npay


def _check(ctx, names, reads, mode="keep", **fmt):
    """encode under mode; the sections must be names_lib's of the names as mode sees them"""
    text = nl.make_fastq(names, reads, **fmt)
    metas, payload, nm, npay = _encode(ctx, text, len(reads), mode)
    exp_m, exp_p = nl.sections([nl.name_of(b"@" + n, mode) for n in names], BR)
    assert nm == exp_m
    assert npay == exp_p
    return text, metas, payload, nm, npay


def _cols(m, pay):
    """the three columns of section m"""
    n, o = m["n_reads"], m["payload_off"]
    return (np.frombuffer(pay, "<u2", n, o).tolist(), list(pay[o + 2 * n:o + 3 * n]), list(pay[o + 3 * n:o + 4 * n]))


def _unpack(ctx, metas, payload):
    arr = (nt.BlockMeta * len(metas))(*metas)
    ok, nr, nb = ctx.unpack(arr, payload, len(metas))
    assert ok == len(metas)
    return nr, nb


def _tune(names, block, padded):
    """grow the last name of a whole block, byte by byte, until its section needs padding or not
    ('~' occurs in no other name, so only that name's mid grows)"""
    last = (block + 1) * BR - 1
    for _ in range(8):
        m = nl.sections(names, BR)[0][block]
        if ((4 * m["n_reads"] + m["mid_bytes"]) % 8 != 0) == padded:
            return
        names[last] += b"~"
    raise AssertionError("unreachable")


@pytest.fixture(scope="module")
def lengths_batch(env):
    """Three and a half blocks: every length class, the two 255 caps, the neighbour cases, and
    identical names across the group and the block boundary."""
    genome = env[0]
    rng = np.random.default_rng(1)
    names = nl.edge_names()
    names += nl.illumina_names(rng, 3 * BR + BR // 2 - len(names))
    names[62] = names[63] = names[64] = b"across:the:group"
    names[BR - 2] = names[BR - 1] = names[BR] = b"across:the:block"
    _tune(names, 1, padded=False)
    _tune(names, 2, padded=True)
    return names, _reads(rng, genome, len(names))


# 1 ---------------------------------------------------------------------------------------------
def test_lengths(env, lengths_batch):
    _, _, ctx = env
    names, reads = lengths_batch
    assert {len(n) for n in names} >= {0, 1, 63, 64, 65, 255, 256, 257, 300, 4095}
    assert min(len(r) for r in reads) == 1 and max(len(r) for r in reads) == 300
    _, _, _, nm, npay = _check(ctx, names, reads)
    assert [m["n_reads"] for m in nm] == [BR, BR, BR, BR // 2]
    for m in nm:
        assert m["payload_bytes"] == 8 * ((4 * m["n_reads"] + m["mid_bytes"] + 7) // 8)
    assert len(npay) == sum(m["payload_bytes"] for m in nm)
    pads = [m["payload_bytes"] - 4 * m["n_reads"] - m["mid_bytes"] for m in nm]
    assert pads[1] == 0 and pads[2] > 0
    lens, pres, sufs = _cols(nm[0], npay)
    i = names.index(next(n for n in names if n.endswith(b"second:longer")))
    assert (pres[i], sufs[i]) == (255, 0)  # 300 shared leading bytes: the cap
    j = next(k for k, n in enumerate(names) if n.startswith(b"another"))
    assert (pres[j], sufs[j]) == (0, 255)  # 300 shared trailing bytes


# 2 ---------------------------------------------------------------------------------------------
def test_neighbours(env, lengths_batch):
    _, _, ctx = env
    names, reads = lengths_batch
    _, _, _, nm, npay = _check(ctx, names, reads)
    lens, pres, sufs = _cols(nm[0], npay)
    at = lambda first: next(k for k in range(len(names)) if names[k] == first)
    s = at(b"same")
    assert [(pres[k], sufs[k]) for k in (s + 1, s + 2)] == [(4, 0), (4, 0)]  # identical neighbours
    p = at(b"prefix:of:the:next")
    assert (pres[p + 1], sufs[p + 1], lens[p + 1]) == (6, 0, 6)  # a prefix of the previous one: no mid
    assert (pres[p + 2], sufs[p + 2]) == (6, 0)                  # and the reverse
    a = at(b"aaaa")
    assert [(pres[k], sufs[k]) for k in (a + 1, a + 3)] == [(2, 0), (1, 1)]  # the two overlap cases
    assert names[63] == names[64] and (pres[63], sufs[63]) == (16, 0) and (pres[64], sufs[64], lens[64]) == (0, 0, 16)
    l1, p1, s1 = _cols(nm[1], npay)
    assert names[BR - 1] == names[BR] and (pres[BR - 1], sufs[BR - 1]) == (16, 0) and (p1[0], s1[0], l1[0]) == (0, 0, 16)


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["crlf", "no_last_newline", "bytes", "empty"])
def test_text_shapes(env, shape):
    genome, _, ctx = env
    rng = np.random.default_rng(3)
    names = nl.illumina_names(rng, BR + 77)
    reads = _reads(rng, genome, len(names))
    fmt = {}
    if shape == "crlf":
        fmt["eol"] = b"\r\n"
    elif shape == "no_last_newline":
        fmt["last_newline"] = False
    elif shape == "bytes":
        names[5:10] = [b"@at@", b"+plus+", b"sp ace and\ttab ", b"hi\x80\xff\xfe", b"\t"]
        names[-1] = b"@+ \t\xc3\xa9"
    else:
        names[0] = names[1] = names[64] = names[-1] = b""
    text, metas, payload, nm, _ = _check(ctx, names, reads, **fmt)
    assert sum(m["name_bytes"] for m in nm) == sum(len(n) for n in names)
    m0, p0, nb0 = ctx.encode_pack_fastq(text, len(reads), block_reads=BR)
    assert _blob(metas) == _blob(m0) and payload == p0  # the records of the run without names


# 4 ---------------------------------------------------------------------------------------------
def test_mode_id(env):
    genome, _, ctx = env
    rng = np.random.default_rng(4)
    names = nl.illumina_names(rng, BR + 9)  # "id comment": cut at the space
    names[3:9] = [b"tab\there", b"tab\tthere", b"nowhitespace", b" leading space", b"x" * 70 + b" one", b"x" * 70 + b" two"]
    reads = _reads(rng, genome, len(names))
    _, _, _, nm, npay = _check(ctx, names, reads, "id")
    lens, pres, sufs = _cols(nm[0], npay)
    assert lens[3:9] == [3, 3, 12, 0, 70, 70]
    assert (pres[4], sufs[4]) == (3, 0) and (pres[8], sufs[8]) == (70, 0)  # measured on the cut names
    assert sum(m["name_bytes"] for m in nm) < sum(len(n) for n in names)
    _check(ctx, names, reads, "id", eol=b"\r\n")
    _check(ctx, names, reads, "keep")


# 5 ---------------------------------------------------------------------------------------------
def test_errors(env):
    genome, _, ctx = env
    rng = np.random.default_rng(5)
    names = nl.illumina_names(rng, BR + 40)
    reads = _reads(rng, genome, len(names))
    names[BR + 7] = b"n" * 4096
    for second in (None, 20):
        if second is not None:
            names[second] = b"m" * 4096
        text = nl.make_fastq(names, reads)
        with pytest.raises(nt.NtcError) as e:
            ctx.encode_pack_fastq(text, len(reads), block_reads=BR, names="keep")
        assert e.value.code == FORMAT and e.value.bad_read == (BR + 7 if second is None else second)
        assert ctx.names() == ([], b"")
    assert len(ctx.encode_pack_fastq(text, len(reads), block_reads=BR)[0]) == 2  # fine where names are dropped
    names[20] = b"m" * 4095 + b" cut away"
    names[BR + 7] = b"n" * 4095
    _check(ctx, names, reads, "id")
    assert ctx.get_option("names") == 0
    bases, offs = nt.pack_reads(reads)
    ctx.set_option("names", 1)
    try:
        with pytest.raises(nt.NtcError) as e:
            ctx.encode_pack(bases, offs, block_reads=BR)
        assert e.value.code == UNSUPPORTED
        with pytest.raises(nt.NtcError) as e:
            ctx.encode(bases, offs)
        assert e.value.code == UNSUPPORTED
    finally:
        ctx.set_option("names", 0)
    assert len(ctx.encode_pack(bases, offs, block_reads=BR)[0]) == 2


# 6 ---------------------------------------------------------------------------------------------
def test_decode(env, lengths_batch):
    _, _, ctx = env
    names, reads = lengths_batch
    rng = np.random.default_rng(6)
    quals = [bytes(rng.integers(33, 127, len(r), dtype=np.uint8)) for r in reads]
    reads = list(reads)
    for i in range(0, len(reads), 5):  # N runs for the exceptions
        r = bytearray(reads[i])
        p = int(rng.integers(0, len(r)))
        r[p:p + 7] = b"N" * len(r[p:p + 7])
        reads[i] = bytes(r)
    text = nl.make_fastq(names, reads, quals)
    metas, payload, nb, runs, (qm, qp), (nm, npay) = ctx.encode_pack_fastq(
        text, len(reads), block_reads=BR, non_acgt="keep", qualities="keep", names="keep")
    assert len(runs) >= len(reads) // 5 and [nl.meta_dict(m) for m in nm] == nl.sections(names, BR)[0]
    masked = [r.replace(b"N", bytes([ctx.substitute])) for r in reads]
    _unpack(ctx, metas, payload)
    ctx.set_names(nm, npay)  # names alone: FASTA
    assert ctx.decode_fasta_unpacked(first_id=1) == nl.named_text(names, masked)
    ctx.set_names(nm, npay)  # with qualities: FASTQ
    ctx.set_qualities(qm, qp)
    assert ctx.decode_fasta_unpacked(first_id=1) == nl.named_text(names, masked, quals)
    ctx.set_names(nm, npay)  # and with the exceptions: the text that went in
    ctx.set_qualities(qm, qp)
    ctx.set_exceptions(runs, ctx.substitute)
    assert ctx.decode_fasta_unpacked(first_id=1) == text
    again = ctx.decode_fasta_unpacked(first_id=5)  # the sections were used: seq.N again
    assert again == b"".join(b">seq.%d\n%s\n" % (5 + i, r) for i, r in enumerate(masked))
    ctx.set_names(nm, npay)
    ctx.set_names([], b"")  # cleared
    assert ctx.decode_fasta_unpacked(first_id=5) == again


# 7 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded(env):
    genome, _, ctx = env
    rng = np.random.default_rng(7)
    names = nl.illumina_names(rng, BR + 70)
    names[1:3] = [b"ab", b"abcdefgh"]
    reads = _reads(rng, genome, len(names))
    text = nl.make_fastq(names, reads)
    metas, payload, nb, (nm, npay) = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, names="keep")
    return names, reads, metas, payload, nm, npay


@pytest.mark.parametrize("damage", ["pre_plus_suf", "pre_past_previous", "restart_pre", "mids", "len_4096", "one_read_fewer",
                                    "one_read_more"])
def test_bad_sections_on_decode(env, encoded, damage):
    _, _, ctx = env
    names, reads, metas, payload, nm, npay = encoded
    nm = [nt.NameMeta.from_buffer_copy(_blob([m])) for m in nm]
    pay = bytearray(npay)
    n0 = nm[0].n_reads
    if damage == "pre_plus_suf":  # read 5: suf = len, pre stays >= 1
        assert pay[2 * n0 + 5] >= 1
        pay[3 * n0 + 5] = min(255, names[5].__len__())
    elif damage == "pre_past_previous":  # "ab" then "abcdefgh": pre 3 fits the name, not its predecessor
        pay[2 * n0 + 2], pay[3 * n0 + 2] = 3, 0
    elif damage == "restart_pre":
        pay[2 * n0 + 64] = 1
    elif damage == "mids":  # eight bytes of mid that no read claims
        nm[1].mid_bytes += 8
        nm[1].payload_bytes += 8
        pay += bytes(8)
    elif damage == "len_4096":
        pay[0:2] = (4096).to_bytes(2, "little")
    else:
        more = names[:-1] if damage == "one_read_fewer" else names + [b"x"]
        m, p = nl.sections(more, BR)
        nm = [nt.NameMeta(x["n_reads"], x["name_bytes"], x["mid_bytes"], x["payload_off"], x["payload_bytes"]) for x in m]
        pay = p
    _unpack(ctx, metas, payload)
    ctx.set_names(nm, bytes(pay))
    with pytest.raises(nt.NtcError) as e:  # no text comes back
        ctx.decode_fasta_unpacked(first_id=1)
    assert e.value.code == FORMAT
    assert ctx.decode_fasta_unpacked(first_id=1).startswith(b">seq.1\n")  # the sections are gone
    ctx.set_names(*[encoded[4], encoded[5]])  # and the good ones still decode
    assert ctx.decode_fasta_unpacked(first_id=1) == nl.named_text(names, reads)


def test_set_names_checks_size_and_place(env, encoded):
    _, _, ctx = env
    nm = [nt.NameMeta.from_buffer_copy(_blob([m])) for m in encoded[4]]
    for field, delta in (("payload_bytes", 8), ("payload_off", 4), ("payload_off", 1 << 20), ("mid_bytes", 8)):
        bad = [nt.NameMeta.from_buffer_copy(_blob([m])) for m in nm]
        setattr(bad[1], field, getattr(bad[1], field) + delta)
        with pytest.raises(nt.NtcError) as e:
            ctx.set_names(bad, encoded[5])
        assert e.value.code == FORMAT, field


# 8 ---------------------------------------------------------------------------------------------
def _encode_file(ctxs, path, tmp_path, tag, mode="keep", **kw):
    with open(tmp_path / (tag + ".dat"), "wb") as f, open(tmp_path / (tag + ".ntcn"), "wb") as q:
        st = nt.encode_file(ctxs, str(path), f.fileno(), threads=4, blocks_per_batch=1, deflate="zlib",
                            names=mode, n_fd=q.fileno(), **kw)
    return st, (tmp_path / (tag + ".ntcn")).read_bytes()


def test_files_round_trip(env, tmp_path):
    genome, _, ctx = env
    ctx2 = nt.GpuContext(0)
    ctx2.share_index(ctx)
    try:
        n, L = 70_000, 40
        rng = np.random.default_rng(8)
        flat = nt.synth_reads(genome, 9, 0, n, L, 10_000).tobytes()
        reads = [flat[i * L:(i + 1) * L] for i in range(n)]
        names = nl.illumina_names(rng, n)
        text = nl.make_fastq(names, reads)
        (tmp_path / "r.fq").write_bytes(text)
        with gzip.open(tmp_path / "r.fq.gz", "wb", compresslevel=1) as f:
            f.write(text)
        with open(tmp_path / "plainest.dat", "wb") as f:  # today's call, no option at all
            nt.encode_file([ctx], str(tmp_path / "r.fq"), f.fileno(), threads=4, blocks_per_batch=1, deflate="zlib")
        exp_m, exp_p = nl.sections(names, 65536)
        side = {}
        for tag, path, ctxs in (("plain", "r.fq", [ctx]), ("gz", "r.fq.gz", [ctx]), ("two", "r.fq", [ctx, ctx2])):
            st, side[tag] = _encode_file(ctxs, tmp_path / path, tmp_path, tag)
            assert st["reads"] == n and st["dropped_blocks"] == 0 and st["blocks"] == 2 and st["gpu_parsed"] > 0
            assert (tmp_path / (tag + ".dat")).read_bytes() == (tmp_path / "plainest.dat").read_bytes()
            mode, metas, pay = nt.read_names(tmp_path / (tag + ".ntcn"))
            assert mode == 1 and [nl.meta_dict(m) for m in metas] == exp_m and pay == exp_p
            assert st["n"] == dict(sections=2, names=n, name_bytes=sum(len(x) for x in names), payload_bytes=len(exp_p),
                                   deflated_bytes=len(side[tag]) - 32 - 2 * 32)
        assert side["plain"] == side["gz"] == side["two"]
        assert ctx.get_option("names") == 0 and ctx2.get_option("names") == 0
        for ctxs in ([ctx], [ctx, ctx2]):
            with open(tmp_path / "named.out", "wb") as f:
                std = nt.decode_file(ctxs, str(tmp_path / "plain.dat"), f.fileno(), threads=4, blocks_per_batch=1,
                                     n_path=str(tmp_path / "plain.ntcn"))
            assert std["reads"] == n and (tmp_path / "named.out").read_bytes() == nl.named_text(names, reads)
        with open(tmp_path / "plain.out", "wb") as f:  # without the side file: seq.N
            nt.decode_file([ctx], str(tmp_path / "plain.dat"), f.fileno(), threads=4, blocks_per_batch=1)
        assert (tmp_path / "plain.out").read_bytes() == b"".join(b">seq.%d\n%s\n" % (i + 1, r) for i, r in enumerate(reads))
        # a side file with a section removed belongs to another encoding
        raw = side["plain"]
        gz0 = int.from_bytes(raw[32 + 24:32 + 28], "little")
        (tmp_path / "short.ntcn").write_bytes(raw[:32 + 32 + gz0])
        with open(tmp_path / "bad.out", "wb") as f, pytest.raises(nt.NtcError) as e:
            nt.decode_file([ctx], str(tmp_path / "plain.dat"), f.fileno(), threads=4, blocks_per_batch=1,
                           n_path=str(tmp_path / "short.ntcn"))
        assert e.value.code == FORMAT and "names" in str(e.value)
    finally:
        ctx2.close()


@pytest.mark.parametrize("case", ["blank_line", "fasta", "host_parse"])
def test_files_without_a_gpu_text_path_are_unsupported(env, tmp_path, case):
    genome, _, ctx = env
    rng = np.random.default_rng(9)
    reads = _reads(rng, genome, 300, 40, 40)
    names = nl.sra_names(300, 40)
    text = nl.make_fastq(names, reads)
    kw = {}
    if case == "blank_line":
        cut = text.index(b"\n@SRR", len(text) // 2) + 1
        text = text[:cut] + b"\n" + text[cut:]
    elif case == "fasta":
        text = nl.named_text(names, reads)
    else:
        kw["host_parse"] = True
    (tmp_path / "u.fq").write_bytes(text)
    with pytest.raises(nt.NtcError) as e:
        _encode_file([ctx], tmp_path / "u.fq", tmp_path, "u", **kw)
    assert e.value.code == UNSUPPORTED and "names: " in str(e.value)
    assert {"blank_line": "blank line", "fasta": "not FASTQ", "host_parse": "host_parse"}[case] in str(e.value)
    if case == "blank_line":
        assert e.value.bad_read == 0  # the batch that holds the line starts at read 0
    with open(tmp_path / "ok.dat", "wb") as f:  # and each passes where the names are dropped
        assert nt.encode_file([ctx], str(tmp_path / "u.fq"), f.fileno(), threads=4, **kw)["reads"] == 300
    assert ctx.get_option("names") == 0


# 9 ---------------------------------------------------------------------------------------------
def test_lossless_fastq_through_the_native_cli(env, tmp_path):
    """A canonical FASTQ file (LF, upper-case bases with N / IUPAC runs, bare '+', Illumina-style
    names) comes back byte for byte from the three side files."""
    genome, ix, _ = env
    rng = np.random.default_rng(10)
    n = 3000
    reads = _reads(rng, genome, n, 20, 150)
    for i in range(0, n, 6):
        r = bytearray(reads[i])
        p = int(rng.integers(0, len(r)))
        sym = b"NRYKM"[i % 5:i % 5 + 1]
        r[p:p + 5] = sym * len(r[p:p + 5])
        reads[i] = bytes(r)
    quals = [bytes(rng.integers(33, 75, len(r), dtype=np.uint8)) for r in reads]
    text = nl.make_fastq(nl.illumina_names(rng, n), reads, quals)
    (tmp_path / "in.fq").write_bytes(text)
    ix.save(str(tmp_path / "idx"))
    side = ["--exceptions", str(tmp_path / "x.ntcx"), "--quality-file", str(tmp_path / "q.ntcq"),
            "--name-file", str(tmp_path / "n.ntcn")]
    with open(tmp_path / "enc.dat", "wb") as f:
        r = subprocess.run([NATIVE, "encode", "-i", str(tmp_path / "idx"), "--non-acgt", "keep", "--qualities", "keep",
                            "--names", "keep", *side, "--stats", str(tmp_path / "in.fq")], stdout=f,
                           stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert b'"names": "keep"' in r.stderr and b'"n_names": 3000' in r.stderr
    with open(tmp_path / "out.fq", "wb") as f:
        r = subprocess.run([NATIVE, "decode", "-i", str(tmp_path / "idx"), *side, str(tmp_path / "enc.dat")], stdout=f,
                           stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "out.fq").read_bytes() == text
