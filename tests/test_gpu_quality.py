"""FASTQ quality scores on the GPU (quality.hip): the canonical packed sections
ntc_encode_pack_fastq yields under qualities keep / bin8, and their way back to FASTQ text
on decode.

The checker is independent of the code under test: qual_lib.py (numpy) holds the mode
tables, the alphabet, the width rule and the bit packing."""
import ctypes

import numpy as np
import pytest

import ntcomp_amd as nt
import qual_lib as ql

pytestmark = pytest.mark.gpu
FORMAT, UNSUPPORTED = 8, 10
BR = 1024  # block_reads


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


def _batch(rng, n_syms_per_block, n_reads=3 * BR + BR // 2, ends=(63, 1, 0)):
    return ql.ragged_batch(rng, n_syms_per_block, BR, n_reads, ends)


def _encode(ctx, text, n, mode="keep", **kw):
    """-> (block metas, payload, quality metas as dicts, quality words)"""
    out = ctx.encode_pack_fastq(text, n, block_reads=BR, qualities=mode, **kw)
    qm, qp = out[-1]
    return out[0], out[1], [ql.meta_dict(m) for m in qm], np.frombuffer(qp, dtype="<u8")


def _check_sections(ctx, text, n, mode="keep"):
    metas, payload, qm, qw = _encode(ctx, text, n, mode)
    exp_m, exp_w = ql.sections(text, BR, mode)
    assert qm == exp_m
    assert np.array_equal(qw, exp_w)
    return metas, payload, qm, qw


def _unpack(ctx, metas, payload):
    arr = (nt.BlockMeta * len(metas))(*metas)
    ok, nr, nb = ctx.unpack(arr, payload, len(metas))
    assert ok == len(metas)
    return nr, nb


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_syms,w", [(1, 0), (2, 1), (3, 2), (4, 2), (5, 4), (16, 4), (17, 8), (94, 8)])
def test_widths_and_word_boundaries(env, n_syms, w):
    """Three and a half blocks of ragged reads (1..300 bases, a read of one base); blocks 0,
    1, 2 hold 63, 1 and 0 qualities modulo 64, the last block is short."""
    _, _, ctx = env
    reads, quals = _batch(np.random.default_rng(100 + n_syms), [n_syms] * 4)
    text = ql.make_fastq(reads, quals)
    _, _, qm, qw = _check_sections(ctx, text, len(reads))
    assert [m["n_quals"] % 64 for m in qm[:3]] == [63, 1, 0] and qm[3]["n_reads"] == BR // 2
    assert min(len(r) for r in reads) == 1 and max(len(r) for r in reads) == 300
    for m in qm:  # the packed size follows from the width alone
        assert (m["width"], m["n_syms"]) == (w, n_syms)
        assert m["payload_bytes"] == 8 * ((m["n_quals"] * w + 63) // 64)
    assert len(qw) * 8 == sum(m["payload_bytes"] for m in qm)
    if w:
        assert any(m["n_quals"] * w % 64 == 0 for m in qm) and any(m["n_quals"] * w % 64 for m in qm)


# 2 ---------------------------------------------------------------------------------------------
def test_alphabets_are_per_block(env):
    """2, 17 and 1 symbols in blocks 0, 1, 2: a presence map that leaked into the next block
    would widen it."""
    _, _, ctx = env
    reads, quals = _batch(np.random.default_rng(2), [2, 17, 1], n_reads=3 * BR)
    _, _, qm, _ = _check_sections(ctx, ql.make_fastq(reads, quals), len(reads))
    assert [(m["n_syms"], m["width"]) for m in qm] == [(2, 1), (17, 8), (1, 0)]
    assert qm[2]["payload_bytes"] == 0 and qm[2]["payload_off"] == qm[1]["payload_off"] + qm[1]["payload_bytes"]


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["crlf", "no_last_newline", "at_plus", "one_base"])
def test_text_shapes(env, shape):
    _, _, ctx = env
    rng = np.random.default_rng(3)
    reads, quals = _batch(rng, [5, 5], n_reads=BR + 77, ends=())
    kw = {}
    if shape == "crlf":
        kw["eol"] = b"\r\n"
    elif shape == "no_last_newline":
        kw["last_newline"] = False
    elif shape == "at_plus":
        quals = [(b"@" if i % 2 else b"+") + q[1:] for i, q in enumerate(quals)]
    else:
        reads[-1], quals[-1] = reads[-1][:1], quals[-1][:1]
        reads[0], quals[0] = reads[0][:1], quals[0][:1]
    text = ql.make_fastq(reads, quals, **kw)
    metas, payload, qm, _ = _check_sections(ctx, text, len(reads))
    assert sum(m["n_quals"] for m in qm) == sum(len(q) for q in quals)
    m0, p0, nb0 = ctx.encode_pack_fastq(text, len(reads), block_reads=BR)
    assert _blob(metas) == _blob(m0) and payload == p0  # the records of the run without qualities


# 4 ---------------------------------------------------------------------------------------------
def test_bin8(env):
    _, _, ctx = env
    rng = np.random.default_rng(4)
    reads, quals = _batch(rng, [94, 94], n_reads=BR + 300, ends=())
    text = ql.make_fastq(reads, quals)
    tab = ql.mode_table("bin8")
    for q, level in ((0, 0), (1, 1), (2, 6), (9, 6), (10, 15), (19, 15), (20, 22), (24, 22), (25, 27), (29, 27), (30, 33),
                     (34, 33), (35, 37), (39, 37), (40, 40), (93, 40)):
        assert tab[33 + q] == 33 + level  # the table itself, as the issue states it
    metas, payload, qm, qw = _check_sections(ctx, text, len(reads), "bin8")
    for m in qm:
        assert m["n_syms"] == 9 and m["alphabet"] == bytes(33 + v for v in (0, 1, 6, 15, 22, 27, 33, 37, 40))
    qmetas, qpay = ctx.qualities()
    _unpack(ctx, metas, payload)
    ctx.set_qualities(qmetas, qpay)
    assert ctx.decode_fasta_unpacked(first_id=1) == ql.fastq_text(list(zip(reads, quals)), 1, "bin8")


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["0x1f", "0x7f", "space"])
def test_errors_name_the_read(env, damage):
    _, _, ctx = env
    reads, quals = _batch(np.random.default_rng(5), [4, 4], n_reads=BR + 200, ends=())
    bad = BR + 101
    reads[bad] = b"ACGTACGTAC"
    quals[bad] = b"IIIIIIIIII"
    if damage == "space":
        reads[bad] = b"ACGT CGTAC"  # 9 bases kept, 10 qualities
    else:
        quals[bad] = b"IIII" + bytes([int(damage, 16)]) + b"IIIII"
    text = ql.make_fastq(reads, quals)
    for mode in ("keep", "bin8"):
        with pytest.raises(nt.NtcError) as e:
            ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities=mode)
        assert e.value.code == FORMAT and e.value.bad_read == bad
        assert ctx.qualities() == ([], b"")
    for kw in ({}, {"qualities": "drop"}):
        assert len(ctx.encode_pack_fastq(text, len(reads), block_reads=BR, **kw)[0]) == 2


# 6 ---------------------------------------------------------------------------------------------
def test_default_is_untouched(env):
    _, _, ctx = env
    reads, quals = _batch(np.random.default_rng(6), [7, 7], n_reads=BR + 10, ends=())
    text = ql.make_fastq(reads, quals)
    assert ctx.get_option("qualities") == 0
    m0, p0, nb0 = ctx.encode_pack_fastq(text, len(reads), block_reads=BR)
    m1, p1, nb1, (qm, qp) = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="drop")
    assert (qm, qp) == ([], b"") and _blob(m1) == _blob(m0) and p1 == p0 and nb1 == nb0
    m2, p2, nb2, (qm, qp) = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="keep")
    assert len(qm) == 2 and _blob(m2) == _blob(m0) and p2 == p0 and nb2 == nb0
    assert ctx.get_option("qualities") == 0  # the mode held for that call only
    bases, offs = nt.pack_reads(reads)
    ctx.set_option("qualities", 1)
    try:
        with pytest.raises(nt.NtcError) as e:
            ctx.encode_pack(bases, offs, block_reads=BR)
        assert e.value.code == UNSUPPORTED
        with pytest.raises(nt.NtcError) as e:
            ctx.encode(bases, offs)
        assert e.value.code == UNSUPPORTED
    finally:
        ctx.set_option("qualities", 0)
    assert len(ctx.encode_pack(bases, offs, block_reads=BR)[0]) == 2


# 7 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded(env):
    """One batch, encoded once: (reads, quals, block metas, payload, quality metas, words)."""
    _, _, ctx = env
    reads, quals = _batch(np.random.default_rng(7), [4, 40, 1], n_reads=2 * BR + 19, ends=(63, 1))
    text = ql.make_fastq(reads, quals)
    metas, payload, nb, (qm, qp) = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="keep")
    return reads, quals, metas, payload, qm, qp


@pytest.mark.parametrize("first_id", [1, 9, 99, 99_999])
def test_round_trip_to_fastq(env, encoded, first_id):
    _, _, ctx = env
    reads, quals, metas, payload, qm, qp = encoded
    nr, nb = _unpack(ctx, metas, payload)
    assert nr == len(reads)
    ctx.set_qualities(qm, qp)
    text = ctx.decode_fasta_unpacked(first_id=first_id)
    assert text == ql.fastq_text(list(zip(reads, quals)), first_id)
    fasta = ctx.decode_fasta_unpacked(first_id=first_id)  # the sections were used: FASTA again
    assert fasta == b"".join(b">seq.%d\n%s\n" % (first_id + i, r) for i, r in enumerate(reads))


# 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["code", "n_quals", "section_missing", "width"])
def test_decode_validation(env, encoded, damage):
    _, _, ctx = env
    reads, quals, metas, payload, qm, qp = encoded
    qm = [nt.QualMeta.from_buffer_copy(bytes(_blob([m]))) for m in qm]
    qp = bytearray(qp)
    _unpack(ctx, metas, payload)
    at_set = False
    if damage == "code":  # block 0 has 4 symbols at width 2, block 1 40 at width 8: code 255
        assert qm[1].width == 8 and qm[1].n_syms == 40
        qp[qm[1].payload_off + 11] = 0xFF
    elif damage == "n_quals":  # one quality fewer: the same words still hold it
        assert qm[1].n_quals * 8 % 64 == 8
        qm[1].n_quals -= 1
        qm[1].payload_bytes -= 8
    elif damage == "section_missing":
        qm = qm[:-1]
    else:
        qm[0].width = 4
        at_set = True
    if at_set:
        with pytest.raises(nt.NtcError) as e:
            ctx.set_qualities(qm, bytes(qp))
        assert e.value.code == FORMAT
        return
    ctx.set_qualities(qm, bytes(qp))
    with pytest.raises(nt.NtcError) as e:  # no text comes back
        ctx.decode_fasta_unpacked(first_id=1)
    assert e.value.code == FORMAT
    assert ctx.decode_fasta_unpacked(first_id=1).startswith(b">seq.1\n")  # the sections are gone


# 9 ---------------------------------------------------------------------------------------------
def test_together_with_non_acgt_keep(env):
    _, _, ctx = env
    rng = np.random.default_rng(9)
    reads, quals = _batch(rng, [8, 8], n_reads=BR + 50, ends=())
    for i in range(0, len(reads), 7):
        r = bytearray(reads[i])
        p = int(rng.integers(0, len(r)))
        r[p:p + 9] = b"N" * len(r[p:p + 9])
        reads[i] = bytes(r)
    text = ql.make_fastq(reads, quals)
    metas, payload, nb, runs, (qm, qp) = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, non_acgt="keep",
                                                               qualities="keep")
    assert len(runs) > 100 and [ql.meta_dict(m) for m in qm] == ql.sections(text, BR)[0]
    _unpack(ctx, metas, payload)
    ctx.set_exceptions(runs, ctx.substitute)
    ctx.set_qualities(qm, qp)
    assert ctx.decode_fasta_unpacked(first_id=1) == ql.fastq_text(list(zip(reads, quals)))


# 10 --------------------------------------------------------------------------------------------
def _fastq_fixed(reads, quals, L, name=b"@r\n"):
    n = len(reads) // L
    nl = np.full((n, 1), 10, np.uint8)
    rec = np.concatenate([np.frombuffer(name, np.uint8)[None, :].repeat(n, 0), reads.reshape(n, L), nl,
                          np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0), quals.reshape(n, L), nl], axis=1)
    return rec.tobytes()


def _fastq_out(reads, quals, L):
    return b"".join(b"@seq.%d\n%s\n+\n%s\n" % (i + 1, bytes(r), bytes(q))
                    for i, (r, q) in enumerate(zip(reads.reshape(-1, L), quals.reshape(-1, L))))


def _encode_file(ctxs, path, tmp_path, tag, mode="keep", **kw):
    with open(tmp_path / (tag + ".dat"), "wb") as f, open(tmp_path / (tag + ".ntcq"), "wb") as q:
        st = nt.encode_file(ctxs, str(path), f.fileno(), threads=4, blocks_per_batch=1, deflate="zlib",
                            qualities=mode, q_fd=q.fileno(), **kw)
    return st, (tmp_path / (tag + ".ntcq")).read_bytes()


def _decode_file(ctxs, tmp_path, tag):
    with open(tmp_path / (tag + ".fq.out"), "wb") as f:
        st = nt.decode_file(ctxs, str(tmp_path / (tag + ".dat")), f.fileno(), threads=4, blocks_per_batch=1,
                            q_path=str(tmp_path / (tag + ".ntcq")))
    return st, (tmp_path / (tag + ".fq.out")).read_bytes()


def _file_sections(path):
    mode, metas, payload = nt.read_qualities(path)
    return mode, [ql.meta_dict(m) for m in metas], np.frombuffer(payload, dtype="<u8")


def test_files_round_trip(env, tmp_path):
    import gzip
    genome, _, ctx = env
    ctx2 = nt.GpuContext(0)
    ctx2.share_index(ctx)
    try:
        n, L = 140_000, 40
        rng = np.random.default_rng(10)
        reads = nt.synth_reads(genome, 9, 0, n, L, 10_000)
        quals = np.frombuffer(b"#-<F", np.uint8)[rng.integers(0, 4, n * L)]
        quals[70_000 * L:] = ord("F")  # block 2 has one symbol: a section without a member
        text = _fastq_fixed(reads, quals, L)
        (tmp_path / "r.fq").write_bytes(text)
        with gzip.open(tmp_path / "r.fq.gz", "wb", compresslevel=1) as f:
            f.write(text)
        with open(tmp_path / "plainest.dat", "wb") as f:  # today's call, no option at all
            nt.encode_file([ctx], str(tmp_path / "r.fq"), f.fileno(), threads=4, blocks_per_batch=1, deflate="zlib")
        exp_m, exp_w = ql.sections(text, 65536)
        assert [m["width"] for m in exp_m] == [2, 2, 0]
        side = {}
        for tag, path, ctxs in (("plain", "r.fq", [ctx]), ("gz", "r.fq.gz", [ctx]), ("two", "r.fq", [ctx, ctx2])):
            st, side[tag] = _encode_file(ctxs, tmp_path / path, tmp_path, tag)
            assert st["reads"] == n and st["dropped_blocks"] == 0 and st["blocks"] == 3 and st["gpu_parsed"] > 0
            assert (tmp_path / (tag + ".dat")).read_bytes() == (tmp_path / "plainest.dat").read_bytes()
            mode, metas, words = _file_sections(tmp_path / (tag + ".ntcq"))
            assert mode == 1 and metas == exp_m and np.array_equal(words, exp_w)
            assert st["q"]["sections"] == 3 and st["q"]["quals"] == n * L
            assert st["q"]["packed_bytes"] == 8 * len(exp_w) and 0 < st["q"]["deflated_bytes"]
            std, out = _decode_file(ctxs, tmp_path, tag)
            assert std["reads"] == n and out == _fastq_out(reads, quals, L)
        assert side["plain"] == side["gz"] == side["two"]
        assert ctx.get_option("qualities") == 0 and ctx2.get_option("qualities") == 0
        # a side file with a section too few, and one too many, belongs to another encoding
        raw = side["plain"]
        last = len(raw) - 24 - 1  # the last section: width 0, its header and one alphabet byte
        (tmp_path / "short.ntcq").write_bytes(raw[:last])
        (tmp_path / "long.ntcq").write_bytes(raw + raw[last:])
        for name in ("short", "long"):
            with open(tmp_path / "bad.out", "wb") as f, pytest.raises(nt.NtcError) as e:
                nt.decode_file([ctx], str(tmp_path / "plain.dat"), f.fileno(), threads=4, blocks_per_batch=1,
                               q_path=str(tmp_path / (name + ".ntcq")))
            assert e.value.code == FORMAT and "qualities" in str(e.value)
    finally:
        ctx2.close()


def test_files_with_non_acgt_keep_and_bin8(env, tmp_path):
    genome, _, ctx = env
    n, L = 70_000, 40
    rng = np.random.default_rng(11)
    reads = nt.synth_reads(genome, 9, 0, n, L, 10_000).copy().reshape(n, L)
    reads[::9, 3:7] = ord("N")
    reads = reads.reshape(-1)
    quals = rng.integers(33, 75, n * L).astype(np.uint8)
    (tmp_path / "r.fq").write_bytes(_fastq_fixed(reads, quals, L))
    with open(tmp_path / "b.dat", "wb") as f, open(tmp_path / "b.ntcq", "wb") as q, open(tmp_path / "b.ntcx", "wb") as x:
        st = nt.encode_file([ctx], str(tmp_path / "r.fq"), f.fileno(), threads=4, blocks_per_batch=1,
                            non_acgt="keep", nx_fd=x.fileno(), qualities="bin8", q_fd=q.fileno())
    assert st["nx"]["runs"] == len(range(0, n, 9)) and st["q"]["sections"] == 2
    mode, metas, _ = _file_sections(tmp_path / "b.ntcq")
    assert mode == 2 and [m["n_syms"] for m in metas] == [9, 9]
    with open(tmp_path / "b.out", "wb") as f:
        nt.decode_file([ctx], str(tmp_path / "b.dat"), f.fileno(), threads=4, blocks_per_batch=1,
                       nx_path=str(tmp_path / "b.ntcx"), q_path=str(tmp_path / "b.ntcq"))
    assert (tmp_path / "b.out").read_bytes() == _fastq_out(reads, ql.mode_table("bin8")[quals], L)


def test_files_drop_a_section_with_its_block(env, tmp_path):
    """A leading block of 65,536 reads of 8 bases has no long record and is dropped (SURVEY
    App. B.3), as in test_files_renumber_past_a_dropped_block: its section is not written,
    and the rest still round-trips."""
    genome, _, ctx = env
    rng = np.random.default_rng(12)
    n0, L0, n, L = 65_536, 8, 70_000, 40
    head = nt.synth_reads(genome, 10, 0, n0, L0, 0)
    reads = nt.synth_reads(genome, 9, 0, n, L, 10_000)
    hq = np.frombuffer(b"!~", np.uint8)[rng.integers(0, 2, n0 * L0)]
    quals = np.frombuffer(b"#-<FI", np.uint8)[rng.integers(0, 5, n * L)]
    (tmp_path / "d.fq").write_bytes(_fastq_fixed(head, hq, L0) + _fastq_fixed(reads, quals, L))
    st, _ = _encode_file([ctx], tmp_path / "d.fq", tmp_path, "d")
    assert st["reads"] == n0 + n and st["dropped_blocks"] == 1 and st["blocks"] == 2 and st["q"]["sections"] == 2
    mode, metas, words = _file_sections(tmp_path / "d.ntcq")
    exp_m, exp_w = ql.sections(_fastq_fixed(reads, quals, L), 65536)
    assert metas == exp_m and np.array_equal(words, exp_w) and metas[0]["alphabet"] == b"#-<FI"
    std, out = _decode_file([ctx], tmp_path, "d")
    assert std["reads"] == n and out == _fastq_out(reads, quals, L)


@pytest.mark.parametrize("case", ["blank_line", "fasta", "host_parse"])
def test_files_without_a_gpu_text_path_are_unsupported(env, tmp_path, case):
    genome, _, ctx = env
    n, L = 300, 40
    reads = nt.synth_reads(genome, 9, 0, n, L, 0)
    text = _fastq_fixed(reads, np.full(n * L, ord("I"), np.uint8), L)
    kw = {}
    if case == "blank_line":
        cut = text.index(b"@r\n", len(text) // 2)
        text = text[:cut] + b"\n" + text[cut:]
    elif case == "fasta":
        text = b"".join(b">r\n%s\n" % bytes(r) for r in reads.reshape(n, L))
    else:
        kw["host_parse"] = True
    (tmp_path / "u.fq").write_bytes(text)
    with pytest.raises(nt.NtcError) as e:
        _encode_file([ctx], tmp_path / "u.fq", tmp_path, "u", **kw)
    assert e.value.code == UNSUPPORTED and "qualities: " in str(e.value)
    assert {"blank_line": "blank line", "fasta": "not FASTQ", "host_parse": "host_parse"}[case] in str(e.value)
    if case == "blank_line":
        assert e.value.bad_read == 0  # the batch that holds the line starts at read 0
    with open(tmp_path / "ok.dat", "wb") as f:  # and each passes where the qualities are dropped
        assert nt.encode_file([ctx], str(tmp_path / "u.fq"), f.fileno(), threads=4, **kw)["reads"] == n
    assert ctx.get_option("qualities") == 0
