"""The order-1 rANS coder of the quality sections on the GPU (qrans.hip): the sections
ntc_encode_pack_fastq yields under quality_coder = 1, byte for byte against the checker, their
way back to FASTQ text, what the decoder makes of damaged sections, and the files of the
pipeline.

The checker is independent of the code under test: qrans_lib.py (numpy and plain Python) holds
the counts, the normalisation, the span coder and the file format; qual_lib.py the mode tables
and the alphabet."""
import ctypes
import gzip
import struct

import numpy as np
import pytest

import ntcomp_amd as nt
import qrans_lib as qr
import qual_lib as ql

pytestmark = pytest.mark.gpu
INVALID_ARG, FORMAT = 1, 8
BR = 64  # block_reads
WIDTHS = [(1, 0), (2, 1), (3, 2), (4, 2), (5, 4), (16, 4), (17, 8), (40, 8), (94, 8)]


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


def _encode(ctx, text, n, mode="keep", **kw):
    out = ctx.encode_pack_fastq(text, n, block_reads=BR, qualities=mode, quality_coder="rans", **kw)
    qm, qp = out[-1] if "names" not in kw else out[-2]
    return out, qm, qp


def _check_sections(ctx, text, n, mode="keep"):
    """the sections of the call against the checker: metas, tables, span sizes, streams"""
    out, qm, qp = _encode(ctx, text, n, mode)
    exp_m, exp_p = qr.sections(text, BR, mode)
    got_m = [qr.meta_dict(m) for m in qm]
    assert got_m == exp_m
    for m in exp_m:  # part by part, so that a failure says which
        a, b = m["payload_off"], m["payload_off"] + m["payload_bytes"]
        assert qr.split_body(qp[a:b], m["n_quals"], m["n_syms"]) == qr.split_body(exp_p[a:b], m["n_quals"], m["n_syms"])
    assert qp == exp_p  # and the padding between bodies
    assert ctx.get_option("quality_coder") == 0  # the coder held for that call only
    return out, qm, qp, got_m


def _unpack(ctx, metas, payload):
    arr = (nt.BlockMeta * len(metas))(*metas)
    ok, nr, nb = ctx.unpack(arr, payload, len(metas))
    assert ok == len(metas)
    return nr, nb


def _round_trip(ctx, out, qm, qp, recs, first_id=1, mode="keep"):
    _unpack(ctx, out[0], out[1])
    ctx.set_qualities(qm, qp)
    assert ctx.decode_fasta_unpacked(first_id=first_id) == ql.fastq_text(recs, first_id, mode)


def _anchor(reads, genome):
    """The longest read of every block becomes a piece of the genome: a block needs a long record
    beside its short ones, or the packer drops it."""
    g = genome.tobytes()
    for b in range(0, len(reads), BR):
        i = max(range(b, min(b + BR, len(reads))), key=lambda r: len(reads[r]))
        reads[i] = g[1000 + b:1000 + b + len(reads[i])]
    return reads


def _ragged(genome, rng, n_syms_per_block, n_reads, ends=(63, 1, 0)):
    reads, quals = ql.ragged_batch(rng, n_syms_per_block, BR, n_reads, ends)
    return _anchor(reads, genome), quals


def _sized_batch(genome, rng, totals, n_syms, p=None):
    """blocks of BR reads (the last one may be one read) whose qualities number totals[b]; the
    first read of a block has 120 bases of the genome"""
    reads, quals = [], []
    for b, total in enumerate(totals):
        n = 1 if total < BR else BR
        lens = np.full(n, (total - 120) // (n - 1) if n > 1 else total)
        if n > 1:
            lens[0] = 120
            lens[1:1 + total - lens.sum()] += 1
        alpha = ql.random_alphabet(rng, n_syms[b])
        if p is None:
            q = alpha[rng.integers(0, len(alpha), total)]
            q[rng.permutation(total)[:len(alpha)]] = alpha[:total]
        else:
            q = qr.markov_quals(rng, alpha, total, p)
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, total)]
        at = 0
        for ln in lens:
            reads.append(s[at:at + ln].tobytes())
            quals.append(q[at:at + ln].tobytes())
            at += int(ln)
    return _anchor(reads, genome), quals


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_syms,w", WIDTHS)
def test_sections_ragged_reads(env, n_syms, w):
    """Three and a half blocks of ragged reads (1..300 bases, a read of one base)."""
    _, _, ctx = env
    reads, quals = _ragged(env[0], np.random.default_rng(300 + n_syms), [n_syms] * 4, 3 * BR + BR // 2)
    text = ql.make_fastq(reads, quals)
    out, qm, qp, got = _check_sections(ctx, text, len(reads))
    assert min(len(r) for r in reads) == 1 and got[3]["n_reads"] == BR // 2
    for m in got:
        assert (m["width"], m["n_syms"], m["payload_off"] % 8) == (w, n_syms, 0)
        assert (m["payload_bytes"] == 0) == (n_syms <= 1)
    _round_trip(ctx, out, qm, qp, list(zip(reads, quals)))


# 2 ---------------------------------------------------------------------------------------------
def test_span_boundaries_and_a_block_of_one_quality(env):
    """Blocks that end one quality before a span boundary, on it, one after it, two spans and
    one quality, and a last block of a single quality."""
    _, _, ctx = env
    totals = [2047, 2048, 2049, 4097, 1]
    reads, quals = _sized_batch(env[0], np.random.default_rng(2), totals, [5, 5, 5, 5, 1])
    text = ql.make_fastq(reads, quals)
    out, qm, qp, got = _check_sections(ctx, text, len(reads))
    assert [m["n_quals"] for m in got] == totals and got[-1]["n_reads"] == 1
    assert [qr.n_spans(t) for t in totals] == [1, 1, 2, 3, 1]
    # (the packer drops the block of one short read, App. B.3: the first four come back)
    _round_trip(ctx, (out[0][:4], out[1]), qm[:4], qp, list(zip(reads, quals))[:4 * BR])
    # a block of one quality among two symbols cannot be: one quality is one symbol, no body
    assert got[-1]["payload_bytes"] == 0


# 3 ---------------------------------------------------------------------------------------------
def test_alphabets_are_per_block(env):
    _, _, ctx = env
    reads, quals = _ragged(env[0], np.random.default_rng(3), [2, 17, 1, 40], 4 * BR)
    text = ql.make_fastq(reads, quals)
    out, qm, qp, got = _check_sections(ctx, text, len(reads))
    assert [(m["n_syms"], m["width"]) for m in got] == [(2, 1), (17, 8), (1, 0), (40, 8)]
    assert got[3]["payload_off"] == got[2]["payload_off"]  # the body of one symbol is empty
    _round_trip(ctx, out, qm, qp, list(zip(reads, quals)))


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["crlf", "no_last_newline"])
def test_text_shapes(env, shape):
    _, _, ctx = env
    reads, quals = _ragged(env[0], np.random.default_rng(4), [5, 5], BR + 17, ends=())
    kw = {"eol": b"\r\n"} if shape == "crlf" else {"last_newline": False}
    text = ql.make_fastq(reads, quals, **kw)
    out, qm, qp, got = _check_sections(ctx, text, len(reads))
    assert sum(m["n_quals"] for m in got) == sum(len(q) for q in quals)


def test_bin8(env):
    _, _, ctx = env
    reads, quals = _ragged(env[0], np.random.default_rng(5), [94, 94], BR + 30, ends=())
    text = ql.make_fastq(reads, quals)
    out, qm, qp, got = _check_sections(ctx, text, len(reads), "bin8")
    assert all(m["n_syms"] == 9 for m in got)
    _round_trip(ctx, out, qm, qp, list(zip(reads, quals)), mode="bin8")


def test_markov_batch(env):
    """The source the coder is made for: four symbols that stay with p = 0.9, 64 reads x 150."""
    _, _, ctx = env
    recs = ql.records(qr.markov_fastq(11, 2 * BR, 150))
    text = ql.make_fastq(_anchor([r for r, _ in recs], env[0]), [q for _, q in recs])
    out, qm, qp, got = _check_sections(ctx, text, 2 * BR)
    assert all(m["n_quals"] == BR * 150 and m["n_syms"] == 4 for m in got)
    packed = ql.sections(text, BR)[0]
    assert all(r["payload_bytes"] < p["payload_bytes"] for r, p in zip(got, packed))
    _round_trip(ctx, out, qm, qp, ql.records(text))


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["0x1f", "0x7f", "space"])
def test_errors_name_the_read(env, damage):
    _, _, ctx = env
    reads, quals = _ragged(env[0], np.random.default_rng(6), [4, 4], BR + 20, ends=())
    bad = BR + 11
    reads[bad] = b"ACGTACGTAC"
    quals[bad] = b"IIIIIIIIII"
    if damage == "space":
        reads[bad] = b"ACGT CGTAC"  # 9 bases kept, 10 qualities
    else:
        quals[bad] = b"IIII" + bytes([int(damage, 16)]) + b"IIIII"
    text = ql.make_fastq(reads, quals)
    with pytest.raises(nt.NtcError) as e:
        ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="keep", quality_coder="rans")
    assert e.value.code == FORMAT and e.value.bad_read == bad
    assert ctx.qualities() == ([], b"")


# 6 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded(env):
    """One batch, encoded once: block 1 has three spans of 40 symbols."""
    _, _, ctx = env
    reads, quals = _sized_batch(env[0], np.random.default_rng(7), [3000, 5000, 700], [4, 40, 1])
    text = ql.make_fastq(reads, quals)
    out = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="keep", quality_coder="rans")
    qm, qp = out[-1]
    assert qp == qr.sections(text, BR)[1]
    return reads, quals, out[0], out[1], qm, qp


@pytest.mark.parametrize("first_id", [1, 99_999])
def test_round_trip_to_fastq(env, encoded, first_id):
    _, _, ctx = env
    reads, quals, metas, payload, qm, qp = encoded
    nr, _ = _unpack(ctx, metas, payload)
    assert nr == len(reads)
    ctx.set_qualities(qm, qp)
    assert ctx.decode_fasta_unpacked(first_id=first_id) == ql.fastq_text(list(zip(reads, quals)), first_id)
    fasta = ctx.decode_fasta_unpacked(first_id=first_id)  # the sections were used: FASTA again
    assert fasta == b"".join(b">seq.%d\n%s\n" % (first_id + i, r) for i, r in enumerate(reads))


def test_together_with_non_acgt_keep_and_names_keep(env):
    _, _, ctx = env
    rng = np.random.default_rng(8)
    reads, quals = _ragged(env[0], rng, [8, 8], BR + 20, ends=())
    for i in range(0, len(reads), 7):
        r = bytearray(reads[i])
        p = int(rng.integers(0, len(r)))
        r[p:p + 9] = b"N" * len(r[p:p + 9])
        reads[i] = bytes(r)
    text = ql.make_fastq(reads, quals)
    metas, payload, nb, runs, (qm, qp), (nm, npay) = ctx.encode_pack_fastq(
        text, len(reads), block_reads=BR, non_acgt="keep", qualities="keep", names="keep", quality_coder="rans")
    assert len(runs) > 5 and [qr.meta_dict(m) for m in qm] == qr.sections(text, BR)[0]
    _unpack(ctx, metas, payload)
    ctx.set_exceptions(runs, ctx.substitute)
    ctx.set_qualities(qm, qp)
    ctx.set_names(nm, npay)
    exp = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(reads, quals)))
    assert ctx.decode_fasta_unpacked(first_id=1) == exp


# 7 ---------------------------------------------------------------------------------------------
def _flip_that_breaks_the_final_state(body, m):
    """a stream byte of block m's second span whose flip the checker's decoder refuses: found on
    the CPU, so the final-state check provably fails for this seed"""
    tab, sizes, streams = qr.split_body(body, m.n_quals, m.n_syms)
    at = 2 * (m.n_syms + 1) * m.n_syms + 4 * len(sizes) + sizes[0]
    for k in range(8, sizes[1]):
        st = bytearray(streams[1])
        st[k] ^= 0x01
        if not qr.decode_span(bytes(st), min(qr.SPAN, m.n_quals - qr.SPAN), tab, m.n_syms)[1]:
            return at + k
    raise AssertionError("no flip is refused")


@pytest.mark.parametrize("damage", ["flipped_byte", "sizes_swapped", "n_quals", "section_missing"])
def test_decode_validation(env, encoded, damage):
    """Inputs the decoder must survive: each is NTC_ERR_FORMAT and no text."""
    _, _, ctx = env
    reads, quals, metas, payload, qm, qp = encoded
    qm = [nt.QualMeta.from_buffer_copy(bytes(_blob([m]))) for m in qm]
    qp = bytearray(qp)
    m = qm[1]
    body = bytes(qp[m.payload_off:m.payload_off + m.payload_bytes])
    tab, sizes, streams = qr.split_body(body, m.n_quals, m.n_syms)
    assert len(sizes) == 3 and m.coder == 1
    if damage == "flipped_byte":
        qp[m.payload_off + _flip_that_breaks_the_final_state(body, m)] ^= 0x01
    elif damage == "sizes_swapped":
        assert sizes[0] != sizes[1]
        at = m.payload_off + 2 * (m.n_syms + 1) * m.n_syms
        qp[at:at + 8] = struct.pack("<II", sizes[1], sizes[0])
        damaged = bytes(qp[m.payload_off:m.payload_off + m.payload_bytes])
        assert not qr.decode_body(damaged, m.n_quals, m.n_syms, bytes(m.alphabet))[1]
    elif damage == "n_quals":
        m.n_quals -= 1  # the spans stay three: the host has nothing to say
    else:
        qm = qm[:-1]
    _unpack(ctx, metas, payload)
    ctx.set_qualities(qm, bytes(qp))
    with pytest.raises(nt.NtcError) as e:  # no text comes back
        ctx.decode_fasta_unpacked(first_id=1)
    assert e.value.code == FORMAT
    assert ctx.decode_fasta_unpacked(first_id=1).startswith(b">seq.1\n")  # the sections are gone


def test_set_qualities_refuses_what_the_host_can_see(env, encoded):
    _, _, ctx = env
    reads, quals, metas, payload, qm, qp = encoded
    for what in ("row_sum", "span_size", "coder_mixed", "coder_2"):
        ms = [nt.QualMeta.from_buffer_copy(bytes(_blob([m]))) for m in qm]
        p = bytearray(qp)
        if what == "row_sum":
            p[ms[0].payload_off] ^= 1
        elif what == "span_size":
            p[ms[0].payload_off + 2 * 5 * 4] ^= 1
        elif what == "coder_mixed":
            ms[2].coder = 0
        else:
            for m in ms:
                m.coder = 2
        with pytest.raises(nt.NtcError) as e:
            ctx.set_qualities(ms, bytes(p))
        assert e.value.code == FORMAT, what


# 8 ---------------------------------------------------------------------------------------------
def _fastq_fixed(reads, quals, L, name=b"@r\n"):
    n = len(reads) // L
    nl = np.full((n, 1), 10, np.uint8)
    rec = np.concatenate([np.frombuffer(name, np.uint8)[None, :].repeat(n, 0), reads.reshape(n, L), nl,
                          np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0), quals.reshape(n, L), nl], axis=1)
    return rec.tobytes()


def _fastq_out(reads, quals, L):
    return b"".join(b"@seq.%d\n%s\n+\n%s\n" % (i + 1, bytes(r), bytes(q))
                    for i, (r, q) in enumerate(zip(reads.reshape(-1, L), quals.reshape(-1, L))))


def _encode_file(ctxs, path, tmp_path, tag, coder="rans", mode="keep"):
    for c in ctxs:
        c.quality_coder = coder
    try:
        with open(tmp_path / (tag + ".dat"), "wb") as f, open(tmp_path / (tag + ".ntcq"), "wb") as q:
            st = nt.encode_file(ctxs, str(path), f.fileno(), threads=4, blocks_per_batch=1, deflate="zlib",
                                qualities=mode, q_fd=q.fileno())
    finally:
        for c in ctxs:
            c.quality_coder = "pack"
    return st, (tmp_path / (tag + ".ntcq")).read_bytes()


def _decode_file(ctxs, tmp_path, tag):
    with open(tmp_path / (tag + ".fq.out"), "wb") as f:
        st = nt.decode_file(ctxs, str(tmp_path / (tag + ".dat")), f.fileno(), threads=4, blocks_per_batch=1,
                            q_path=str(tmp_path / (tag + ".ntcq")))
    return st, (tmp_path / (tag + ".fq.out")).read_bytes()


def _check_file_sections(path, quals_by_block, n_reads_by_block):
    """The file's sections against the checker: header, metas, every table (numpy counts of the
    whole block), every span size in place, and the first and the last span's stream of each block
    byte for byte (the plain-Python coder is too slow for blocks of 65,536 reads)."""
    raw = path.read_bytes()
    assert raw[:32] == qr.header("keep")
    mode, metas, pay = nt.read_qualities(path)
    assert mode == 1 and len(metas) == len(quals_by_block)
    at = 32
    for m, q, nr in zip(metas, quals_by_block, n_reads_by_block):
        alphabet = np.unique(q)
        n = len(alphabet)
        assert (m.n_reads, m.n_quals, m.n_syms, m.width, m.coder) == (nr, len(q), n, ql.width(n), 1)
        assert bytes(m.alphabet)[:n] == alphabet.tobytes() and m.payload_off % 8 == 0
        body = pay[m.payload_off:m.payload_off + m.payload_bytes]
        assert raw[at:at + 24] == struct.pack("<QQBBHI", nr, len(q), ql.width(n), n, 0, len(body))
        assert raw[at + 24:at + 24 + n + len(body)] == alphabet.tobytes() + body
        at += 24 + n + len(body)
        if n <= 1:
            assert body == b""
            continue
        syms = np.searchsorted(alphabet, q)
        tab, sizes, streams = qr.split_body(body, len(q), n)
        exp_tab = qr.table(qr.counts(syms, n))
        assert tab == exp_tab and len(sizes) == qr.n_spans(len(q))
        assert len(body) == 2 * (n + 1) * n + 4 * len(sizes) + sum(sizes)
        for j in (0, len(sizes) - 1):
            assert streams[j] == qr.encode_span(syms[j * qr.SPAN:(j + 1) * qr.SPAN], exp_tab, n)
    assert at == len(raw)


def test_files_round_trip(env, tmp_path):
    genome, _, ctx = env
    ctx2 = nt.GpuContext(0)
    ctx2.share_index(ctx)
    try:
        n, L = 140_000, 40
        rng = np.random.default_rng(10)
        reads = nt.synth_reads(genome, 9, 0, n, L, 10_000)
        quals = np.frombuffer(b"#-<F", np.uint8)[rng.integers(0, 4, n * L)]
        quals[131_072 * L:] = ord("F")  # block 2 has one symbol: a section without a body
        text = _fastq_fixed(reads, quals, L)
        (tmp_path / "r.fq").write_bytes(text)
        with gzip.open(tmp_path / "r.fq.gz", "wb", compresslevel=1) as f:
            f.write(text)
        with open(tmp_path / "plainest.dat", "wb") as f:  # no option at all
            nt.encode_file([ctx], str(tmp_path / "r.fq"), f.fileno(), threads=4, blocks_per_batch=1, deflate="zlib")
        st, pack_side = _encode_file([ctx], tmp_path / "r.fq", tmp_path, "pack", coder="pack")
        assert (tmp_path / "pack.dat").read_bytes() == (tmp_path / "plainest.dat").read_bytes()
        assert pack_side[:9] == b"NTCQ" + struct.pack("<IB", 1, 1)  # pack files stay version 1
        side = {}
        for tag, path, ctxs in (("plain", "r.fq", [ctx]), ("gz", "r.fq.gz", [ctx]), ("two", "r.fq", [ctx, ctx2])):
            st, side[tag] = _encode_file(ctxs, tmp_path / path, tmp_path, tag)
            assert st["reads"] == n and st["dropped_blocks"] == 0 and st["blocks"] == 3 and st["gpu_parsed"] > 0
            assert (tmp_path / (tag + ".dat")).read_bytes() == (tmp_path / "plainest.dat").read_bytes()
            assert st["q"]["sections"] == 3 and st["q"]["quals"] == n * L
            assert st["q"]["deflated_bytes"] == len(side[tag]) - 32
            std, out = _decode_file(ctxs, tmp_path, tag)
            assert std["reads"] == n and out == _fastq_out(reads, quals, L)
        assert side["plain"] == side["gz"] == side["two"]
        cut = [0, 65_536 * L, 131_072 * L, n * L]
        _check_file_sections(tmp_path / "plain.ntcq", [quals[a:b] for a, b in zip(cut, cut[1:])],
                             [65_536, 65_536, n - 131_072])
        assert ctx.get_option("qualities") == 0 and ctx2.get_option("qualities") == 0
        # contexts that disagree on the coder
        ctx2.quality_coder = "rans"
        try:
            with open(tmp_path / "x.dat", "wb") as f, open(tmp_path / "x.ntcq", "wb") as q, pytest.raises(nt.NtcError) as e:
                nt.encode_file([ctx, ctx2], str(tmp_path / "r.fq"), f.fileno(), threads=4, blocks_per_batch=1,
                               deflate="zlib", qualities="keep", q_fd=q.fileno())
            assert e.value.code == INVALID_ARG
        finally:
            ctx2.quality_coder = "pack"
    finally:
        ctx2.close()


def test_files_drop_a_section_with_its_block(env, tmp_path):
    """A leading block of 65,536 reads of 8 bases has no long record and is dropped: its section
    is not written, and the rest still round-trips."""
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
    _check_file_sections(tmp_path / "d.ntcq", [quals[:65_536 * L], quals[65_536 * L:]], [65_536, n - 65_536])
    std, out = _decode_file([ctx], tmp_path, "d")
    assert std["reads"] == n and out == _fastq_out(reads, quals, L)


# 9 ---------------------------------------------------------------------------------------------
def test_default_is_untouched(env):
    """Under quality_coder = 0, the default, every output is what qual_lib expects of pack."""
    _, _, ctx = env
    reads, quals = _ragged(env[0], np.random.default_rng(13), [7, 40], BR + 10, ends=())
    text = ql.make_fastq(reads, quals)
    assert ctx.get_option("quality_coder") == 0 and ctx.quality_coder == 0
    m0, p0, nb0 = ctx.encode_pack_fastq(text, len(reads), block_reads=BR)
    for kw in ({}, {"quality_coder": "pack"}):
        m1, p1, nb1, (qm, qp) = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="keep", **kw)
        exp_m, exp_w = ql.sections(text, BR)
        assert [ql.meta_dict(m) for m in qm] == exp_m and qp == exp_w.astype("<u8").tobytes()
        assert all(m.coder == 0 and bytes(m.reserved) == bytes(6) for m in qm)
        assert _blob(m1) == _blob(m0) and p1 == p0 and nb1 == nb0
    m2, p2, nb2, _ = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="keep", quality_coder="rans")
    assert _blob(m2) == _blob(m0) and p2 == p0 and nb2 == nb0  # the records do not depend on the coder
    # the coder is ignored where qualities are dropped, and persists until changed
    ctx.quality_coder = "rans"
    try:
        assert ctx.get_option("quality_coder") == 1
        m3, p3, nb3, (qm, qp) = ctx.encode_pack_fastq(text, len(reads), block_reads=BR, qualities="drop")
        assert (qm, qp) == ([], b"") and _blob(m3) == _blob(m0) and p3 == p0
        assert ctx.get_option("quality_coder") == 1
    finally:
        ctx.quality_coder = "pack"
    with pytest.raises(nt.NtcError) as e:
        ctx.set_option("quality_coder", 2)
    assert e.value.code == INVALID_ARG
