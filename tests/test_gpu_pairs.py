"""Paired-end reads on the GPU (pairs.hip): the weave of two mate texts, the mate check, the
split on decode, through the calls, the file pipelines and the native command line.

The existing single-file path is the reference for everything downstream: a paired encode must
give byte for byte what ntc_encode_pack_fastq gives on the interleaved text, and a paired
decode exactly the split of the plain decode's text.  The checker is pair_lib.py (plain Python)."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import names_lib as nl
import ntcomp_amd as nt
import pair_lib as pl

pytestmark = pytest.mark.gpu
INVALID_ARG, CAPACITY, FORMAT, UNSUPPORTED = 1, 5, 8, 10
BR = 128
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
ALL = dict(non_acgt="keep", qualities="keep", names="keep", digests=True)


@pytest.fixture(scope="module")
def env():
    genome = nt.synth_genome(7, 20_000)
    ix = nt.Index.build([genome.tobytes()], 31)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    yield genome, ix, ctx
    ctx.close()


@pytest.fixture()
def paired(env):
    ctx = env[2]
    ctx.paired = "ids"
    yield ctx
    ctx.paired = "off"


def _blob(metas):
    return b"".join(ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m)) for m in metas)


def _flat(out):
    """an encode call's result as comparable bytes: metas, payload, bases, runs, the sections"""
    metas, payload, nb, runs, (qm, qp), (nm, npay), dg = out
    return (_blob(metas), payload, nb, runs.tobytes(), _blob(qm), qp, _blob(nm), npay, _blob(dg))


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


def _mates(rng, genome, n_pairs, lo=1, hi=300, edge=True):
    """(names1, reads1, quals1), (names2, reads2, quals2): agreeing names of every length class,
    read lengths that differ between the mates"""
    ids = [b"p%d:" % p + bytes(rng.integers(65, 91, int(rng.integers(0, 30)), dtype=np.uint8)) for p in range(n_pairs)]
    if edge:  # (pairs 2 mod 3 carry no suffix: these are the names' lengths)
        for p, ln in zip((2, 5, 8, 11, 14, 17), (0, 1, 63, 64, 65, 200)):
            ids[p] = bytes(rng.integers(65, 91, ln, dtype=np.uint8))
    n1 = [i + (b"/1" if p % 3 == 0 else b" 1:N:0:ACGT" if p % 3 == 1 else b"") for p, i in enumerate(ids)]
    n2 = [i + (b"/2" if p % 3 == 0 else b" 2:N:0:ACGT" if p % 3 == 1 else b"") for p, i in enumerate(ids)]
    sides = []
    for names in (n1, n2):
        reads = _reads(rng, genome, n_pairs, lo, hi)
        sides.append((names, reads, [bytes(rng.integers(33, 75, len(r), dtype=np.uint8)) for r in reads]))
    return sides


@pytest.fixture(scope="module")
def batch(env):
    """224 pairs = 3.5 blocks of 128 reads; the texts in LF"""
    rng = np.random.default_rng(20)
    return _mates(rng, env[0], 224)


# 1 weave equality ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["lf", "crlf", "no_nl_1", "no_nl_2", "no_nl_both"])
def test_weave_equals_the_interleaved_call(paired, batch, shape):
    s1, s2 = batch
    eol = b"\r\n" if shape == "crlf" else b"\n"
    t1 = nl.make_fastq(*s1, eol=eol, last_newline=shape not in ("no_nl_1", "no_nl_both"))
    t2 = nl.make_fastq(*s2, eol=eol, last_newline=shape not in ("no_nl_2", "no_nl_both"))
    assert {len(n) for n in s1[0]} >= {0, 1, 63, 64, 65, 200} <= {len(n) for n in s2[0]}
    for t in (t1, t2):  # record sizes and source alignments: every residue mod 16
        sizes = [len(x) for x in pl._records(t, 4)]
        assert {s % 16 for s in sizes} == set(range(16)) == {int(o) % 16 for o in np.cumsum(sizes)}
    assert {len(r) for r in s1[1] + s2[1]} >= {1, 300} and sum(len(a) != len(b) for a, b in zip(s1[1], s2[1])) > 200
    woven = pl.weave(t1, t2)
    ref = _flat(paired.encode_pack_fastq(woven, 448, block_reads=BR, **ALL))
    got = _flat(paired.encode_pack_fastq_paired(t1, t2, 224, block_reads=BR, **ALL))
    assert got == ref
    assert len(ref[0]) == 4 * ctypes.sizeof(nt.BlockMeta) and len(ref[3]) > 0  # 3.5 blocks, exception runs
    paired.paired = "off"  # and the plain call on the same text: the option changes no byte
    assert _flat(paired.encode_pack_fastq(woven, 448, block_reads=BR, **ALL)) == ref


# 2 small counts --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pairs", [0, 1, 63, 64, 65])
def test_small_counts(env, paired, n_pairs):
    rng = np.random.default_rng(30 + n_pairs)
    s1, s2 = _mates(rng, env[0], n_pairs, 20, 60, edge=False) if n_pairs else (([], [], []), ([], [], []))
    t1, t2 = nl.make_fastq(*s1), nl.make_fastq(*s2)
    got = paired.encode_pack_fastq_paired(t1, t2, n_pairs, block_reads=BR, **ALL)
    assert _flat(got) == _flat(paired.encode_pack_fastq(pl.weave(t1, t2), 2 * n_pairs, block_reads=BR, **ALL))
    assert got[2] == sum(len(r) for r in s1[1] + s2[1])


def test_one_pair_of_one_base_reads_without_names(paired):
    t1, t2 = b"@\nA\n+\nI\n", b"@\nC\n+\nJ"
    got = paired.encode_pack_fastq_paired(t1, t2, 1, block_reads=2, **ALL)
    assert _flat(got) == _flat(paired.encode_pack_fastq(b"@\nA\n+\nI\n@\nC\n+\nJ\n", 2, block_reads=2, **ALL))
    assert got[2] == 2


# 3 count mismatch -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_fewer", "one_more", "three_lines", "text1_short", "no_pairs"])
def test_count_mismatch(env, paired, case):
    rng = np.random.default_rng(40)
    s1, s2 = _mates(rng, env[0], 70, 20, 60, edge=False)
    t1, t2 = nl.make_fastq(*s1), nl.make_fastq(*s2)
    paired.encode_pack_fastq_paired(t1, t2, 70, block_reads=BR, **ALL)  # sections that must not survive
    assert paired.names()[0]
    recs = pl._records(t2, 4)
    n = 70
    if case == "one_fewer":
        t2 = b"".join(recs[:-1])
    elif case == "one_more":
        t2 = t2 + recs[0]
    elif case == "three_lines":
        t2 = t2[:t2.rindex(b"\n", 0, len(t2) - 1) + 1]
    elif case == "text1_short":
        t1 = b"".join(pl._records(t1, 4)[:-1])
    else:
        n = 0
    with pytest.raises(nt.NtcError) as e:
        paired.encode_pack_fastq_paired(t1, t2, n, block_reads=BR, **ALL)
    assert e.value.code == FORMAT and "mate texts hold different record counts" in str(e.value)
    assert paired.names() == ([], b"") and paired.qualities() == ([], b"") and paired.encode_digests() == []
    assert len(paired.exceptions()) == 0


# 4 the mate check --------------------------------------------------------------------------------
def _texts(s1, s2):
    return nl.make_fastq(*s1), nl.make_fastq(*s2)


@pytest.mark.parametrize("bad", [(0,), (64,), (223,), (100, 31), (223, 64, 65)])
def test_mate_check(paired, batch, bad):
    s1, s2 = batch
    names2 = list(s2[0])
    for p in bad:
        names2[p] = names2[p][:2] + b"#" + names2[p][2:]
    assert pl.first_bad_pair(s1[0], names2) == min(bad)
    t1, t2 = _texts(s1, (names2, s2[1], s2[2]))
    woven = pl.weave(t1, t2)
    for call in (lambda: paired.encode_pack_fastq_paired(t1, t2, 224, block_reads=BR, **ALL),
                 lambda: paired.encode_pack_fastq(woven, 448, block_reads=BR, **ALL)):
        with pytest.raises(nt.NtcError) as e:
            call()
        assert e.value.code == FORMAT and e.value.bad_read == 2 * min(bad) and "mates" in str(e.value)
        assert paired.names() == ([], b"") and paired.encode_digests() == []
    paired.paired = "nocheck"  # mode 2 accepts the same texts
    got = _flat(paired.encode_pack_fastq_paired(t1, t2, 224, block_reads=BR, **ALL))
    assert got == _flat(paired.encode_pack_fastq(woven, 448, block_reads=BR, **ALL))


def test_a_clean_batch_passes_and_the_rule_holds_on_the_device(paired, batch):
    s1, s2 = batch
    assert pl.first_bad_pair(s1[0], s2[0]) is None
    paired.encode_pack_fastq_paired(*_texts(s1, s2), 224, block_reads=BR, non_acgt="mask")
    x = b"x" * 70
    cases = [(b"x/1", b"x/2"), (b"x 1:N:0:A", b"x 2:N:0:A"), (b"same", b"same"), (b"", b""), (b"/1", b"/2"),
             (b"x/1", b"x"), (b"x/2", b"x/1"), (b"abc", b"abcd"), (b"abcd", b"abc"), (b"x\t1", b"x\t2"), (b"x\tq", b"x y"),
             (x[:63] + b"a" + x[:5], x[:63] + b"b" + x[:5]), (x[:64] + b"a", x[:64] + b"b"), (x[:65] + b"a", x[:65] + b"b"),
             (x + b"/1", x + b"/2"), (x[:62] + b"/1", x[:62] + b"/2"), (x[:63] + b"/1", x[:63] + b"/2"), (b"a/1", b"b/2"),
             (b"a/1 c", b"a/2\td")]
    for i, (a, b) in enumerate(cases):
        n1, n2 = [b"ok"] * len(cases), [b"ok"] * len(cases)
        n1[i], n2[i] = a, b
        reads = [b"ACGTACGTAC"] * len(cases)
        t1, t2 = nl.make_fastq(n1, reads), nl.make_fastq(n2, reads, eol=b"\r\n")
        if pl.mates_agree(a, b):
            paired.encode_pack_fastq_paired(t1, t2, len(cases), block_reads=BR)
        else:
            with pytest.raises(nt.NtcError) as e:
                paired.encode_pack_fastq_paired(t1, t2, len(cases), block_reads=BR)
            assert e.value.code == FORMAT and e.value.bad_read == 2 * i, (a, b)


def test_argument_checks(env, paired, batch):
    _, _, ctx = env
    t1, t2 = _texts(*batch)
    woven = pl.weave(t1, t2)
    for n, br in ((447, BR), (448, BR + 1)):
        with pytest.raises(nt.NtcError) as e:
            ctx.encode_pack_fastq(woven, n, block_reads=br)
        assert e.value.code == INVALID_ARG
    with pytest.raises(nt.NtcError) as e:
        ctx.encode_pack_fastq_paired(t1, t2, 224, block_reads=BR + 1)
    assert e.value.code == INVALID_ARG
    for v in (-1, 3):
        with pytest.raises(nt.NtcError) as e:
            ctx.set_option("paired", v)
        assert e.value.code == INVALID_ARG
    assert ctx.paired == 1
    ctx.paired = "off"
    with pytest.raises(nt.NtcError) as e:
        ctx.encode_pack_fastq_paired(t1, t2, 224, block_reads=BR)
    assert e.value.code == INVALID_ARG
    with pytest.raises(nt.NtcError) as e:
        ctx.pair_split()
    assert e.value.code == INVALID_ARG
    # bytes1 + bytes2 + 2 must stay under 4 GiB: refused before a byte is read
    ctx.paired = "ids"
    metas = (nt.BlockMeta * 1)()
    out, used, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int64()
    buf = np.zeros(16, dtype=np.uint8)
    rc = ctx.L.ntc_encode_pack_fastq_paired(ctx.h, buf.ctypes.data, (1 << 31) - 1, buf.ctypes.data, 1 << 31, 2, 2, metas,
                                            ctypes.byref(out), ctypes.byref(used), None, ctypes.byref(bad))
    assert rc == CAPACITY


# 5 the split -------------------------------------------------------------------------------------
def _unpack(ctx, metas, payload):
    arr = (nt.BlockMeta * len(metas))(*metas)
    ok, nr, nb = ctx.unpack(arr, payload, len(metas))
    assert ok == len(metas)
    return nr, nb


@pytest.fixture(scope="module")
def ragged(env):
    """55 pairs, ragged reads with a one-base read; ids cross 9 -> 10 and 99 -> 100"""
    genome, _, ctx = env
    rng = np.random.default_rng(50)
    s1, s2 = _mates(rng, genome, 55, 1, 120)
    t1, t2 = _texts(s1, s2)
    ctx.paired = "ids"
    try:
        enc = ctx.encode_pack_fastq_paired(t1, t2, 55, block_reads=BR, **ALL)
    finally:
        ctx.paired = "off"
    return enc, pl.weave(t1, t2)


@pytest.mark.parametrize("fmt", ["fasta", "fastq", "named_fasta", "named_fastq"])
def test_split(env, ragged, fmt):
    _, _, ctx = env
    (metas, payload, nb, runs, (qm, qp), (nm, npay), dg), woven = ragged
    texts = []
    for mode in ("off", "ids"):
        ctx.paired = mode
        try:
            _unpack(ctx, metas, payload)
            if fmt.startswith("named"):
                ctx.set_names(nm, npay)
            if fmt.endswith("fastq"):
                ctx.set_qualities(qm, qp)
            ctx.set_exceptions(runs, ctx.substitute)
            ctx.decode_set_digests(dg)
            need = ctypes.c_uint64()  # the capacity-0 size query (it keeps the sections): the sum of the parts
            assert ctx.L.ntc_decode_fasta_unpacked(ctx.h, 1, None, 0, ctypes.byref(need)) == CAPACITY
            texts.append(ctx.decode_fasta_unpacked(first_id=1))
            if mode == "ids":
                assert ctx.pair_split() == len(texts[1][0])
                assert need.value == len(texts[1][0]) + len(texts[1][1]) == len(texts[0])
        finally:
            ctx.paired = "off"
    whole, parts = texts
    assert parts == pl.split(whole, 4 if fmt.endswith("fastq") else 2)
    if fmt == "named_fastq":
        assert whole == woven
    if fmt == "fasta":
        assert parts[0].startswith(b">seq.1\n") and b">seq.9\n" in parts[0] and b">seq.11\n" in parts[0]
        assert parts[1].startswith(b">seq.2\n") and b">seq.10\n" in parts[1] and b">seq.100\n" in parts[1]


def test_split_through_ntc_decode_fasta(env, paired):
    genome, _, ctx = env
    rng = np.random.default_rng(51)
    reads = _reads(rng, genome, 10, 31, 90)
    bases, offs = nt.pack_reads([r.replace(b"N", b"A") for r in reads])
    ctx.paired = "off"
    recs, _ = ctx.encode(bases, offs)
    out = np.zeros(len(bases) + 20 * 10, dtype=np.uint8)
    got = []
    for mode in (0, 1):
        ctx.paired = mode
        n = ctypes.c_uint64()
        rc = ctx.L.ntc_decode_fasta(ctx.h, recs.ctypes.data, len(recs), 10, len(bases), 95, out.ctypes.data, len(out),
                                    ctypes.byref(n))
        assert rc == 0
        got.append(out[:n.value].tobytes())
    assert got[1] == b"".join(pl.split(got[0], 2)) and ctx.pair_split() == len(pl.split(got[0], 2)[0])
    assert b">seq.99\n" in got[0] and b">seq.100\n" in got[0]


def test_split_refusals(env, ragged):
    _, _, ctx = env
    (metas, payload, nb, runs, (qm, qp), (nm, npay), dg), _ = ragged
    rng = np.random.default_rng(52)
    odd = nl.make_fastq([b"n"] * 3, _reads(rng, env[0], 3, 31, 60))
    m3, p3, _ = ctx.encode_pack_fastq(odd.replace(b"N", b"A"), 3, block_reads=BR)
    ctx.paired = "ids"
    try:
        _unpack(ctx, m3, p3)
        with pytest.raises(nt.NtcError) as e:  # an odd read count
            ctx.decode_fasta_unpacked(first_id=1)
        assert e.value.code == FORMAT
        with pytest.raises(nt.NtcError):
            ctx.pair_split()
        # a damaged name section still ends in its status, with two empty parts
        bad = bytearray(npay)
        bad[0:2] = (4096).to_bytes(2, "little")
        _unpack(ctx, metas, payload)
        ctx.set_names(nm, bytes(bad))
        with pytest.raises(nt.NtcError) as e:
            ctx.decode_fasta_unpacked(first_id=1)
        assert e.value.code == FORMAT and ctx.pair_split() == 0
        ctx.set_names(nm, npay)  # and the good section still decodes, split
        a, b = ctx.decode_fasta_unpacked(first_id=1)
        assert a.count(b">") == b.count(b">") == 55
        ctx.set_option("discard_text", 1)  # nothing is split where no text is wanted
        try:
            need = ctypes.c_uint64()
            assert ctx.L.ntc_decode_fasta_unpacked(ctx.h, 1, None, 0, ctypes.byref(need)) == 0
            assert need.value == sum(len(b">seq.%d\n" % (i + 1)) for i in range(110)) + nb + 110  # (the sections are used up)
            with pytest.raises(nt.NtcError):
                ctx.pair_split()
        finally:
            ctx.set_option("discard_text", 0)
    finally:
        ctx.paired = "off"


# 6 the default path ------------------------------------------------------------------------------
def test_a_plain_call_after_a_paired_one_equals_a_fresh_context(env, batch):
    _, ix, ctx = env
    t1, t2 = _texts(*batch)
    woven = pl.weave(t1, t2)
    ctx.paired = "ids"
    ctx.encode_pack_fastq_paired(t1, t2, 224, block_reads=BR, **ALL)
    ctx.paired = "off"
    after = ctx.encode_pack_fastq(woven, 448, block_reads=BR, **ALL)
    odd = woven[:len(b"".join(pl._records(woven, 4)[:447]))]
    after_odd = ctx.encode_pack_fastq(odd, 447, block_reads=BR - 1, **ALL)  # odd counts are fine again
    _unpack(ctx, after[0], after[1])
    text_after = ctx.decode_fasta_unpacked(first_id=1)
    fresh = nt.GpuContext(0)
    try:
        fresh.share_index(ctx)
        assert _flat(fresh.encode_pack_fastq(woven, 448, block_reads=BR, **ALL)) == _flat(after)
        assert _flat(fresh.encode_pack_fastq(odd, 447, block_reads=BR - 1, **ALL)) == _flat(after_odd)
        _unpack(fresh, after[0], after[1])
        assert fresh.decode_fasta_unpacked(first_id=1) == text_after and isinstance(text_after, bytes)
    finally:
        fresh.close()


# 7 the file pipelines ------------------------------------------------------------------------------
SIDES = ("dat", "ntcx", "ntcq", "ntcn", "ntcd")


def _encode_files(ctxs, tmp_path, tag, in_path, **kw):
    fds = {s: open(tmp_path / f"{tag}.{s}", "wb") for s in SIDES}
    try:
        st = nt.encode_file(ctxs, str(in_path), fds["dat"].fileno(), threads=4, blocks_per_batch=1, deflate="zlib",
                            non_acgt="keep", nx_fd=fds["ntcx"].fileno(), qualities="keep", q_fd=fds["ntcq"].fileno(),
                            names="keep", n_fd=fds["ntcn"].fileno(), d_fd=fds["ntcd"].fileno(), **kw)
    finally:
        for f in fds.values():
            f.close()
    return st, {s: (tmp_path / f"{tag}.{s}").read_bytes() for s in SIDES}


@pytest.fixture(scope="module")
def mate_files(env, tmp_path_factory):
    """40,000 pairs of 30-60 bp reads: one whole block of 65,536 reads and a part"""
    genome, _, ctx = env
    d = tmp_path_factory.mktemp("mates")
    rng = np.random.default_rng(60)
    s1, s2 = _mates(rng, genome, 40_000, 30, 60, edge=False)
    t1, t2 = _texts(s1, s2)
    (d / "r1.fq").write_bytes(t1)
    (d / "r2.fq").write_bytes(t2)
    (d / "both.fq").write_bytes(pl.weave(t1, t2))
    for name, t in (("r1.fq.gz", t1), ("r2.fq.gz", t2)):
        with gzip.open(d / name, "wb", compresslevel=1) as f:
            f.write(t)
    ref = _encode_files([ctx], d, "ref", d / "both.fq")  # the single-file encode of the interleaved file
    assert ref[0]["reads"] == 80_000 and ref[0]["blocks"] == 2 and ref[0]["gpu_parsed"] == 2
    return d, t1, t2, ref[1]


@pytest.mark.parametrize("n_ctx", [1, 2])
@pytest.mark.parametrize("kinds", ["plain+plain", "gzip+gzip", "plain+gzip"])
def test_pipeline_equals_the_interleaved_file(env, mate_files, tmp_path, kinds, n_ctx):
    _, _, ctx = env
    d, t1, t2, ref = mate_files
    ctxs = [ctx]
    if n_ctx == 2:
        ctxs.append(nt.GpuContext(0))
        ctxs[1].share_index(ctx)
    try:
        k1, k2 = kinds.split("+")
        st, got = _encode_files(ctxs, tmp_path, "p", d / ("r1.fq" if k1 == "plain" else "r1.fq.gz"),
                                mate_path=str(d / ("r2.fq" if k2 == "plain" else "r2.fq.gz")))
        assert st["reads"] == 80_000 and st["blocks"] == 2 and st["gpu_parsed"] == 2
        assert st["p"] == dict(pairs=40_000, bytes1=len(t1), bytes2=len(t2), mode=1)
        for s in SIDES:
            assert got[s] == ref[s], s
        assert all(c.paired == 0 for c in ctxs)
        if kinds != "plain+plain":
            return
        side = dict(nx_path=str(tmp_path / "p.ntcx"), q_path=str(tmp_path / "p.ntcq"), n_path=str(tmp_path / "p.ntcn"),
                    d_path=str(tmp_path / "p.ntcd"))
        with open(tmp_path / "o1.fq", "wb") as f1, open(tmp_path / "o2.fq", "wb") as f2:
            sd = nt.decode_file(ctxs, str(tmp_path / "p.dat"), f1.fileno(), threads=4, blocks_per_batch=1, out_fd2=f2.fileno(),
                                pair_mode="ids", **side)
        assert (tmp_path / "o1.fq").read_bytes() == t1 and (tmp_path / "o2.fq").read_bytes() == t2
        assert sd["p"] == dict(pairs=40_000, bytes1=len(t1), bytes2=len(t2), mode=1) and sd["reads"] == 80_000
        sv = nt.decode_file(ctxs, str(tmp_path / "p.dat"), -1, threads=4, blocks_per_batch=1, pair_mode="ids", **side)  # verify
        assert sv["reads"] == 80_000 and sv["d"]["sections"] == 2
        with open(tmp_path / "o1.fa", "wb") as f1, open(tmp_path / "o2.fa", "wb") as f2:  # without names: the archive's numbering
            nt.decode_file(ctxs, str(tmp_path / "p.dat"), f1.fileno(), threads=4, blocks_per_batch=1, out_fd2=f2.fileno(),
                           pair_mode="nocheck")
        assert (tmp_path / "o1.fa").read_bytes().startswith(b">seq.1\n") and (tmp_path / "o2.fa").read_bytes().startswith(b">seq.2\n")
        with open(tmp_path / "x.fa", "wb") as f1, pytest.raises(nt.NtcError) as e:
            nt.decode_file(ctxs, str(tmp_path / "p.dat"), f1.fileno(), pair_mode="ids")  # no second output
        assert e.value.code == INVALID_ARG
    finally:
        for c in ctxs[1:]:
            c.close()


def test_pipeline_interleaved_input_is_checked(env, mate_files, tmp_path):
    _, _, ctx = env
    d, t1, t2, ref = mate_files
    st, got = _encode_files([ctx], tmp_path, "i", d / "both.fq", pair_mode="ids")
    assert all(got[s] == ref[s] for s in SIDES) and st["p"]["pairs"] == 40_000
    recs = pl._records(pl.weave(t1, t2), 4)
    (tmp_path / "odd.fq").write_bytes(b"".join(recs[:-1]))
    with pytest.raises(nt.NtcError) as e:
        _encode_files([ctx], tmp_path, "o", tmp_path / "odd.fq", pair_mode="nocheck")
    assert e.value.code == FORMAT and "odd number of reads" in str(e.value)
    recs[2 * 33_000 + 1] = recs[2 * 33_000 + 1].replace(b"@p", b"@q", 1)
    (tmp_path / "bad.fq").write_bytes(b"".join(recs))
    with pytest.raises(nt.NtcError) as e:
        _encode_files([ctx], tmp_path, "b", tmp_path / "bad.fq", pair_mode="ids")
    assert e.value.code == FORMAT and e.value.bad_read == 66_000 and "mates" in str(e.value)
    assert _encode_files([ctx], tmp_path, "n", tmp_path / "bad.fq", pair_mode="nocheck")[0]["reads"] == 80_000


@pytest.mark.parametrize("case", ["one_short", "one_short_gz", "slipped", "host_parse", "fasta", "blank_line"])
def test_pipeline_refusals(env, mate_files, tmp_path, case):
    _, _, ctx = env
    d, t1, t2, _ = mate_files
    recs = pl._records(t2, 4)
    kw, code, word, bad = {}, FORMAT, "mate files hold different numbers of records", None
    if case == "one_short":
        (tmp_path / "m.fq").write_bytes(b"".join(recs[:-1]))
    elif case == "one_short_gz":
        with gzip.open(tmp_path / "m.fq", "wb", compresslevel=1) as f:
            f.write(b"".join(recs[:-1]))
    elif case == "slipped":  # its first record removed and one appended: every pair is off by one
        (tmp_path / "m.fq").write_bytes(b"".join(recs[1:] + recs[:1]))
        word, bad = "mates", 0
    elif case == "host_parse":
        (tmp_path / "m.fq").write_bytes(t2)
        kw, code, word = dict(host_parse=True), UNSUPPORTED, "pairs: host_parse"
    elif case == "fasta":
        (tmp_path / "m.fq").write_bytes(b">a\nACGT\n")
        code, word = UNSUPPORTED, "pairs: the mate input is not FASTQ"
    else:
        (tmp_path / "m.fq").write_bytes(b"".join(recs[:100]) + b"\n" + b"".join(recs[100:]))
        code, word = UNSUPPORTED, "pairs: a blank line"
    with pytest.raises(nt.NtcError) as e:
        if case in ("host_parse", "fasta"):  # (without side files: theirs are refused likewise, and first)
            with open(tmp_path / "r.dat", "wb") as f:
                nt.encode_file([ctx], str(d / "r1.fq"), f.fileno(), threads=4, mate_path=str(tmp_path / "m.fq"), **kw)
        else:
            _encode_files([ctx], tmp_path, "r", d / "r1.fq", mate_path=str(tmp_path / "m.fq"), **kw)
    assert e.value.code == code and word in str(e.value)
    if bad is not None:
        assert e.value.bad_read == bad
    assert ctx.paired == 0


# 8 the native command line ---------------------------------------------------------------------------
def test_native_round_trip(env, tmp_path):
    """R1 and R2 in, R1 and R2 out, byte for byte, from the three side files (and checked
    against the digest file on the way)"""
    genome, ix, _ = env
    rng = np.random.default_rng(70)
    s1, s2 = _mates(rng, genome, 1500, 20, 150, edge=False)
    t1, t2 = _texts(s1, s2)
    (tmp_path / "r1.fq").write_bytes(t1)
    with gzip.open(tmp_path / "r2.fq.gz", "wb", compresslevel=1) as f:
        f.write(t2)
    ix.save(str(tmp_path / "idx"))
    side = ["--exceptions", str(tmp_path / "x.ntcx"), "--quality-file", str(tmp_path / "q.ntcq"),
            "--name-file", str(tmp_path / "n.ntcn"), "--digest-file", str(tmp_path / "d.ntcd")]
    with open(tmp_path / "enc.dat", "wb") as f:
        r = subprocess.run([NATIVE, "encode", "-i", str(tmp_path / "idx"), "--non-acgt", "keep", "--qualities", "keep",
                            "--names", "keep", *side, "--mate-file", str(tmp_path / "r2.fq.gz"), "--stats",
                            str(tmp_path / "r1.fq")], stdout=f, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert b'"pairs": 1500' in r.stderr and b'"mate_check": "ids"' in r.stderr
    assert b'"mate1_bytes": %d' % len(t1) in r.stderr and b'"mate2_bytes": %d' % len(t2) in r.stderr
    with open(tmp_path / "o1.fq", "wb") as f:
        r = subprocess.run([NATIVE, "decode", "-i", str(tmp_path / "idx"), *side, "--mate-out", str(tmp_path / "o2.fq"),
                            "--stats", str(tmp_path / "enc.dat")], stdout=f, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "o1.fq").read_bytes() == t1 and (tmp_path / "o2.fq").read_bytes() == t2
    assert b'"pairs": 1500' in r.stderr
    r = subprocess.run([NATIVE, "verify", "-i", str(tmp_path / "idx"), *side, str(tmp_path / "enc.dat")],
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and b"verify: OK: 1 blocks, 3000 reads" in r.stdout, r.stderr[-2000:]
    # a slipped mate file is caught at its first pair
    (tmp_path / "slip.fq").write_bytes(b"".join(pl._records(t2, 4)[1:] + pl._records(t2, 4)[:1]))
    with open(tmp_path / "bad.dat", "wb") as f:
        r = subprocess.run([NATIVE, "encode", "-i", str(tmp_path / "idx"), "--non-acgt", "mask", "--mate-file",
                            str(tmp_path / "slip.fq"), str(tmp_path / "r1.fq")], stdout=f, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode != 0 and b"mates" in r.stderr and b"(read 1)" in r.stderr
