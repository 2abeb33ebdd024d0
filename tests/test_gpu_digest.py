"""Per-block content digests on the GPU (digest.hip): what ntc_encode_pack_fastq and
ntc_encode_pack_batch yield under "digests" 1 against the definition, for every component,
length class and block split; the decode side's verification, its verdicts on damaged records,
damaged digests and missing side files; the "NTCD" file through the pipelines and both command
lines.

The checker is independent of the code under test: digest_lib.py (plain Python)."""
import ctypes
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import digest_lib as dl
import names_lib as nl
import ntcomp_amd as nt
import qual_lib as ql
from oracle_lib import OracleIndex

pytestmark = pytest.mark.gpu
FORMAT, DIGEST = 8, 12
K = 31
# every length class of k_dg_sum: around the 8-byte word, the quarter-wave's 16 words (128
# bytes), kDgLong = 2048 (one length on each side: the workgroup path starts at 2049), and one
# read a workgroup walks for many steps
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049, 70_000]
NX = bytes(nt.NX_SYMBOLS)


@pytest.fixture(scope="module")
def env():
    genome = nt.synth_genome(11, 80_000)
    ix = nt.Index.build([genome.tobytes()], K)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    yield genome, ix, ctx
    ctx.close()


def _substrings(rng, genome, lens):
    g = genome.tobytes()
    return [g[s:s + n] for s, n in ((int(rng.integers(0, len(g) - n + 1)), n) for n in lens)]


def _masked(reads, sub):
    return [r.translate(bytes.maketrans(NX, bytes([sub]) * len(NX))) for r in reads]


@pytest.fixture(scope="module")
def batch(env):
    """323 reads: the length classes first, then 1..300 bases; N and IUPAC runs in a fifth of
    the reads of the first 200 (so whole blocks of 64 and 65 have none); names of 0, 1, 8, 9 and
    4095 bytes, one with a NUL, one with bytes >= 0x80; one read in lower case with a U."""
    genome, _, ctx = env
    rng = np.random.default_rng(5)
    lens = LENGTHS + rng.integers(1, 301, 303).tolist()
    reads = [bytearray(r) for r in _substrings(rng, genome, lens)]
    for i in range(0, 200, 5):
        for _ in range(1 + i % 3):
            at = int(rng.integers(0, len(reads[i])))
            run = bytes([NX[int(rng.integers(0, len(NX)))]]) * int(rng.integers(1, 9))
            reads[i][at:at + len(run)] = run[:len(reads[i]) - at]
    reads = [bytes(r) for r in reads]
    lines = list(reads)
    lines[30] = reads[30].lower().replace(b"t", b"u")
    names = nl.illumina_names(rng, len(reads))
    names[0:7] = [b"", b"x", b"8 bytes!", b"nine byte", b"n" * 4095, b"nu\0l\0", b"hi\x80\xff\xfe caf\xc3\xa9"]
    names[-1] = b""
    quals = [bytes(rng.integers(33, 127, len(r), dtype=np.uint8)) for r in reads]
    text = nl.make_fastq(names, lines, quals)
    sym = [ql.normalise(l) for l in lines]
    assert sym == [r.upper() for r in reads] and any(set(r) - set(b"ACGT") for r in sym)
    return dict(text=text, n=len(reads), sym=sym, seq=_masked(sym, ctx.substitute), quals=quals, names=names)


def _dicts(metas):
    return [m.as_dict() for m in metas]


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("br", [1, 5, 64, 65, 256])
def test_encode_equals_the_restatement(env, batch, br):
    """all four components, every length class, block boundaries inside a quarter-wave group (5),
    inside a wave (65) and inside a workgroup's chunk (all of them); the last block is partial"""
    _, _, ctx = env
    b = batch
    assert b["n"] % br or br == 1  # the last block is partial
    out = ctx.encode_pack_fastq(b["text"], b["n"], block_reads=br, non_acgt="keep", qualities="keep", names="keep",
                                digests=True)
    exp = dl.metas(br, b["seq"], b["sym"], b["quals"], b["names"])
    assert _dicts(out[-1]) == exp
    assert all(m["components"] == 15 for m in exp)
    # sym differs from seq exactly in the blocks that hold a non-ACGT symbol
    for i, m in enumerate(exp):
        holds = any(set(r) - set(b"ACGT") for r in b["sym"][i * br:(i + 1) * br])
        assert (m["d_sym"] != m["d_seq"]) == holds
    if br >= 64:
        assert any(m["d_sym"] == m["d_seq"] for m in exp) and any(m["d_sym"] != m["d_seq"] for m in exp)
    assert ctx.digests == 0 and _dicts(ctx.encode_digests()) == exp  # the option was on for the call alone


def test_off_by_default_and_after_a_failure(env, batch):
    _, _, ctx = env
    b = batch
    plain = ctx.encode_pack_fastq(b["text"], b["n"], block_reads=64, non_acgt="keep")
    assert ctx.encode_digests() == []  # option off: no table
    on = ctx.encode_pack_fastq(b["text"], b["n"], block_reads=64, non_acgt="keep", digests=True)
    assert len(on[-1]) == 6 and on[1] == plain[1]  # the records do not change
    with pytest.raises(nt.NtcError):  # policy error: the N fails the call, which leaves no digests
        ctx.encode_pack_fastq(b["text"], b["n"], block_reads=64, digests=True)
    assert ctx.encode_digests() == []


# 2 ---------------------------------------------------------------------------------------------
def test_mask_has_seq_alone_and_the_same_value(env, batch):
    _, _, ctx = env
    b = batch
    keep = ctx.encode_pack_fastq(b["text"], b["n"], block_reads=64, non_acgt="keep", digests=True)[-1]
    mask = ctx.encode_pack_fastq(b["text"], b["n"], block_reads=64, non_acgt="mask", digests=True)[-1]
    assert _dicts(mask) == dl.metas(64, b["seq"])
    assert [m.components for m in mask] == [1] * 6 and [m.components for m in keep] == [3] * 6
    assert [m.d_seq for m in mask] == [m.d_seq for m in keep]


def test_bin8_and_id_digest_what_decode_prints(env, batch):
    _, _, ctx = env
    b = batch
    out = ctx.encode_pack_fastq(b["text"], b["n"], block_reads=64, non_acgt="keep", qualities="bin8", names="id",
                                digests=True)
    tab = ql.mode_table("bin8")
    binned = [tab[np.frombuffer(q, dtype=np.uint8)].tobytes() for q in b["quals"]]
    cut = [nl.name_of(b"@" + n, "id") for n in b["names"]]
    exp = dl.metas(64, b["seq"], b["sym"], binned, cut)
    assert _dicts(out[-1]) == exp
    raw = dl.metas(64, b["seq"], b["sym"], b["quals"], b["names"])
    assert all(e["d_qual"] != r["d_qual"] for e, r in zip(exp, raw))
    assert any(e["d_name"] != r["d_name"] for e, r in zip(exp, raw))


def test_pack_batch_from_an_odd_offset(env, batch):
    """ntc_encode_pack_batch (host-parsed input) has seq and sym; read_offsets[0] = 5"""
    _, _, ctx = env
    b = batch
    bases, offs = nt.pack_reads(b["sym"])
    lead = np.concatenate([np.frombuffer(b"#####", dtype=np.uint8), bases])
    for br in (5, 256):
        out = ctx.encode_pack(lead, offs + np.uint64(5), block_reads=br, non_acgt="keep", digests=True)
        assert _dicts(out[-1]) == dl.metas(br, b["seq"], b["sym"])
    out = ctx.encode_pack(lead, offs + np.uint64(5), block_reads=256, non_acgt="mask", digests=True)
    assert _dicts(out[-1]) == dl.metas(256, b["seq"])
    assert ctx.encode_pack(lead, offs + np.uint64(5), block_reads=256, non_acgt="mask")[1] == out[1]
    assert ctx.encode_digests() == []


# 3 ---------------------------------------------------------------------------------------------
def test_forced_regrow_rerun_leaves_the_same_digests(env):
    """long reads with errors need the record pool; with empty pools the call is run again"""
    genome, ix, ctx = env
    rng = np.random.default_rng(9)
    reads = []
    for r in _substrings(rng, genome, rng.integers(5_000, 20_000, 24).tolist()):
        s = bytearray(r)
        for _ in range(len(s) // 50):
            s[int(rng.integers(0, len(s)))] = b"ACGT"[int(rng.integers(0, 4))]
        reads.append(bytes(s))
    quals = [b"I" * len(r) for r in reads]
    names = nl.illumina_names(rng, len(reads))
    text = nl.make_fastq(names, reads, quals)
    exp = dl.metas(5, reads, None, quals, names)
    small = nt.GpuContext(0)
    try:
        small.set_option("pool_per_read", 0)
        small.upload(ix)
        got = small.encode_pack_fastq(text, len(reads), block_reads=5, qualities="keep", names="keep", digests=True)
        assert small.get_option("spill_reruns") > 0
    finally:
        small.close()
    # a run without one: the second call of this size on a context (its pools remember the need)
    ctx.encode_pack_fastq(text, len(reads), block_reads=5, qualities="keep", names="keep")
    before = ctx.get_option("spill_reruns")
    ref = ctx.encode_pack_fastq(text, len(reads), block_reads=5, qualities="keep", names="keep", digests=True)
    assert ctx.get_option("spill_reruns") == before
    assert _dicts(got[-1]) == _dicts(ref[-1]) == exp and got[1] == ref[1]


# 4 ---------------------------------------------------------------------------------------------
BR = 128


@pytest.fixture(scope="module")
def encoded(env, batch):
    _, _, ctx = env
    b = batch
    metas, payload, nb, runs, (qm, qp), (nm, npay), dg = ctx.encode_pack_fastq(
        b["text"], b["n"], block_reads=BR, non_acgt="keep", qualities="keep", names="keep", digests=True)
    assert len(dg) == 3
    return dict(metas=metas, payload=payload, runs=runs, q=(qm, qp), n=(nm, npay), dg=dg)


def _copy(dg):
    return [nt.DigestMeta.from_buffer_copy(ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m))) for m in dg]


def _unpack(ctx, e):
    arr = (nt.BlockMeta * len(e["metas"]))(*e["metas"])
    assert ctx.unpack(arr, e["payload"], len(e["metas"]))[0] == len(e["metas"])


def _decode(ctx, e, dg, side=("x", "q", "n")):
    _unpack(ctx, e)
    if "x" in side:
        ctx.set_exceptions(e["runs"], ctx.substitute)
    if "q" in side:
        ctx.set_qualities(*e["q"])
    if "n" in side:
        ctx.set_names(*e["n"])
    ctx.decode_set_digests(dg)
    return ctx.decode_fasta_unpacked(first_id=1)


def test_decode_verifies(env, batch, encoded):
    _, _, ctx = env
    b, e = batch, encoded
    text = _decode(ctx, e, e["dg"])
    assert text == nl.named_text(b["names"], b["sym"], b["quals"])
    assert _dicts(ctx.decode_digests()) == _dicts(e["dg"])  # all four components checked
    # the expected digests were used: the next call checks nothing and prints as ever
    _unpack(ctx, e)
    assert ctx.decode_fasta_unpacked(first_id=1).startswith(b">seq.1\n")
    # sections that do not cover exactly the reads
    for dg in (e["dg"][:2], e["dg"] + e["dg"][:1]):
        with pytest.raises(nt.NtcError) as err:
            _decode(ctx, e, dg)
        assert err.value.code == FORMAT


def test_not_checkable_components_pass(env, batch, encoded):
    """qual and name bits, decoded without those side files (and sym without the exceptions)"""
    _, _, ctx = env
    b, e = batch, encoded
    text = _decode(ctx, e, e["dg"], side=())
    assert text == b"".join(b">seq.%d\n%s\n" % (i + 1, r) for i, r in enumerate(b["seq"]))
    got = ctx.decode_digests()
    assert [m.components for m in got] == [1, 1, 1]
    assert [(m.d_seq, m.d_sym, m.d_qual, m.d_name) for m in got] == [(m.d_seq, 0, 0, 0) for m in e["dg"]]
    _decode(ctx, e, e["dg"], side=("x", "q"))
    assert [m.components for m in ctx.decode_digests()] == [7, 7, 7]


@pytest.mark.parametrize("block,field", [(1, "d_qual"), (2, "d_name"), (0, "d_seq"), (1, "d_sym"), (2, "n_bases")])
def test_damaged_digests_name_block_and_component(env, encoded, block, field):
    _, _, ctx = env
    e = encoded
    dg = _copy(e["dg"])
    setattr(dg[block], field, getattr(dg[block], field) ^ (1 << 17))
    with pytest.raises(nt.NtcError) as err:
        _decode(ctx, e, dg)
    comp = "seq" if field == "n_bases" else field[2:]
    assert err.value.code == DIGEST and f"block {block}," in str(err.value) and f"component {comp}" in str(err.value)
    assert _dicts(ctx.decode_digests()) == _dicts(e["dg"])  # what was computed is still the truth
    assert _decode(ctx, e, e["dg"]).startswith(b"@")  # and the next call is clean


def test_mismatch_in_two_blocks_reports_the_lower(env, encoded):
    _, _, ctx = env
    e = encoded
    dg = _copy(e["dg"])
    dg[2].d_seq ^= 1
    dg[1].d_name ^= 1
    with pytest.raises(nt.NtcError) as err:
        _decode(ctx, e, dg)
    assert err.value.code == DIGEST and "block 1," in str(err.value) and "component name" in str(err.value)


def test_set_digests_refuses(env, encoded):
    _, _, ctx = env
    for change in ({"components": 2}, {"components": 31}, {"reserved": 1}, {"n_reads": 0}):
        dg = _copy(encoded["dg"])
        for k, v in change.items():
            setattr(dg[1], k, v)
        with pytest.raises(nt.NtcError) as err:
            ctx.decode_set_digests(dg)
        assert err.value.code == 1
    dg = _copy(encoded["dg"])
    dg[0].components, dg[0].d_name = 7, dg[0].d_name | 1
    with pytest.raises(nt.NtcError):
        ctx.decode_set_digests(dg)


# 5 ---------------------------------------------------------------------------------------------
def test_damaged_record_is_a_seq_mismatch(env):
    """one long record's colex id moved to a neighbouring node, chosen with the CPU oracle so that
    the record still decodes to as many bases, but to other bases"""
    genome, ix, ctx = env
    rng = np.random.default_rng(21)
    n, L, br = 96, 150, 32
    reads = _substrings(rng, genome, [L] * n)
    bases, offs = nt.pack_reads(reads)
    dg = ctx.encode_pack(bases, offs, block_reads=br, digests=True)[-1]
    assert _dicts(dg) == dl.metas(br, reads)
    recs, roff = ctx.encode(bases, offs)
    orc = OracleIndex(ix.n, K, ix.rows, ix.C, ix.lcs)
    flags = recs >> np.uint64(56)
    victim = 40  # a read of block 1
    at = next(int(i) for i in range(int(roff[victim]), int(roff[victim + 1])) if not int(flags[i]) & 2)
    bad = None
    for step in (1, -1, 2, -2, 3, -3, 5, -5, 8, -8):
        node = int(recs[at] & np.uint64(0xFFFFFFFF)) + step
        if not 0 < node < ix.n:
            continue
        trial = recs.copy()
        trial[at] = (recs[at] & ~np.uint64(0xFFFFFFFF)) | np.uint64(node)
        try:
            out, o2 = orc.decode(trial)
        except RuntimeError:
            continue
        if np.array_equal(o2, offs) and not np.array_equal(out, bases) and set(out.tolist()) <= set(b"ACGT"):
            bad = trial
            break
    assert bad is not None
    L_ = ctx.L
    out = np.zeros(n * (L + 16), dtype=np.uint8)
    need = ctypes.c_uint64()

    def run(r):
        ctx.decode_set_digests(dg)
        return L_.ntc_decode_fasta(ctx.h, r.ctypes.data_as(ctypes.c_void_p), len(r), n, n * L, 1,
                                   out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(need))

    assert run(recs) == 0
    assert out[:need.value].tobytes() == b"".join(b">seq.%d\n%s\n" % (i + 1, r) for i, r in enumerate(reads))
    assert run(bad) == DIGEST
    msg = L_.ntc_last_error(ctx.h).decode()
    assert "block 1," in msg and "component seq" in msg
    got = ctx.decode_digests()
    assert (got[0].d_seq, got[2].d_seq) == (dg[0].d_seq, dg[2].d_seq) and got[1].d_seq != dg[1].d_seq
    assert run(recs) == 0  # and without digests the damaged records decode quietly, as ever
    assert L_.ntc_decode_fasta(ctx.h, bad.ctypes.data_as(ctypes.c_void_p), len(bad), n, n * L, 1,
                               out.ctypes.data_as(ctypes.c_void_p), len(out), ctypes.byref(need)) == 0


# 6 ---------------------------------------------------------------------------------------------
# The file pipelines and both command lines.  A block has 65,536 reads there: three blocks of
# 60-base reads, the middle one of exact genome substrings (no short record: the pipeline drops
# it, as the reference does), the last one partial.
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
PBR = 65536


@pytest.fixture(scope="module")
def files(env, tmp_path_factory):
    genome, ix, ctx = env
    d = tmp_path_factory.mktemp("digest_files")
    ix.save(str(d / "idx"))
    other = nt.Index.build([nt.synth_genome(12, 80_000).tobytes()], K)
    other.save(str(d / "other"))
    L, n_last = 60, 1000
    g = genome.tobytes()
    rng = np.random.default_rng(31)
    noisy = nt.synth_reads(genome, 7, 0, PBR + n_last, L, 30_000).reshape(-1, L)
    exact = np.stack([np.frombuffer(g[s:s + L], dtype=np.uint8) for s in rng.integers(0, len(g) - L, PBR).tolist()])
    reads = np.concatenate([noisy[:PBR], exact, noisy[PBR:]])
    n = len(reads)
    lines = []
    for i in range(n):
        lines += [b"@r%d x" % i, reads[i].tobytes(), b"+", b"I" * (L - 1) + b"5"]
    text = b"\n".join(lines) + b"\n"
    (d / "r.fq").write_bytes(text)
    with gzip.open(d / "r.fq.gz", "wb", compresslevel=1) as f:
        f.write(text)
    # the digests of the blocks the pipeline writes (0 and 2), from the call test 1 pinned
    dg = ctx.encode_pack_fastq(text, n, block_reads=PBR, qualities="keep", names="keep", digests=True)[-1]
    paths = dict(e=d / "e.dat", q=d / "e.ntcq", n=d / "e.ntcn", d=d / "e.ntcd")
    with open(paths["e"], "wb") as fe, open(paths["q"], "wb") as fq, open(paths["n"], "wb") as fn, \
            open(paths["d"], "wb") as fd:
        st = nt.encode_file([ctx], str(d / "r.fq"), fe.fileno(), threads=4, deflate="zlib", qualities="keep",
                            q_fd=fq.fileno(), names="keep", n_fd=fn.fileno(), d_fd=fd.fileno())
    kept = [i for i in range(n) if not PBR <= i < 2 * PBR]
    out_text = b"".join(b"@r%d x\n%s\n+\n%s\n" % (i, reads[i].tobytes(), b"I" * (L - 1) + b"5") for i in kept)
    return dict(dir=d, n=n, L=L, dg=dg, st=st, paths=paths, out_text=out_text, n_kept=len(kept))


def _side(f):
    return dict(q_path=str(f["paths"]["q"]), n_path=str(f["paths"]["n"]))


def test_pipeline_writes_the_sections_of_the_blocks_written(env, files):
    _, ix, ctx = env
    f = files
    assert f["st"]["blocks"] == 2 and f["st"]["dropped_blocks"] == 1
    assert f["st"]["d"] == dict(sections=2, blocks_seq=2, blocks_sym=0, blocks_qual=2, blocks_name=2, not_checkable=0)
    comp, k, n_nodes, metas = nt.read_digests(str(f["paths"]["d"]))
    assert (comp, k, n_nodes) == (13, K, ix.n) and ctx.get_option("digests") == 0
    assert _dicts(metas) == [_dicts(f["dg"])[0], _dicts(f["dg"])[2]]  # the dropped block took its section
    assert f["paths"]["d"].read_bytes() == dl.file_bytes(13, K, ix.n, _dicts(metas))
    # without the digest file the other three files are byte for byte the same
    d = f["dir"]
    with open(d / "p.dat", "wb") as fe, open(d / "p.ntcq", "wb") as fq, open(d / "p.ntcn", "wb") as fn:
        nt.encode_file([ctx], str(d / "r.fq"), fe.fileno(), threads=4, deflate="zlib", qualities="keep", q_fd=fq.fileno(),
                       names="keep", n_fd=fn.fileno())
    for a, b in (("p.dat", "e"), ("p.ntcq", "q"), ("p.ntcn", "n")):
        assert (d / a).read_bytes() == f["paths"][b].read_bytes(), a


def test_digest_file_does_not_depend_on_contexts_or_compression(env, files):
    _, ix, ctx = env
    f, d = files, files["dir"]
    second = nt.GpuContext(0)
    try:
        second.share_index(ctx)
        for name, ctxs, src in (("two", [ctx, second], "r.fq"), ("gz", [ctx], "r.fq.gz")):
            with open(d / (name + ".dat"), "wb") as fe, open(d / (name + ".q"), "wb") as fq, \
                    open(d / (name + ".n"), "wb") as fn, open(d / (name + ".d"), "wb") as fd:
                nt.encode_file(ctxs, str(d / src), fe.fileno(), threads=4, blocks_per_batch=1, deflate="zlib",
                               qualities="keep", q_fd=fq.fileno(), names="keep", n_fd=fn.fileno(), d_fd=fd.fileno())
            assert (d / (name + ".d")).read_bytes() == f["paths"]["d"].read_bytes(), name
            assert (d / (name + ".dat")).read_bytes() == f["paths"]["e"].read_bytes(), name
        # a host-parsed input has seq alone
        with open(d / "hp.dat", "wb") as fe, open(d / "hp.d", "wb") as fd:
            st = nt.encode_file([ctx], str(d / "r.fq"), fe.fileno(), threads=4, host_parse=True, d_fd=fd.fileno())
        comp, _, _, metas = nt.read_digests(str(d / "hp.d"))
        assert comp == 1 and st["d"]["sections"] == 2
        assert [(m.d_seq, m.components) for m in metas] == [(f["dg"][0].d_seq, 1), (f["dg"][2].d_seq, 1)]
    finally:
        second.close()


def test_decode_file_verifies_and_names_what_differs(env, files):
    _, ix, ctx = env
    f, d = files, files["dir"]
    out = d / "o.fq"
    with open(out, "wb") as fo:
        st = nt.decode_file([ctx], str(f["paths"]["e"]), fo.fileno(), threads=4, blocks_per_batch=1,
                            d_path=str(f["paths"]["d"]), **_side(f))
    assert out.read_bytes() == f["out_text"] and st["reads"] == f["n_kept"]
    assert st["d"] == dict(sections=2, blocks_seq=2, blocks_sym=0, blocks_qual=2, blocks_name=2, not_checkable=0)
    # without the side files: the text is FASTA, qual and name cannot be checked
    with open(out, "wb") as fo:
        st = nt.decode_file([ctx], str(f["paths"]["e"]), fo.fileno(), threads=4, d_path=str(f["paths"]["d"]))
    assert st["d"] == dict(sections=2, blocks_seq=2, blocks_sym=0, blocks_qual=0, blocks_name=0, not_checkable=12)
    # out_fd -1: the same verdict, nothing written
    st = nt.decode_file([ctx], str(f["paths"]["e"]), -1, threads=4, d_path=str(f["paths"]["d"]), **_side(f))
    assert st["d"]["sections"] == 2 and st["reads"] == f["n_kept"] and st["bytes_out"] == len(f["out_text"])
    # a flipped digest in the second block written: the first block's text is still written
    data = bytearray(f["paths"]["d"].read_bytes())
    data[32 + 56 + 32 + 3] ^= 0x10  # d_qual of section 1
    (d / "flip.ntcd").write_bytes(bytes(data))
    with open(out, "wb") as fo, pytest.raises(nt.NtcError) as err:
        nt.decode_file([ctx], str(f["paths"]["e"]), fo.fileno(), threads=4, blocks_per_batch=1,
                       d_path=str(d / "flip.ntcd"), **_side(f))
    assert err.value.code == DIGEST and err.value.bad_read == PBR
    assert "block 1 " in str(err.value) and "component qual" in str(err.value)
    got = out.read_bytes()
    assert f["out_text"].startswith(got) and len(got) < len(f["out_text"])  # a prefix of the true text
    # a side file of another run whose block sizes match: the names of block 0 given for block 1
    comp, k, n_nodes, metas = nt.read_digests(str(f["paths"]["d"]))
    swapped = _copy(metas)
    swapped[1].d_name = metas[0].d_name
    with open(d / "swap.ntcd", "wb") as fs:
        nt.write_digests(fs.fileno(), comp, k, n_nodes, swapped)
    with pytest.raises(nt.NtcError) as err:
        nt.decode_file([ctx], str(f["paths"]["e"]), -1, threads=4, d_path=str(d / "swap.ntcd"), **_side(f))
    assert err.value.code == DIGEST and "block 1 " in str(err.value) and "component name" in str(err.value)


def test_truncated_input_and_leftover_sections(env, files):
    _, ix, ctx = env
    f, d = files, files["dir"]
    data = f["paths"]["e"].read_bytes()
    (d / "trunc.dat").write_bytes(data[:-7])
    with open(d / "o.fa", "wb") as fo:  # without the digest file: ends quietly, as ever
        st = nt.decode_file([ctx], str(d / "trunc.dat"), fo.fileno(), threads=4)
    assert st["blocks"] == 1 and st["reads"] == PBR
    with open(d / "o.fa", "wb") as fo, pytest.raises(nt.NtcError) as err:
        nt.decode_file([ctx], str(d / "trunc.dat"), fo.fileno(), threads=4, d_path=str(f["paths"]["d"]))
    assert err.value.code == FORMAT and "truncated" in str(err.value)
    # one section too few
    (d / "short.ntcd").write_bytes(f["paths"]["d"].read_bytes()[:-56])
    with pytest.raises(nt.NtcError) as err:
        nt.decode_file([ctx], str(f["paths"]["e"]), -1, threads=4, d_path=str(d / "short.ntcd"))
    assert err.value.code == FORMAT and "fewer sections" in str(err.value)
    # one too many
    (d / "long.ntcd").write_bytes(f["paths"]["d"].read_bytes() + f["paths"]["d"].read_bytes()[-56:])
    with pytest.raises(nt.NtcError) as err:
        nt.decode_file([ctx], str(f["paths"]["e"]), -1, threads=4, d_path=str(d / "long.ntcd"))
    assert err.value.code == FORMAT and "more sections" in str(err.value)


def _cli(which, *args, stdout=subprocess.PIPE):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    envv = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), stdout=stdout, stderr=subprocess.PIPE, env=envv, timeout=300)


@pytest.mark.parametrize("which", ["native", "python"])
def test_command_lines_fail_loudly(env, files, which):
    """encode --digest-file writes the pipeline's file; decode and verify pass on the intact set and
    name block and component for a wrong index, a flipped record and a flipped digest"""
    f, d = files, files["dir"]
    side = ["--quality-file", str(f["paths"]["q"]), "--name-file", str(f["paths"]["n"])]
    with open(d / "cli.dat", "wb") as fo:
        r = _cli(which, "encode", "-i", str(d / "idx"), "--devices", "0,0", "--deflate", "zlib", "--qualities", "keep",
                 "--quality-file", str(d / "cli.q"), "--names", "keep", "--name-file", str(d / "cli.n"), "--digest-file",
                 str(d / "cli.d"), str(d / "r.fq.gz"), stdout=fo)
    assert r.returncode == 0, r.stderr
    assert (d / "cli.d").read_bytes() == f["paths"]["d"].read_bytes()
    assert (d / "cli.dat").read_bytes() == f["paths"]["e"].read_bytes()
    good = ["-i", str(d / "idx"), "--digest-file", str(f["paths"]["d"]), *side, str(f["paths"]["e"])]
    r = _cli(which, "decode", *good)
    assert r.returncode == 0 and r.stdout == f["out_text"], r.stderr
    r = _cli(which, "verify", *good)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"verify: OK: 2 blocks, %d reads, checked seq,qual,name, not checkable -\n" % f["n_kept"]
    r = _cli(which, "verify", "-i", str(d / "idx"), "--digest-file", str(f["paths"]["d"]), str(f["paths"]["e"]))
    assert r.returncode == 0 and r.stdout.endswith(b"checked seq, not checkable qual,name\n"), r.stderr
    # another genome's index with the same k: before any output
    for command in ("decode", "verify"):
        r = _cli(which, command, "-i", str(d / "other"), "--digest-file", str(f["paths"]["d"]), *side, str(f["paths"]["e"]))
        assert r.returncode != 0 and r.stdout == b"" and b"written against another index" in r.stderr, r.stderr
    # bases that differ from the digested ones (what a flipped record gives: the records' own
    # damage is test_damaged_record_is_a_seq_mismatch's), and a flipped digest
    flip = bytearray(f["paths"]["d"].read_bytes())
    flip[32 + 16] ^= 1  # d_seq of section 0
    (d / "seq.ntcd").write_bytes(bytes(flip))
    flip = bytearray(f["paths"]["d"].read_bytes())
    flip[32 + 56 + 40] ^= 1  # d_name of section 1
    (d / "name.ntcd").write_bytes(bytes(flip))
    for path, block, comp in ((d / "seq.ntcd", 0, b"seq"), (d / "name.ntcd", 1, b"name")):
        for command in ("decode", "verify"):
            r = _cli(which, command, "-i", str(d / "idx"), "--digest-file", str(path), *side, str(f["paths"]["e"]))
            assert r.returncode != 0, (command, path)
            assert b"block %d " % block in r.stderr and b"component " + comp in r.stderr, r.stderr
            assert f["out_text"].startswith(r.stdout) and len(r.stdout) < len(f["out_text"])
            if command == "verify":
                assert r.stdout == b""
    # a truncated encoded.dat: an error under --digest-file, quiet without it
    (d / "t.dat").write_bytes(f["paths"]["e"].read_bytes()[:-9])
    r = _cli(which, "decode", "-i", str(d / "idx"), str(d / "t.dat"))
    assert r.returncode == 0 and r.stdout.count(b"\n") == 2 * PBR
    for command in ("decode", "verify"):
        r = _cli(which, command, "-i", str(d / "idx"), "--digest-file", str(f["paths"]["d"]), str(d / "t.dat"))
        assert r.returncode != 0 and b"truncated" in r.stderr, r.stderr
