"""Reads with N and IUPAC symbols on the GPU (nonacgt.hip): policy mask / keep on every
host-buffer encode entry point, the exception runs, their way back on decode, and the
file-to-file pipelines with the "NTCX" side file.

The checker is independent of the code under test: nx_lib.py (numpy) masks with the
substitute base and lists the canonical runs, and the C oracle (oracle_lib) encodes the
masked reads."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import ntcomp_amd as nt
from nx_lib import SYMS, hand_batch, mask, nonacgt, ragged_batch, runs_of
from oracle_lib import OracleIndex

pytestmark = pytest.mark.gpu
INVALID_BASE, FORMAT, UNSUPPORTED = 2, 8, 10


@pytest.fixture(scope="module")
def env():
    genome = nt.synth_genome(7, 20_000)
    ix = nt.Index.build([genome.tobytes()], 31)
    ctx = nt.GpuContext(0)
    ctx.upload(ix)
    orc = OracleIndex(ix.n, ix.k, ix.rows, ix.C, ix.lcs)
    yield genome, ix, ctx, orc
    ctx.close()


def _blob(metas):
    return b"".join(ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m)) for m in metas)


def _round_trip(ctx, recs, runs, sub):
    ctx.set_exceptions(runs, sub)
    return ctx.decode(recs)


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead,shift,tail", [(5, 0, 1), (0, 1, 0), (16, 2, 16)])
def test_canonical_runs_on_the_hand_built_batch(env, lead, shift, tail):
    """nx_lib.hand_batch: runs starting and ending at batch positions 15, 16, 17, 63, 64, 65
    (over the three shifts), totals that are and are not multiples of 16 and 64, a read of
    one N, all-N reads of 1, 150 and 5000, NN | NN across a read boundary, NNRRN, all twelve
    symbols, read_offsets[0] = 5 (not 0, no multiple of 16)."""
    _, _, ctx, orc = env
    bases, offs = hand_batch(lead=lead, tail=tail, shift=shift)
    assert int(offs[0]) == lead and int(offs[-1] - offs[0]) % 64 == tail
    sub = ctx.substitute
    assert sub == ord("A")
    recs, roff, runs = ctx.encode(bases, offs, non_acgt="keep")
    exp = runs_of(bases, offs)
    assert set(exp["sym"].tolist()) == set(SYMS) and 5000 in exp["len"].tolist()
    assert np.array_equal(runs, exp)
    assert ctx.get_option("nx_runs") == len(exp) and ctx.get_option("nx_bases") == int(exp["len"].sum())
    B, rel = bases[int(offs[0]):int(offs[-1])], offs - offs[0]
    erecs, eroff = orc.encode(mask(B, sub), rel)
    assert np.array_equal(roff, eroff) and np.array_equal(recs, erecs)
    out, o2 = _round_trip(ctx, recs, runs, sub)
    assert np.array_equal(o2, rel) and np.array_equal(out, B)
    assert ctx.get_option("non_acgt") == 0  # the policy held for that call only


# 2 ---------------------------------------------------------------------------------------------
def test_scan_across_workgroups_ragged(env):
    _, _, ctx, _ = env
    bases, offs = ragged_batch(np.random.default_rng(23), 20_000)
    recs, roff, runs = ctx.encode(bases, offs, non_acgt="keep")
    exp = runs_of(bases, offs)
    assert len(exp) > 5000 and np.array_equal(runs, exp)
    out, o2 = _round_trip(ctx, recs, runs, ctx.substitute)
    assert np.array_equal(o2, offs) and np.array_equal(out, bases)


def test_scan_across_workgroups_dense(env):
    """NANANA... over 100,000 bases in reads of 150: 50,000 runs, more than the run list's
    first guess holds, so the batch is staged and run a second time."""
    _, _, ctx, _ = env
    bases = np.frombuffer(b"NA" * 50_000, dtype=np.uint8)
    offs = np.append(np.arange(0, 100_000, 150), 100_000).astype(np.uint64)
    recs, roff, runs = ctx.encode(bases, offs, non_acgt="keep")
    assert len(runs) == 50_000 and np.array_equal(runs, runs_of(bases, offs))
    out, o2 = _round_trip(ctx, recs, runs, ctx.substitute)
    assert np.array_equal(o2, offs) and np.array_equal(out, bases)
    metas, payload, runs2 = ctx.encode_pack(bases, offs, non_acgt="keep")
    assert np.array_equal(runs2, runs)


# 3 ---------------------------------------------------------------------------------------------
def test_clean_batch_is_untouched(env):
    genome, _, ctx, _ = env
    n, L = 3000, 150
    reads = nt.synth_reads(genome, 5, 0, n, L, 10_000)
    offs = np.arange(0, n * L + 1, L, dtype=np.uint64)
    m0, p0 = ctx.encode_pack(reads, offs, block_reads=1024)
    m1, p1, runs = ctx.encode_pack(reads, offs, block_reads=1024, non_acgt="keep")
    assert len(runs) == 0 and ctx.get_option("nx_runs") == 0 and ctx.get_option("nx_bases") == 0
    assert _blob(m1) == _blob(m0) and p1 == p0
    r0, o0 = ctx.encode(reads, offs)
    r1, o1, runs = ctx.encode(reads, offs, non_acgt="keep")
    assert len(runs) == 0 and np.array_equal(r0, r1) and np.array_equal(o0, o1)


# 4 ---------------------------------------------------------------------------------------------
def test_default_policy_is_unchanged(env):
    genome, _, ctx, _ = env
    n, L = 200, 100
    reads = nt.synth_reads(genome, 6, 0, n, L, 0).copy()
    offs = np.arange(0, n * L + 1, L, dtype=np.uint64)
    reads[77 * L + 3] = ord("N")
    assert ctx.get_option("non_acgt") == 0
    for call in (ctx.encode, ctx.encode_pack, lambda b, o: ctx.encode(b, o, non_acgt="error")):
        with pytest.raises(nt.NtcError) as e:
            call(reads, offs)
        assert e.value.code == INVALID_BASE and e.value.bad_read == 77
    assert len(ctx.exceptions()) == 0


def test_device_entry_points_refuse_or_ignore(env):
    _, _, ctx, _ = env
    ctx.set_option("non_acgt", 1)
    try:
        rc = ctx.L.ntc_encode_batch_device(ctx.h, None, None, 0, 0, None, 0, ctypes.c_void_p(8))
        assert rc == UNSUPPORTED
    finally:
        ctx.set_option("non_acgt", 0)


# 5 ---------------------------------------------------------------------------------------------
def test_mask_is_lossy_and_lists_nothing(env):
    _, _, ctx, orc = env
    bases, offs = ragged_batch(np.random.default_rng(31), 2000)
    recs, roff, runs = ctx.encode(bases, offs, non_acgt="mask")
    assert len(runs) == 0 and len(ctx.exceptions()) == 0
    exp = runs_of(bases, offs)
    assert ctx.get_option("nx_runs") == len(exp) > 0 and ctx.get_option("nx_bases") == int(nonacgt(bases).sum())
    erecs, eroff = orc.encode(mask(bases, ctx.substitute), offs)
    assert np.array_equal(roff, eroff) and np.array_equal(recs, erecs)
    out, _ = ctx.decode(recs)
    assert np.array_equal(out, mask(bases, ctx.substitute))


# 6 ---------------------------------------------------------------------------------------------
def test_substitute_is_the_lowest_base_of_the_index():
    rng = np.random.default_rng(41)
    cg = np.frombuffer(b"CG", dtype=np.uint8)[rng.integers(0, 2, 2000)]
    ix = nt.Index.build([cg.tobytes()], 11)
    ctx = nt.GpuContext(0)
    try:
        ctx.upload(ix)
        assert ctx.substitute == ord("C")
        reads = [bytearray(cg[a:a + 60].tobytes()) for a in range(0, 1800, 60)]
        reads[3][10:14] = b"NNNN"
        reads[4][0:1] = b"R"
        reads[29][59:60] = b"N"
        bases, offs = nt.pack_reads([bytes(r) for r in reads])
        recs, roff, runs = ctx.encode(bases, offs, non_acgt="keep")
        assert np.array_equal(runs, runs_of(bases, offs)) and len(runs) == 3
        orc = OracleIndex(ix.n, ix.k, ix.rows, ix.C, ix.lcs)
        erecs, eroff = orc.encode(mask(bases, "C"), offs)
        assert np.array_equal(roff, eroff) and np.array_equal(recs, erecs)
        out, o2 = _round_trip(ctx, recs, runs, "C")
        assert np.array_equal(out, bases) and np.array_equal(o2, offs)
        reads[7][5:6] = b"A"  # a base the index does not contain: an error under every policy
        bases, offs = nt.pack_reads([bytes(r) for r in reads])
        for policy in ("keep", "mask", "error"):
            with pytest.raises(nt.NtcError) as e:
                ctx.encode(bases, offs, non_acgt=policy)
            assert e.value.code == INVALID_BASE and e.value.bad_read == (3 if policy == "error" else 7)
    finally:
        ctx.close()


# 7 ---------------------------------------------------------------------------------------------
def test_passes_hand_each_pass_its_own_runs(env):
    _, _, ctx, _ = env
    bases, offs = ragged_batch(np.random.default_rng(53), 400, frac=0.6)
    one = ctx.encode(bases, offs, non_acgt="keep")
    ctx.set_option("max_pass_bases", 4096)
    try:
        assert int(offs[-1]) > 8 * 4096
        many = ctx.encode(bases, offs, non_acgt="keep")
        for a, b in zip(one, many):
            assert np.array_equal(a, b)
        assert np.array_equal(many[2], runs_of(bases, offs))
        out, o2 = _round_trip(ctx, many[0], many[2], ctx.substitute)
        assert np.array_equal(out, bases) and np.array_equal(o2, offs)
    finally:
        ctx.set_option("max_pass_bases", 1 << 30)


# 8 ---------------------------------------------------------------------------------------------
def test_fastq_on_the_gpu_equals_the_host_parser(env, tmp_path):
    """The iupac_and_junk shape of test_gpu_fastq.py, regenerated."""
    _, _, ctx, _ = env
    rng = np.random.default_rng(17)
    alphabet = np.frombuffer(b"ACGTNacgtnRYSWKMBDHVrYswkmbdhvuU.~-xX*0", np.uint8)
    text = []
    for i in range(2000):
        seq = bytes(rng.choice(alphabet, int(rng.integers(20, 301))))
        text.append(b"@read_%d some description\n" % i + seq + b"\n+\n" + b"F" * len(seq) + b"\n")
    text = b"".join(text)
    (tmp_path / "x.fq").write_bytes(text)
    rd = nt.FastxReader(str(tmp_path / "x.fq"))
    bases, offs = rd.batch(1 << 20)
    rd.close()
    assert len(offs) - 1 == 2000
    m0, p0, r0 = ctx.encode_pack(bases, offs, block_reads=512, non_acgt="keep")
    m1, p1, nb, r1 = ctx.encode_pack_fastq(text, 2000, block_reads=512, non_acgt="keep")
    assert nb == len(bases) and np.array_equal(r0, runs_of(bases, offs)) and len(r0) > 10_000
    assert np.array_equal(r1, r0) and _blob(m1) == _blob(m0) and p1 == p0


# 9 ---------------------------------------------------------------------------------------------
BAD_RUNS = {
    "read past the reads": ([(2, 0, 1, "N")], None),
    "pos + len past the read": ([(1, 3, 2, "N")], None),
    "wrong sub": (None, "G"),
    "over a base that is not the substitute": ([(0, 1, 1, "N")], None),
    "sym A": ([(0, 4, 2, "A")], None),
}


@pytest.mark.parametrize("what", sorted(BAD_RUNS))
def test_decode_validates_every_run(env, what):
    _, _, ctx, _ = env
    bases, offs = nt.pack_reads([b"ACGTNNACGT", b"NACG"])
    recs, _, runs = ctx.encode(bases, offs, non_acgt="keep")
    assert len(runs) == 2
    rows, sub = BAD_RUNS[what]
    bad = runs if rows is None else np.array([(r, p, n, ord(s), 0) for r, p, n, s in rows], dtype=nt.NX_RUN)
    ctx.set_exceptions(bad, sub or "A")
    with pytest.raises(nt.NtcError) as e:
        ctx.decode(recs)
    assert e.value.code == FORMAT
    out, o2 = ctx.decode(recs)  # the runs are gone: a clean call gives the masked reads
    assert bytes(out) == b"ACGTAAACGTAACG" and np.array_equal(o2, offs)
    out, _ = _round_trip(ctx, recs, runs, "A")
    assert np.array_equal(out, bases)


# 10 --------------------------------------------------------------------------------------------
def _fastq(reads, L):
    n = len(reads) // L
    nl = np.full((n, 1), 10, np.uint8)
    rec = np.concatenate([np.frombuffer(b"@r\n", np.uint8)[None, :].repeat(n, 0), reads.reshape(n, L), nl,
                          np.frombuffer(b"+\n", np.uint8)[None, :].repeat(n, 0), np.full((n, L), ord("I"), np.uint8), nl],
                         axis=1)
    return rec.tobytes()


def _with_runs(reads, L, rng, frac):
    reads = reads.copy().reshape(-1, L)
    for r in np.flatnonzero(rng.random(len(reads)) < frac):
        p = int(rng.integers(0, L))
        reads[r, p:p + int(rng.integers(1, 9))] = SYMS[int(rng.integers(0, 12))]
    return reads.reshape(-1)


def _fasta(reads, L):
    return b"".join(b">seq.%d\n%s\n" % (i + 1, bytes(r)) for i, r in enumerate(reads.reshape(-1, L)))


def _encode_file(ctxs, path, tmp_path, tag, **kw):
    with open(tmp_path / (tag + ".dat"), "wb") as f, open(tmp_path / (tag + ".ntcx"), "wb") as x:
        st = nt.encode_file(ctxs, str(path), f.fileno(), threads=4, blocks_per_batch=1, deflate="zlib",
                            non_acgt="keep", nx_fd=x.fileno(), **kw)
    return st, (tmp_path / (tag + ".ntcx")).read_bytes()


def _decode_file(ctxs, tmp_path, tag, nx=True):
    with open(tmp_path / (tag + ".fa"), "wb") as f:
        st = nt.decode_file(ctxs, str(tmp_path / (tag + ".dat")), f.fileno(), threads=4, blocks_per_batch=1,
                            nx_path=str(tmp_path / (tag + ".ntcx")) if nx else None)
    return st, (tmp_path / (tag + ".fa")).read_bytes()


def test_files_keep_and_restore(env, tmp_path):
    genome, _, ctx, _ = env
    ctx2 = nt.GpuContext(0)
    ctx2.share_index(ctx)
    try:
        n, L = 140_000, 40
        rng = np.random.default_rng(61)
        reads = _with_runs(nt.synth_reads(genome, 9, 0, n, L, 10_000), L, rng, 0.2)
        offs = np.arange(0, n * L + 1, L, dtype=np.uint64)
        exp = runs_of(reads, offs)
        (tmp_path / "r.fq").write_bytes(_fastq(reads, L))
        with gzip.open(tmp_path / "r.fq.gz", "wb", compresslevel=1) as f:
            f.write(_fastq(reads, L))
        side = {}
        # plain FASTQ parsed on the GPU; the same file gzip'd, parsed by the host pool; two contexts
        for tag, path, ctxs in (("plain", "r.fq", [ctx]), ("gz", "r.fq.gz", [ctx]), ("two", "r.fq", [ctx, ctx2])):
            st, side[tag] = _encode_file(ctxs, tmp_path / path, tmp_path, tag, host_parse=tag == "gz")
            assert st["reads"] == n and st["dropped_blocks"] == 0 and st["blocks"] == 3
            assert (st["gpu_parsed"] > 0) == (tag != "gz")
            assert st["nx"] == {"runs": len(exp), "bases": int(nonacgt(reads).sum()),
                                "reads": len(np.unique(exp["read"])), "runs_in_dropped_blocks": 0}
            runs, sub = nt.read_exceptions(tmp_path / (tag + ".ntcx"))
            assert sub == ord("A") and np.array_equal(runs, exp)
            std, text = _decode_file(ctxs, tmp_path, tag)
            assert std["reads"] == n and text == _fasta(reads, L)
        assert side["plain"] == side["gz"] == side["two"]
        # without the side file: the masked reads, from our decoder as from any other
        _, text = _decode_file([ctx], tmp_path, "plain", nx=False)
        assert text == _fasta(mask(reads, "A"), L)
        # the old entry point keeps today's behaviour
        with open(tmp_path / "old.dat", "wb") as f, pytest.raises(nt.NtcError) as e:
            nt.encode_file([ctx], str(tmp_path / "r.fq"), f.fileno(), threads=4, blocks_per_batch=1)
        assert e.value.code == INVALID_BASE and e.value.bad_read == int(exp["read"][0])
        # a side file that belongs to another encoding is refused
        other = exp.copy()
        other["pos"][0], other["len"][0] = L - 2, 8  # past the read's end
        with open(tmp_path / "plain.ntcx", "wb") as x:
            nt.write_exceptions(x.fileno(), other[:1], "A")
        with open(tmp_path / "bad.fa", "wb") as f, pytest.raises(nt.NtcError) as e:
            nt.decode_file([ctx], str(tmp_path / "plain.dat"), f.fileno(), threads=4, blocks_per_batch=1,
                           nx_path=str(tmp_path / "plain.ntcx"))
        assert e.value.code == FORMAT
        assert ctx.get_option("non_acgt") == 0 and ctx2.get_option("non_acgt") == 0
    finally:
        ctx2.close()


def test_files_renumber_past_a_dropped_block(env, tmp_path):
    """A leading block of 65,536 reads of 8 bases has no long record and is dropped (SURVEY
    App. B.3): its runs are not written, and every later read's number moves down by 65,536,
    exactly as decode numbers its seq.N lines."""
    genome, _, ctx, _ = env
    rng = np.random.default_rng(67)
    n0, L0, n, L = 65_536, 8, 140_000, 40
    head = _with_runs(nt.synth_reads(genome, 10, 0, n0, L0, 0), L0, rng, 0.1)
    reads = _with_runs(nt.synth_reads(genome, 9, 0, n, L, 10_000), L, rng, 0.2)
    reads[:3] = ord("N")  # the first read after the dropped block has its own Ns
    (tmp_path / "d.fq").write_bytes(_fastq(head, L0) + _fastq(reads, L))
    st, _ = _encode_file([ctx], tmp_path / "d.fq", tmp_path, "d")
    exp = runs_of(reads, np.arange(0, n * L + 1, L, dtype=np.uint64))
    dropped = runs_of(head, np.arange(0, n0 * L0 + 1, L0, dtype=np.uint64))
    assert st["reads"] == n0 + n and st["dropped_blocks"] == 1 and len(dropped) > 1000
    assert st["nx"]["runs_in_dropped_blocks"] == len(dropped) and st["nx"]["runs"] == len(exp)
    assert st["nx"]["bases"] == int(nonacgt(head).sum() + nonacgt(reads).sum())
    runs, _ = nt.read_exceptions(tmp_path / "d.ntcx")
    assert np.array_equal(runs, exp)  # numbered from the first read that was written
    std, text = _decode_file([ctx], tmp_path, "d")
    assert std["reads"] == n and text.startswith(b">seq.1\nNNN") and text == _fasta(reads, L)
