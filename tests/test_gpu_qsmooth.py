"""Quality smoothing inside long reference matches on the GPU (k_q_smooth in quality.hip): the
sections ntc_encode_pack_fastq yields under "quality_smooth", byte for byte against the checker,
for both modes and both coders; the alphabet and the width of smoothed blocks; the count; the
way back to FASTQ text, the digests, pairs, ranges and two contexts through both command lines;
the option table; and that nothing of a smoothed call is left for the next one.

The checker is independent of the code under test: qsmooth_lib.py (numpy) restates the rule over
the CPU oracle's records, qual_lib.py / qrans_lib.py make the expected sections from the smoothed
bytes."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ntcomp_amd as nt
import qrans_lib as qr
import qsmooth_lib as qs
import qual_lib as ql
from oracle_lib import OracleIndex

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "ntcomp_amd", "ntcomp")
INVALID_ARG = 1
BR, K = 1024, 31
MS = (12, 32)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
QUALS = np.frombuffer(b"#,5<FI", dtype=np.uint8)  # '#' and ',' fall on one bin8 level, '<' on a level of its own


def _with_errors(rng, read, rate):
    r = bytearray(read)
    for p in np.flatnonzero(rng.random(len(r)) < rate):
        r[p] = b"ACGT"[(b"ACGT".index(r[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(r)


def make_batch(genome, sub):
    """About three and a half blocks of BR reads, ragged over 1..300 bases with about 1 % of
    substituted bases; mixed in: reads of random bases, error-free reads of exactly M and M - 1
    bases for both M and of 33 (the leftmost base of such a read gets a short record of its own, so
    they hold long records of 12, 31 and 32 bases), one read of 5,000 bases with errors (more than 64 records), and reads
    whose N (quality '#') stands where the genome has the substitute base, so that the masked
    read matches on.  -> (reads as the text has them, quality lines)"""
    rng = np.random.default_rng(21)
    g = genome.tobytes()
    n = 3 * BR + BR // 2
    lens = rng.integers(1, 301, n)
    flat = nt.synth_reads(genome, 2, 0, n, 300, 10_000).tobytes()
    reads = [flat[300 * i:300 * i + int(L)] for i, L in enumerate(lens)]
    for i in range(40, n, 67):  # random bases
        reads[i] = bytes(ACGT[rng.integers(0, 4, int(rng.integers(20, 200)))])
    reads[BR + 7] = _with_errors(rng, g[2000:7000], 0.02)
    sub_at = np.flatnonzero(genome == sub)
    for i in range(60, n, 97):  # N where the genome holds the substitute base
        at = int(rng.integers(0, len(g) - 120))
        r = bytearray(g[at:at + 120])
        for p in sub_at[(sub_at >= at + 40) & (sub_at < at + 80)][:3]:
            r[p - at] = ord("N")
        reads[i] = bytes(r)
    for j, i in enumerate(range(50, n, 211)):  # error-free reads of exactly M and M - 1 bases (last: none is overwritten)
        L = (12, 11, 32, 31, 33)[j % 5]
        at = int(rng.integers(0, len(g) - L))
        reads[i] = g[at:at + L]
    quals = []
    for r in reads:
        q = QUALS[rng.integers(1, len(QUALS), len(r))]
        q[rng.random(len(r)) < 0.02] = ord("#")  # some no-call scores on plain bases too
        q[np.frombuffer(r, dtype=np.uint8) == ord("N")] = ord("#")
        quals.append(q.tobytes())
    return reads, quals


def masked(reads, sub):
    return [r.replace(b"N", bytes([sub])) for r in reads]


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    e = Env()
    e.genome = nt.synth_genome(7, 20_000)
    e.ix = nt.Index.build([e.genome.tobytes()], K)
    e.ctx = nt.GpuContext(0)
    e.ctx.upload(e.ix)
    e.oracle = OracleIndex(e.ix.n, K, e.ix.rows, e.ix.C, e.ix.lcs)
    e.reads, e.quals = make_batch(e.genome, e.ctx.substitute)
    e.seq = masked(e.reads, e.ctx.substitute)
    e.text = ql.make_fastq(e.reads, e.quals)
    e.n = len(e.reads)
    e.recs, e.roff, e.offs = qs.oracle_records(e.oracle, e.seq)  # once: every test shares them
    e.mask = {M: qs.trusted(e.offs, e.recs, e.roff, M) for M in MS}
    e.smoothed = {}
    yield e
    e.ctx.close()


def _expected(e, M, mode, to=b"I"):
    """-> (the smoothed quality lines, bytes replaced), computed once per case"""
    key = (M, mode, bytes(to))
    if key not in e.smoothed:
        q = ql.mode_table(mode)[np.frombuffer(b"".join(e.quals), dtype=np.uint8)]
        out, count = qs.smooth(q, e.mask[M], mode, to)
        o = e.offs.astype(np.int64)
        e.smoothed[key] = ([out[o[r]:o[r + 1]].tobytes() for r in range(e.n)], count)
    return e.smoothed[key]


def _blob(metas):
    return b"".join(ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m)) for m in metas)


def _sections_equal(qm, qp, lines_text, mode, coder, br=BR):
    """the call's sections against the checker's over the smoothed text"""
    if coder == "rans":
        exp_m, exp_p = qr.sections(lines_text, br, mode)
        assert [qr.meta_dict(m) for m in qm] == exp_m
        assert qp == exp_p
    else:
        exp_m, exp_w = ql.sections(lines_text, br, mode)
        assert [ql.meta_dict(m) for m in qm] == exp_m
        assert qp == exp_w.astype("<u8").tobytes()
    return exp_m


# the fixture, from the oracle: no test below passes vacuously ------------------------------------
def test_fixture_conditions(env):
    e = env
    o = e.offs.astype(np.int64)
    for M in MS:
        assert 0.3 <= e.mask[M].mean() <= 0.9, (M, e.mask[M].mean())
    m = e.mask[32]
    both = sum(1 for r in range(e.n) if m[o[r]:o[r + 1]].any() and not m[o[r]:o[r + 1]].all())
    assert both >= 100, both
    q = np.frombuffer(b"".join(e.quals), dtype=np.uint8)
    on_n = np.frombuffer(b"".join(e.reads), dtype=np.uint8) == ord("N")
    assert (m & on_n & (q == ord("#"))).sum() >= 1  # a '#' on an N that was masked into a trusted match
    assert int(e.roff[BR + 8] - e.roff[BR + 7]) > 64  # the 5,000-base read loops over chunks
    lens = np.diff(o)
    exact = {int(lens[r]): r for r in range(50, e.n, 211)}  # error-free reads of exactly M and M - 1 bases, and of 33
    assert sorted(exact) == [11, 12, 31, 32, 33]
    share = lambda M, L: int(e.mask[M][o[exact[L]]:o[exact[L] + 1]].sum())
    assert (share(12, 12), share(12, 11)) == (12, 0)
    assert (share(32, 33), share(32, 32), share(32, 31)) == (32, 0, 0)  # long records of exactly M and M - 1 bases
    assert lens.min() == 1 and e.n == 3 * BR + BR // 2


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", ["pack", "rans"])
@pytest.mark.parametrize("mode", ["keep", "bin8"])
@pytest.mark.parametrize("M", MS)
def test_sections_equal_the_checker(env, M, mode, coder):
    e = env
    out = e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities=mode, quality_coder=coder,
                                  quality_smooth=M)
    qm, qp = out[-1]
    lines, count = _expected(e, M, mode)
    _sections_equal(qm, qp, ql.make_fastq(e.seq, lines), mode, coder)
    assert e.ctx.quality_smoothed == count and count > 0
    assert e.ctx.quality_smooth == 0 and e.ctx.quality_coder == 0  # held for that call only


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", ["pack", "rans"])
def test_m_larger_than_every_read_changes_nothing(env, coder):
    e = env
    plain = e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_coder=coder)
    big = e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_coder=coder,
                                  quality_smooth=5001)
    assert e.ctx.quality_smoothed == 0
    assert _blob(big[-1][0]) == _blob(plain[-1][0]) and big[-1][1] == plain[-1][1]
    assert _blob(big[0]) == _blob(plain[0]) and big[1] == plain[1]


# 3 ---------------------------------------------------------------------------------------------
def test_alphabet_and_width_follow_the_smoothed_bytes(env):
    """Three blocks of 64 reads.  0: '<' stands on trusted ground only, so it disappears: five
    symbols, four bits -> four symbols, two bits.  1: the target is a new symbol: two symbols, one
    bit -> three symbols, two bits.  2: every position trusted and above the floor: one symbol, no
    bits, no payload: every trusted position is above the floor, every other one holds the target."""
    e, br, M = env, 64, 32
    rng = np.random.default_rng(3)
    g = e.genome.tobytes()
    exact = lambda L: g[(at := int(rng.integers(0, len(g) - L))):at + L]
    rand = lambda L: bytes(ACGT[rng.integers(0, 4, L)])
    draw = lambda syms, n: rng.choice(np.frombuffer(syms, dtype=np.uint8), n)
    reads = [exact(100) if i % 2 else rand(25) for i in range(2 * br)] + [exact(60 + i) for i in range(br)]
    recs, roff, offs = qs.oracle_records(e.oracle, reads)
    mask = qs.trusted(offs, recs, roff, M)
    o = offs.astype(np.int64)
    b1, b2 = int(o[br]), int(o[2 * br])
    assert mask[:b1].any() and mask[b1:b2].any() and 0.8 < mask[b2:].mean() < 1  # (a read's leftmost bases are never trusted)
    q = np.zeros(int(o[-1]), dtype=np.uint8)
    q[:b1] = np.where(mask[:b1], ord("<"), draw(b"#5FI", b1))  # block 0: '<' on trusted ground only
    q[b1:b2] = draw(b"5F", b2 - b1)                              # block 1: two symbols, neither the target
    q[b2:] = np.where(mask[b2:], draw(b"5F<", int(o[-1]) - b2), ord("I"))  # block 2
    quals = [q[o[r]:o[r + 1]].tobytes() for r in range(len(reads))]
    text = ql.make_fastq(reads, quals)
    lines, count, mask2 = qs.smoothed(e.oracle, reads, quals, M)
    assert np.array_equal(mask, mask2) and count == int((mask & (q > ord("#"))).sum())
    before = [(m["n_syms"], m["width"]) for m in ql.sections(text, br)[0]]
    assert before == [(5, 4), (2, 1), (4, 2)]
    for coder in ("pack", "rans"):
        out = e.ctx.encode_pack_fastq(text, len(reads), block_reads=br, qualities="keep", quality_coder=coder,
                                      quality_smooth=M)
        qm, qp = out[-1]
        exp = _sections_equal(qm, qp, ql.make_fastq(reads, lines), "keep", coder, br)
        assert [(m["n_syms"], m["width"]) for m in exp] == [(4, 2), (3, 2), (1, 0)]
        assert exp[0]["alphabet"] == b"#5FI" and exp[1]["alphabet"] == b"5FI" and exp[2]["alphabet"] == b"I"
        assert qm[2].payload_bytes == 0 and e.ctx.quality_smoothed == count


# 4 ---------------------------------------------------------------------------------------------
def test_count_and_the_encoded_blocks_are_untouched(env):
    e = env
    bare = e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep")
    out = e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_smooth=32)
    assert e.ctx.quality_smoothed == _expected(e, 32, "keep")[1]
    assert _blob(out[0]) == _blob(bare[0]) and out[1] == bare[1]
    assert out[3].tobytes() == bare[3].tobytes() and len(out[3]) > 0  # the exception runs
    # another target: the count is that of the positions, not of the bytes that differ
    e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_smooth=32,
                            quality_smooth_to=b"5")
    assert e.ctx.quality_smoothed == _expected(e, 32, "keep", b"5")[1] == _expected(e, 32, "keep")[1]
    assert e.ctx.quality_smooth_to == b"I"


# 5 ---------------------------------------------------------------------------------------------
def test_decode_prints_the_smoothed_text(env):
    e = env
    for mode, coder in (("keep", "pack"), ("bin8", "rans")):
        out = e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="mask", qualities=mode, quality_coder=coder,
                                      quality_smooth=32)
        qm, qp = out[-1]
        arr = (nt.BlockMeta * len(out[0]))(*out[0])
        assert e.ctx.unpack(arr, out[1], len(out[0]))[0] == len(out[0])
        e.ctx.set_qualities(qm, qp)
        assert e.ctx.decode_fasta_unpacked(first_id=1) == qs.fastq_text(e.seq, _expected(e, 32, mode)[0])


def _cli(which, *args, stdout=subprocess.PIPE):
    cmd = [NATIVE] if which == "native" else [sys.executable, "-m", "ntcomp_amd"]
    envv = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + list(args), stdout=stdout, stderr=subprocess.PIPE, env=envv, timeout=300)


@pytest.fixture(scope="module")
def files(env, tmp_path_factory):
    """The index and the batch on disk, with an even number of reads for the paired test and no
    N (the command lines run under --non-acgt error)."""
    e, d = env, tmp_path_factory.mktemp("qsmooth")
    e.ix.save(str(d / "idx"))
    (d / "r.fq").write_bytes(ql.make_fastq(e.seq, e.quals))
    return d


def _encode_cli(which, d, name, *flags, devices="0", fq="r.fq"):
    with open(d / (name + ".dat"), "wb") as fo:
        r = _cli(which, "encode", "-i", str(d / "idx"), "--devices", devices, "--deflate", "zlib", "--qualities", "keep",
                 "--quality-file", str(d / (name + ".q")), "--digest-file", str(d / (name + ".d")), "--stats", *flags,
                 str(d / fq), stdout=fo)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_digests_verify_and_stats(env, files, which):
    e, d = env, files
    r = _encode_cli(which, d, "s_" + which, "--quality-smooth")  # M = 32 when left out
    lines, count = _expected(e, 32, "keep")
    assert b'"quality_smooth": 32' in r.stderr and b'"quality_smooth_to": "I"' in r.stderr
    assert b'"q_smoothed": %d' % count in r.stderr, r.stderr
    _encode_cli(which, d, "u_" + which)
    base = ["-i", str(d / "idx")]
    sm = [str(d / f"s_{which}.dat")]
    r = _cli(which, "decode", *base, "--quality-file", str(d / f"s_{which}.q"), "--digest-file", str(d / f"s_{which}.d"), *sm)
    assert r.returncode == 0 and r.stdout == qs.fastq_text(e.seq, lines), r.stderr
    r = _cli(which, "verify", *base, "--quality-file", str(d / f"s_{which}.q"), "--digest-file", str(d / f"s_{which}.d"), *sm)
    assert r.returncode == 0 and b"checked seq,qual" in r.stdout, r.stderr
    # the digests of an unsmoothed encode: the bases agree, the qual component does not
    assert (d / f"s_{which}.dat").read_bytes() == (d / f"u_{which}.dat").read_bytes()
    r = _cli(which, "verify", *base, "--quality-file", str(d / f"s_{which}.q"), "--digest-file", str(d / f"u_{which}.d"), *sm)
    assert r.returncode != 0 and b"component qual" in r.stderr, r.stderr


# 6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["native", "python"])
def test_cli_pairs_and_a_range_of_reads(env, files, which):
    e, d = env, files
    lines = _expected(e, 12, "keep", b"5")[0]
    _encode_cli(which, d, "p_" + which, "--quality-smooth", "12", "--quality-smooth-to", "5", "--interleaved",
                "--mate-check", "off")
    a, b = 1501, 2600  # across the block boundary of the 5,000-base read's neighbours
    r = _cli(which, "decode", "-i", str(d / "idx"), "--quality-file", str(d / f"p_{which}.q"), "--reads", f"{a}-{b}",
             str(d / f"p_{which}.dat"))
    assert r.returncode == 0, r.stderr
    assert r.stdout == qs.fastq_text(e.seq[a - 1:b], lines[a - 1:b], first_id=a)


# 7 ---------------------------------------------------------------------------------------------
def test_two_contexts_write_the_same_side_file(env, files):
    """Two blocks of the pipeline (65,536 reads and the rest), one per call, so that with
    --devices 0,0 each context takes one; and the first block's section against the checker."""
    e, d = env, files
    rng = np.random.default_rng(77)
    g = e.genome.tobytes()
    n, L = 65_536 + 700, 40
    starts = rng.integers(0, len(g) - L, n)
    reads = [g[s:s + L] for s in starts.tolist()]
    for i in range(0, n, 3):  # an error in a third of them, at 1/4 of the read: a record of >= 29 bases is left
        r = bytearray(reads[i])
        r[10] = b"ACGT"[(b"ACGT".index(r[10]) + 1) % 4]
        reads[i] = bytes(r)
    q = QUALS[rng.integers(0, len(QUALS), n * L)].tobytes()
    quals = [q[i * L:(i + 1) * L] for i in range(n)]
    (d / "big.fq").write_bytes(ql.make_fastq(reads, quals))
    r1 = _encode_cli("native", d, "one", "--quality-smooth", "16", "--blocks-per-batch", "1", fq="big.fq")
    r2 = _encode_cli("native", d, "two", "--quality-smooth", "16", "--blocks-per-batch", "1", devices="0,0", fq="big.fq")
    for ext in (".q", ".d", ".dat"):
        assert (d / ("one" + ext)).read_bytes() == (d / ("two" + ext)).read_bytes(), ext
    lines, count, mask = qs.smoothed(e.oracle, reads[-700:], quals[-700:], 16)  # the last block, by the checker
    assert 0 < count < 700 * L
    mode, metas, pay = nt.read_qualities(d / "two.q")
    exp_m, exp_w = ql.sections(ql.make_fastq(reads[-700:], lines), 65_536)
    assert len(metas) == 2 and {k: v for k, v in ql.meta_dict(metas[1]).items() if k != "payload_off"} == \
        {k: v for k, v in exp_m[0].items() if k != "payload_off"}
    assert pay[metas[1].payload_off:metas[1].payload_off + metas[1].payload_bytes] == exp_w.astype("<u8").tobytes()
    tot = [int(re.search(rb'"q_smoothed": (\d+)', r.stderr).group(1)) for r in (r1, r2)]
    assert tot[0] == tot[1] > count  # the sum over both contexts is the sum over one


# 8 ---------------------------------------------------------------------------------------------
def test_option_table(env):
    e = env
    c = nt.GpuContext(0)
    try:
        def set_(key, v):
            rc = c.L.ntc_ctx_set_option(c.h, key.encode(), v)
            return rc, c.L.ntc_last_error(c.h).decode()

        assert (c.quality_smooth, c.quality_smooth_to, c.quality_smoothed) == (0, b"I", 0)
        msg = "quality_smooth must be 0 (off) or 12..16777215"
        for v in (0, 12, 32, 16777215):
            assert set_("quality_smooth", v)[0] == 0 and c.quality_smooth == v
        for v in (-1, 1, 11, 16777216):
            assert set_("quality_smooth", v) == (INVALID_ARG, msg), v
        assert c.quality_smooth == 16777215  # a refused value changes nothing
        msg = "quality_smooth_to must be a byte in '$'..'~'"
        for v in (ord("$"), ord("~"), ord("I")):
            assert set_("quality_smooth_to", v)[0] == 0 and c.quality_smooth_to == bytes([v])
        for v in (ord("#"), 127, 0, -1):
            assert set_("quality_smooth_to", v) == (INVALID_ARG, msg), v
        assert set_("quality_smoothed", 0) == (INVALID_ARG, "unknown option quality_smoothed")  # read-only
        # at the call: refused under qualities 0, and under bin8 for a target whose level is that of '#'
        c.share_index(e.ctx)
        c.quality_smooth = 32
        with pytest.raises(nt.NtcError) as err:
            c.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep")
        assert err.value.code == INVALID_ARG and "quality_smooth needs qualities 1 (keep) or 2 (bin8)" in str(err.value)
        for to in (b"$", b"(", b"*"):
            with pytest.raises(nt.NtcError) as err:
                c.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="bin8", quality_smooth_to=to)
            assert err.value.code == INVALID_ARG and "quality_smooth_to" in str(err.value)
            assert c.qualities() == ([], b"")  # a refused call leaves no sections
        c.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="bin8", quality_smooth_to=b"+")
        assert c.quality_smoothed == _expected(e, 32, "bin8")[1]
        c.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_smooth_to=b"$")
        assert c.quality_smoothed == _expected(e, 32, "keep")[1]
    finally:
        c.close()


# 9 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", ["pack", "rans"])
def test_no_state_is_left_for_the_next_call(env, coder):
    e = env
    fresh = nt.GpuContext(0)
    try:
        fresh.upload(e.ix)
        ref = fresh.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_coder=coder,
                                      digests=True)
    finally:
        fresh.close()
    e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_coder=coder,
                            quality_smooth=12, digests=True)
    assert e.ctx.quality_smoothed > 0
    got = e.ctx.encode_pack_fastq(e.text, e.n, block_reads=BR, non_acgt="keep", qualities="keep", quality_coder=coder,
                                  digests=True)
    assert e.ctx.quality_smoothed == 0
    assert _blob(got[-2][0]) == _blob(ref[-2][0]) and got[-2][1] == ref[-2][1]
    assert _blob(got[-1]) == _blob(ref[-1])  # the digests too
    _sections_equal(*got[-2], e.text, "keep", coder)
